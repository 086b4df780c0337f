/*
 * oracle/ref/ref_driver.c -- TEST INFRASTRUCTURE ONLY.
 *
 * A main() of our own over the reference sampler's public API (the functions its mcmc.h declares),
 * linked with the unmodified reference mcmc.c (oracle/Makefile: _ref/ref_driver; the reference's
 * own main is renamed away on the compiler's command line, it is not called).  Two modes:
 *
 *   ref_driver chain <manycd> <tb> <ts> < dataset        seed from GSL_RNG_SEED
 *     mcmc_init, mcmc_readmodel, mcmc_randomize, mcmc_consistent, tb burn-in calls of mcmc_sample,
 *     then ts calls.  Prints the state after mcmc_randomize ("state init") and after each of the ts
 *     calls ("state <k>"): a, b, pi as integers, every c[i], d[i] and loglik as the 16 hex digits of
 *     the double's bit pattern, and the totals t0a f0a t1a f1a.  Then "words <n>", the 32-bit words
 *     the generator produced, and "consistent <flag>".  Exit status: mcmc_consistent's at the end.
 *
 *   ref_driver unit < cases
 *     each case: L o c d u x[0] .. x[L-1]   (c, d, u as 16 hex digits; x = walk-order bits)
 *     runs mcmc_auxa (which calls mcmc_logtop and mcmc_randompick) over x with b = L from limit
 *     a = o, the uniform that mcmc_randompick draws forced to u through the stand-in's queue.
 *     Prints "pick <a> counts <t0 f0 t1 f1> q <L + 1 hex doubles>" (q = the probabilities).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <gsl/gsl_math.h>
#include <gsl/gsl_matrix.h>
#include <gsl/gsl_vector.h>
#include <gsl/gsl_permutation.h>
#include <gsl/gsl_rng.h>
#include <gsl/gsl_randist.h>
#include "mcmc.h"

extern gsl_rng *r; /* the reference's global generator (mcmc_init allocates it) */

static void put_bits(double v)
{
  uint64_t b;
  memcpy(&b, &v, 8);
  printf(" %016llx", (unsigned long long)b);
}

static int get_bits(double *v)
{
  unsigned long long b;
  if (scanf("%llx", &b) != 1) return 0;
  uint64_t w = b;
  memcpy(v, &w, 8);
  return 1;
}

static void put_state(const mcmc_model *x, const char *tag)
{
  int i;
  printf("state %s\na", tag);
  for (i = 0; i < x->M; i++) printf(" %d", gsl_vector_int_get(x->a, i));
  printf("\nb");
  for (i = 0; i < x->M; i++) printf(" %d", gsl_vector_int_get(x->b, i));
  printf("\npi");
  for (i = 0; i < x->N; i++) printf(" %d", (int)gsl_permutation_get(x->pi, i));
  printf("\nc");
  for (i = 0; i < x->M; i++) put_bits(gsl_vector_get(x->c, i));
  printf("\nd");
  for (i = 0; i < x->M; i++) put_bits(gsl_vector_get(x->d, i));
  printf("\nloglik");
  put_bits(x->loglik);
  printf("\ncounts %d %d %d %d\n", x->t0a, x->f0a, x->t1a, x->f1a);
}

static int chain_mode(int manycd, int tb, int ts)
{
  mcmc_model x;
  char tag[32];
  int i, flag;
  mcmc_init();
  mcmc_readmodel(&x, stdin, manycd);
  mcmc_randomize(&x);
  put_state(&x, "init");
  mcmc_consistent(&x);
  for (i = 0; i < tb; i++) mcmc_sample(&x);
  for (i = 0; i < ts; i++) {
    mcmc_sample(&x);
    snprintf(tag, sizeof tag, "%d", i);
    put_state(&x, tag);
  }
  printf("words %llu\n", gsl_standin_words(r));
  flag = mcmc_consistent(&x);
  printf("consistent %d\n", flag);
  mcmc_freemodel(&x);
  mcmc_free();
  return flag;
}

static int unit_mode(void)
{
  int L, o, i;
  mcmc_init();
  while (scanf("%d %d", &L, &o) == 2) {
    double c, d, u;
    int a = o, t0 = 0, f0 = 0, t1 = 0, f1 = 0;
    if (L < 0 || o < 0 || o > L || !get_bits(&c) || !get_bits(&d) || !get_bits(&u)) return 2;
    gsl_vector_int *v = gsl_vector_int_alloc(L);
    gsl_vector *q = gsl_vector_calloc(L + 1);
    gsl_vector_int *dt0 = gsl_vector_int_alloc(L + 1), *df0 = gsl_vector_int_alloc(L + 1);
    gsl_vector_int *dt1 = gsl_vector_int_alloc(L + 1), *df1 = gsl_vector_int_alloc(L + 1);
    for (i = 0; i < L; i++) {
      int bit;
      if (scanf("%d", &bit) != 1) return 2;
      gsl_vector_int_set(v, i, bit);
    }
    gsl_standin_force_uniform(u);
    mcmc_auxa(v, L, c, d, &a, &t0, &f0, &t1, &f1, q, dt0, df0, dt1, df1);
    printf("pick %d counts %d %d %d %d q", a, t0, f0, t1, f1);
    for (i = 0; i <= L; i++) put_bits(gsl_vector_get(q, i));
    printf("\n");
    gsl_vector_int_free(v); gsl_vector_free(q);
    gsl_vector_int_free(dt0); gsl_vector_int_free(df0); gsl_vector_int_free(dt1); gsl_vector_int_free(df1);
  }
  mcmc_free();
  return 0;
}

#undef main /* the command line renames the reference's main; this one is the program's */
int main(int argc, char *argv[])
{
  int manycd, tb, ts;
  if (argc == 2 && !strcmp(argv[1], "unit")) return unit_mode();
  if (argc >= 5 && !strcmp(argv[1], "chain") && sscanf(argv[2], "%d", &manycd) == 1 &&
      sscanf(argv[3], "%d", &tb) == 1 && tb >= 0 && sscanf(argv[4], "%d", &ts) == 1 && ts >= 0)
    return chain_mode(manycd, tb, ts);
  fprintf(stderr, "usage: %s chain <manycd> <tb> <ts> < dataset | %s unit < cases\n", argv[0], argv[0]);
  return 2;
}
