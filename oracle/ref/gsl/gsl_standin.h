/*
 * oracle/ref/gsl/gsl_standin.h -- TEST INFRASTRUCTURE ONLY.
 *
 * A stand-in for the part of the GNU Scientific Library that the reference sampler's
 * C_Implementation/mcmc.c calls, written from GSL's documented API (the GSL reference manual:
 * "Vectors and Matrices", "Permutations", "Random Number Generation", "Random Number
 * Distributions").  With -I oracle/ref the reference's `#include <gsl/gsl_*.h>` lines find the six
 * one-line headers next to this file, so the unmodified reference source compiles and runs where
 * GSL is not installed (oracle/Makefile: _ref/mcmc_ref, _ref/ref_driver).
 *
 * Containers are implemented here.  Every accessor checks its index and abort()s on a bad one,
 * as GSL does with range checking on and its default error handler.
 * The generator and the distributions forward to the restatement in ../../om_gsl.h
 * (om_rng_*, om_uniform*, om_shuffle, om_choose, om_beta): what runs under this header is the
 * reference's own program text, what it does NOT check is om_gsl.h against real GSL.
 *
 * State shared between translation units (the default seed, the forced-uniform queue of the unit
 * driver) is defined once, in the file that defines GSL_STANDIN_IMPLEMENTATION (gsl_standin.c).
 */
#ifndef GSL_STANDIN_H
#define GSL_STANDIN_H
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../om_gsl.h"

#define GSL_SUCCESS 0
#define GSL_FAILURE (-1)
#define GSL_MAX(a, b) ((a) > (b) ? (a) : (b))
#define GSL_MIN(a, b) ((a) < (b) ? (a) : (b))

static inline void gsl_standin_die(const char *what, size_t i, size_t n)
{
  fprintf(stderr, "gsl: %s: index %lu out of range (size %lu)\n", what, (unsigned long)i, (unsigned long)n);
  abort();
}

static inline void *gsl_standin_alloc(size_t count, size_t size, int zero)
{
  void *p = zero ? calloc(count ? count : 1, size) : malloc((count ? count : 1) * size);
  if (!p) { fprintf(stderr, "gsl: out of memory\n"); abort(); }
  return p;
}

/* ------------------------------------------------------------------ gsl_vector (double) */
typedef struct { size_t size; size_t stride; double *data; int owner; } gsl_vector;

static inline gsl_vector *gsl_standin_vector_new(size_t n, int zero)
{
  gsl_vector *v = (gsl_vector *)gsl_standin_alloc(1, sizeof *v, 1);
  v->size = n; v->stride = 1; v->owner = 1;
  v->data = (double *)gsl_standin_alloc(n, sizeof(double), zero);
  return v;
}
static inline gsl_vector *gsl_vector_alloc(size_t n) { return gsl_standin_vector_new(n, 0); }
static inline gsl_vector *gsl_vector_calloc(size_t n) { return gsl_standin_vector_new(n, 1); }
static inline void gsl_vector_free(gsl_vector *v) { if (v) { if (v->owner) free(v->data); free(v); } }
static inline double gsl_vector_get(const gsl_vector *v, size_t i)
{
  if (i >= v->size) gsl_standin_die("gsl_vector_get", i, v->size);
  return v->data[i * v->stride];
}
static inline void gsl_vector_set(gsl_vector *v, size_t i, double x)
{
  if (i >= v->size) gsl_standin_die("gsl_vector_set", i, v->size);
  v->data[i * v->stride] = x;
}

/* --------------------------------------------------------------------- gsl_vector_int */
typedef struct { size_t size; size_t stride; int *data; int owner; } gsl_vector_int;
typedef struct { gsl_vector_int vector; } gsl_vector_int_view;

static inline gsl_vector_int *gsl_standin_vector_int_new(size_t n, int zero)
{
  gsl_vector_int *v = (gsl_vector_int *)gsl_standin_alloc(1, sizeof *v, 1);
  v->size = n; v->stride = 1; v->owner = 1;
  v->data = (int *)gsl_standin_alloc(n, sizeof(int), zero);
  return v;
}
static inline gsl_vector_int *gsl_vector_int_alloc(size_t n) { return gsl_standin_vector_int_new(n, 0); }
static inline gsl_vector_int *gsl_vector_int_calloc(size_t n) { return gsl_standin_vector_int_new(n, 1); }
static inline void gsl_vector_int_free(gsl_vector_int *v) { if (v) { if (v->owner) free(v->data); free(v); } }
static inline int gsl_vector_int_get(const gsl_vector_int *v, size_t i)
{
  if (i >= v->size) gsl_standin_die("gsl_vector_int_get", i, v->size);
  return v->data[i * v->stride];
}
static inline void gsl_vector_int_set(gsl_vector_int *v, size_t i, int x)
{
  if (i >= v->size) gsl_standin_die("gsl_vector_int_set", i, v->size);
  v->data[i * v->stride] = x;
}
static inline int gsl_vector_int_reverse(gsl_vector_int *v)
{
  for (size_t i = 0; i < v->size / 2; i++) {
    const size_t j = v->size - 1 - i;
    const int t = v->data[i * v->stride];
    v->data[i * v->stride] = v->data[j * v->stride];
    v->data[j * v->stride] = t;
  }
  return GSL_SUCCESS;
}

/* --------------------------------------------------------------------- gsl_matrix_int */
typedef struct { size_t size1; size_t size2; size_t tda; int *data; int owner; } gsl_matrix_int;

static inline gsl_matrix_int *gsl_standin_matrix_int_new(size_t n1, size_t n2, int zero)
{
  gsl_matrix_int *m = (gsl_matrix_int *)gsl_standin_alloc(1, sizeof *m, 1);
  m->size1 = n1; m->size2 = n2; m->tda = n2; m->owner = 1;
  m->data = (int *)gsl_standin_alloc(n1 * n2, sizeof(int), zero);
  return m;
}
static inline gsl_matrix_int *gsl_matrix_int_alloc(size_t n1, size_t n2) { return gsl_standin_matrix_int_new(n1, n2, 0); }
static inline gsl_matrix_int *gsl_matrix_int_calloc(size_t n1, size_t n2) { return gsl_standin_matrix_int_new(n1, n2, 1); }
static inline void gsl_matrix_int_free(gsl_matrix_int *m) { if (m) { if (m->owner) free(m->data); free(m); } }
static inline int gsl_matrix_int_get(const gsl_matrix_int *m, size_t i, size_t j)
{
  if (i >= m->size1) gsl_standin_die("gsl_matrix_int_get (row)", i, m->size1);
  if (j >= m->size2) gsl_standin_die("gsl_matrix_int_get (column)", j, m->size2);
  return m->data[i * m->tda + j];
}
static inline void gsl_matrix_int_set(gsl_matrix_int *m, size_t i, size_t j, int x)
{
  if (i >= m->size1) gsl_standin_die("gsl_matrix_int_set (row)", i, m->size1);
  if (j >= m->size2) gsl_standin_die("gsl_matrix_int_set (column)", j, m->size2);
  m->data[i * m->tda + j] = x;
}
/* a view of row i: the matrix's own storage, not a copy */
static inline gsl_vector_int_view gsl_matrix_int_row(gsl_matrix_int *m, size_t i)
{
  gsl_vector_int_view w;
  if (i >= m->size1) gsl_standin_die("gsl_matrix_int_row", i, m->size1);
  w.vector.size = m->size2; w.vector.stride = 1; w.vector.data = m->data + i * m->tda; w.vector.owner = 0;
  return w;
}
/* copy column j into v (v->size must equal the number of rows) */
static inline int gsl_matrix_int_get_col(gsl_vector_int *v, const gsl_matrix_int *m, size_t j)
{
  if (j >= m->size2) gsl_standin_die("gsl_matrix_int_get_col", j, m->size2);
  if (v->size != m->size1) gsl_standin_die("gsl_matrix_int_get_col (vector length)", v->size, m->size1);
  for (size_t i = 0; i < m->size1; i++) v->data[i * v->stride] = m->data[i * m->tda + j];
  return GSL_SUCCESS;
}

/* -------------------------------------------------------------------- gsl_permutation */
typedef struct { size_t size; size_t *data; } gsl_permutation;

static inline gsl_permutation *gsl_permutation_alloc(size_t n)
{
  gsl_permutation *p = (gsl_permutation *)gsl_standin_alloc(1, sizeof *p, 1);
  p->size = n;
  p->data = (size_t *)gsl_standin_alloc(n, sizeof(size_t), 0);
  return p;
}
/* calloc: initialised to the identity */
static inline gsl_permutation *gsl_permutation_calloc(size_t n)
{
  gsl_permutation *p = gsl_permutation_alloc(n);
  for (size_t i = 0; i < n; i++) p->data[i] = i;
  return p;
}
static inline void gsl_permutation_free(gsl_permutation *p) { if (p) { free(p->data); free(p); } }
static inline size_t gsl_permutation_get(const gsl_permutation *p, size_t i)
{
  if (i >= p->size) gsl_standin_die("gsl_permutation_get", i, p->size);
  return p->data[i];
}
/* GSL_SUCCESS for a permutation of 0..size-1; otherwise GSL reports through its error handler,
   whose default aborts */
static inline int gsl_permutation_valid(const gsl_permutation *p)
{
  for (size_t i = 0; i < p->size; i++) {
    if (p->data[i] >= p->size) { fprintf(stderr, "gsl: permutation index outside range\n"); abort(); }
    for (size_t j = 0; j < i; j++)
      if (p->data[i] == p->data[j]) { fprintf(stderr, "gsl: duplicate permutation index\n"); abort(); }
  }
  return GSL_SUCCESS;
}
static inline int gsl_permutation_inverse(gsl_permutation *inv, const gsl_permutation *p)
{
  if (inv->size != p->size) gsl_standin_die("gsl_permutation_inverse (length)", inv->size, p->size);
  for (size_t i = 0; i < p->size; i++) {
    if (p->data[i] >= p->size) gsl_standin_die("gsl_permutation_inverse", p->data[i], p->size);
    inv->data[p->data[i]] = i;
  }
  return GSL_SUCCESS;
}
/* apply p to v in place: v'[i] = v[p[i]] */
static inline int gsl_permute_vector_int(const gsl_permutation *p, gsl_vector_int *v)
{
  if (v->size != p->size) gsl_standin_die("gsl_permute_vector_int (length)", v->size, p->size);
  int *t = (int *)gsl_standin_alloc(v->size, sizeof(int), 0);
  for (size_t i = 0; i < v->size; i++) {
    if (p->data[i] >= v->size) gsl_standin_die("gsl_permute_vector_int", p->data[i], v->size);
    t[i] = v->data[p->data[i] * v->stride];
  }
  for (size_t i = 0; i < v->size; i++) v->data[i * v->stride] = t[i];
  free(t);
  return GSL_SUCCESS;
}

/* ---------------------------------------------------------------------------- gsl_rng */
typedef struct { const char *name; } gsl_rng_type;
typedef struct { const gsl_rng_type *type; om_rng state; } gsl_rng;

extern const gsl_rng_type *gsl_rng_default;
extern unsigned long int gsl_rng_default_seed;

/* Hooks of the unit driver (not GSL): values queued here are what the next gsl_rng_uniform /
   gsl_rng_uniform_pos calls return, before the generator is asked again; and the number of
   32-bit words the generator has produced so far. */
void gsl_standin_force_uniform(double u);
unsigned long long gsl_standin_words(const gsl_rng *r);

const gsl_rng_type *gsl_rng_env_setup(void);
gsl_rng *gsl_rng_alloc(const gsl_rng_type *T);
void gsl_rng_free(gsl_rng *r);
double gsl_rng_uniform(gsl_rng *r);
double gsl_rng_uniform_pos(gsl_rng *r);
unsigned long int gsl_rng_uniform_int(gsl_rng *r, unsigned long int n);
void gsl_ran_shuffle(gsl_rng *r, void *base, size_t n, size_t size);
void *gsl_ran_choose(gsl_rng *r, void *dest, size_t k, void *src, size_t n, size_t size);
double gsl_ran_beta(gsl_rng *r, double a, double b);

#ifdef GSL_STANDIN_IMPLEMENTATION
static const gsl_rng_type gsl_standin_mt19937 = {"mt19937"};
const gsl_rng_type *gsl_rng_default = &gsl_standin_mt19937;
unsigned long int gsl_rng_default_seed = 0;

#define GSL_STANDIN_QUEUE 16
static double gsl_standin_queue[GSL_STANDIN_QUEUE];
static int gsl_standin_qhead = 0, gsl_standin_qlen = 0;

void gsl_standin_force_uniform(double u)
{
  if (gsl_standin_qlen == GSL_STANDIN_QUEUE) { fprintf(stderr, "gsl stand-in: forced-uniform queue full\n"); abort(); }
  gsl_standin_queue[(gsl_standin_qhead + gsl_standin_qlen++) % GSL_STANDIN_QUEUE] = u;
}
static int gsl_standin_forced(double *u)
{
  if (!gsl_standin_qlen) return 0;
  *u = gsl_standin_queue[gsl_standin_qhead];
  gsl_standin_qhead = (gsl_standin_qhead + 1) % GSL_STANDIN_QUEUE;
  gsl_standin_qlen--;
  return 1;
}
unsigned long long gsl_standin_words(const gsl_rng *r) { return r->state.ndraw; }

/* GSL_RNG_TYPE / GSL_RNG_SEED from the environment, echoed on stderr when set.  Only mt19937
   (GSL's default) exists here: another generator's name ends the program with status 1. */
const gsl_rng_type *gsl_rng_env_setup(void)
{
  unsigned long seed = 0;
  if (om_rng_env_setup(&seed)) exit(1);
  gsl_rng_default_seed = seed;
  gsl_rng_default = &gsl_standin_mt19937;
  return gsl_rng_default;
}
/* a new generator, seeded with gsl_rng_default_seed */
gsl_rng *gsl_rng_alloc(const gsl_rng_type *T)
{
  gsl_rng *r = (gsl_rng *)gsl_standin_alloc(1, sizeof *r, 1);
  r->type = T;
  om_rng_seed(&r->state, gsl_rng_default_seed);
  return r;
}
void gsl_rng_free(gsl_rng *r) { free(r); }
double gsl_rng_uniform(gsl_rng *r)
{
  double u;
  return gsl_standin_forced(&u) ? u : om_uniform(&r->state);
}
double gsl_rng_uniform_pos(gsl_rng *r)
{
  double u;
  return gsl_standin_forced(&u) ? u : om_uniform_pos(&r->state);
}
unsigned long int gsl_rng_uniform_int(gsl_rng *r, unsigned long int n)
{
  if (n == 0 || n > 0xffffffffUL) {
    fprintf(stderr, "gsl: gsl_rng_uniform_int: invalid n, either 0 or exceeds maximum value of generator\n");
    abort();
  }
  return om_uniform_int(&r->state, n);
}
void gsl_ran_shuffle(gsl_rng *r, void *base, size_t n, size_t size)
{
  if (n) om_shuffle(&r->state, base, n, size);
}
void *gsl_ran_choose(gsl_rng *r, void *dest, size_t k, void *src, size_t n, size_t size)
{
  if (om_choose(&r->state, dest, k, src, n, size)) { fprintf(stderr, "gsl: gsl_ran_choose: k is greater than n\n"); abort(); }
  return dest;
}
double gsl_ran_beta(gsl_rng *r, double a, double b) { return om_beta(&r->state, a, b); }
#endif /* GSL_STANDIN_IMPLEMENTATION */

#endif
