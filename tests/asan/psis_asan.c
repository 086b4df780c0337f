/* Stand-alone driver for csrc/sr_psis.h under AddressSanitizer + UndefinedBehaviorSanitizer (make
 * build/asan/psis_asan, then run it; no GPU, no Python).  Every buffer is malloc'ed at its exact size, so a read past
 * y [n], G [m] or L [n] is caught.  Random tails of every length class, read forwards and -- as the finish kernel
 * reads its heap -- backwards through a negative stride, and the degenerate ones: all equal, ties up to the first
 * quartile, n < 5 with no tables, ratios at e^600, a tail that is not sorted, zeros, infinities and NaNs.  Exit status
 * 0 and the line "psis_asan ok" when nothing was flagged and every result is a shape that is finite or +inf with an
 * elpd that is a number wherever the input was a legal tail. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_psis.h"

static const sr_mtab TAB = {(const uint64_t *)sr_exp_tab, sr_log_tab};
static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;

static double uni(void)
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) * 0x1p-53;
}

static int cmp(const void *a, const void *b)
{
  const double x = *(const double *)a, y = *(const double *)b;
  return x < y ? -1 : (x > y ? 1 : 0);
}

static long runs = 0, smoothed = 0, bad = 0;

/* y [n] ascending (or whatever the case holds), forwards and reversed through stride -1: the same bits */
static void one(int64_t T, int32_t n, const double *vals, double r_cut, double Sr, int legal)
{
  int32_t m = 30 + sr_psis_isqrt(n);
  double *y = (double *)malloc(sizeof(double) * (n ? n : 1)), *rev = (double *)malloc(sizeof(double) * (n ? n : 1));
  double *G = n >= 5 ? (double *)malloc(sizeof(double) * m) : NULL, *L = n >= 5 ? (double *)malloc(sizeof(double) * n) : NULL;
  for (int32_t i = 0; i < n; i++) { y[i] = vals[i]; rev[n - 1 - i] = vals[i]; }
  if (n >= 5) {
    for (int32_t j = 1; j <= m; j++) G[j - 1] = (1.0 - sqrt((double)m / ((double)j - 0.5))) / 3.0;
    for (int32_t j = 1; j <= n; j++) L[j - 1] = log(1.0 - ((double)j - 0.5) / (double)n);
  }
  double k1, e1, k2, e2;
  sr_psis_tail(y, 1, n, r_cut, Sr, T, G, m, L, &TAB, &k1, &e1);
  sr_psis_tail(rev + (n ? n - 1 : 0), -1, n, r_cut, Sr, T, G, m, L, &TAB, &k2, &e2);
  runs++;
  if (sr_bits(k1) != sr_bits(k2) || sr_bits(e1) != sr_bits(e2)) { bad++; printf("stride mismatch n=%d\n", n); }
  if (k1 != k1 || (legal && e1 != e1)) { bad++; printf("NaN result n=%d k=%g e=%g\n", n, k1, e1); }
  if (k1 < INFINITY) smoothed++;
  free(y); free(rev); free(G); free(L);
}

int main(void)
{
  static const int64_t Ts[] = {3, 24, 25, 30, 40, 225, 1000, 8000, 1864135};
  for (size_t c = 0; c < sizeof(Ts) / sizeof(Ts[0]); c++) {
    const int64_t T = Ts[c];
    const int32_t n = sr_psis_tail_len(T);
    double *r = (double *)malloc(sizeof(double) * T);
    for (int trial = 0; trial < (T > 100000 ? 2 : 30); trial++) {
      const double shape = 0.05 + 2.5 * uni(), shift = 3.0 * uni();
      double Sr = 0.0;
      for (int64_t i = 0; i < T; i++) {
        const double u = uni();
        r[i] = trial % 3 == 0 ? pow(1.0 - u, -shape) + shift
             : trial % 3 == 1 ? 1.0 / (u < 0.1 ? 0.001 + 0.1 * uni() : 0.5 + 0.499 * uni())
                              : 1.0 + u * u * pow(10.0, (double)(trial % 7) - 3.0);
        Sr += r[i];
      }
      qsort(r, (size_t)T, sizeof(double), cmp);
      one(T, n, r + (T - n), r[T - n - 1], Sr, 1);
    }
    /* degenerate tails of this length */
    double *y = (double *)malloc(sizeof(double) * (n ? n : 1));
    const int32_t q = (n + 2) / 4;
    for (int32_t i = 0; i < n; i++) y[i] = 3.5;
    one(T, n, y, 3.5, 3.5 * (double)T, 1);                                  /* all equal */
    for (int32_t i = 0; i < n; i++) y[i] = i < q ? 3.5 : 4.0 + (double)i;
    one(T, n, y, 3.5, 1e7, 1);                                              /* ties up to index q */
    if (q >= 1 && n >= 5) { y[q - 1] = nextafter(3.5, 4.0); one(T, n, y, 3.5, 1e7, 1); }   /* up to q - 1 */
    for (int32_t i = 0; i < n; i++) y[i] = exp(600.0) * (0.5 + 0.5 * (double)(i + 1) / (double)n);
    one(T, n, y, 1.0, exp(600.0) * (double)n, 1);                           /* the domain's edge */
    for (int32_t i = 0; i < n; i++) y[i] = exp(600.0);
    one(T, n, y, exp(600.0), exp(600.0) * (double)T, 1);
    for (int32_t i = 0; i < n; i++) y[i] = (double)(n - i);                 /* not sorted: any result, no fault */
    one(T, n, y, 0.5, 1e9, 0);
    for (int32_t i = 0; i < n; i++) y[i] = 0.0;
    one(T, n, y, 0.0, 0.0, 0);
    for (int32_t i = 0; i < n; i++) y[i] = i % 2 ? INFINITY : 1.0 + (double)i;
    one(T, n, y, 1.0, INFINITY, 0);
    for (int32_t i = 0; i < n; i++) y[i] = i == n / 2 ? NAN : 2.0 + (double)i;
    one(T, n, y, 1.0, NAN, 0);
    for (int32_t i = 0; i < n; i++) y[i] = 1.0 + (double)i * 0x1p-52;       /* one ulp apart */
    one(T, n, y, 1.0, (double)T, 1);
    free(y);
    free(r);
  }
  /* every tail length of the fitted range once, m = 30 + isqrt(n) along */
  for (int32_t n = 0; n <= SR_PSIS_NMAX; n += (n < 80 ? 1 : 97)) {
    double *y = (double *)malloc(sizeof(double) * (n ? n : 1));
    double Sr = 0.0;
    for (int32_t i = 0; i < n; i++) { y[i] = 2.0 + pow(1.0 - (i + 0.5) / n, -0.7); }
    qsort(y, (size_t)n, sizeof(double), cmp);
    for (int32_t i = 0; i < n; i++) Sr += y[i];
    one((int64_t)n * 5 + 1, n, y, 2.0, Sr + 2.0 * (4.0 * n + 1), 1);
    free(y);
  }
  printf("psis_asan %s: %ld tails, %ld smoothed, %ld flagged\n", bad ? "FAILED" : "ok", runs, smoothed, bad);
  return bad ? 1 : 0;
}
