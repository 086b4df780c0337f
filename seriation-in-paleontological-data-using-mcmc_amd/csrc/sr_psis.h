/*
 * sr_psis.h -- one cell's Pareto-smoothed importance-sampling tail (include/seriation.h "PSIS-LOO"): the
 * generalised-Pareto fit of Zhang & Stephens 2009 to the n largest importance ratios and the smoothed
 * leave-one-out estimate, compiled both for the host (gcc, -ffp-contract=off) and for gfx950 (hipcc,
 * -ffp-contract=off) like sr_math.h.  The finish kernel of sr_loo.hip and sr_loo_tail (sr_host.c) run this source;
 * every sum is sequential ascending from +0.0 and exp / log are sr_exp_m / sr_log_m, so both give the bits of the
 * definition.
 */
#ifndef SR_PSIS_H
#define SR_PSIS_H
#include <stddef.h>
#include <stdint.h>
#include "sr_math.h"

#define SR_PSIS_NMAX 4096                /* the longest tail: n <= 4096 */
#define SR_PSIS_MMAX (30 + 64)           /* m = 30 + isqrt(n) */

/* the tail length n = min(T / 5, s), s the smallest integer with s * s >= 9 T (1 <= T < 2^31) */
SR_HD int32_t sr_psis_tail_len(int64_t T)
{
  const int64_t t9 = 9 * T;
  int64_t lo = 0, hi = 1 << 18;          /* (2^18)^2 = 2^36 > 9 * 2^31 */
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (mid * mid >= t9) hi = mid;
    else lo = mid + 1;
  }
  const int64_t n = T / 5 < lo ? T / 5 : lo;
  return (int32_t)n;
}

/* m - 30 = isqrt(n), 0 <= n <= SR_PSIS_NMAX */
SR_HD int32_t sr_psis_isqrt(int32_t n)
{
  int32_t r = 0;
  while ((r + 1) * (r + 1) <= n) r++;
  return r;
}

SR_HD int sr_psis_finite(double x) { return (sr_bits(x) & 0x7FF0000000000000ULL) != 0x7FF0000000000000ULL; }

/* y_j = y[(j - 1) * ystride], j = 1..n, ascending: the n largest of the cell's T ratios; r_cut the next one; Sr the
   sum of all T; G [m] and L [n] the host tables.  *k the Pareto shape (+inf: the tail was not smoothed), *elpd the
   leave-one-out log predictive density. */
SR_HD void sr_psis_tail(const double *y, ptrdiff_t ystride, int32_t n, double r_cut, double Sr, int64_t T,
                        const double *G, int32_t m, const double *L, const sr_mtab *tb, double *k_out, double *elpd_out)
{
  double lj[SR_PSIS_MMAX];
  const double nd = (double)n;
  int smooth = n >= 5 && n <= SR_PSIS_NMAX && m <= SR_PSIS_MMAX;
  double k = 0.0, sigma = 0.0;
  if (smooth) {
    const double xs = y[(ptrdiff_t)((n + 2) / 4 - 1) * ystride] - r_cut;
    const double xn = y[(ptrdiff_t)(n - 1) * ystride] - r_cut;
    smooth = xs > 0.0;
    if (smooth) {
      const double ixn = 1.0 / xn;
      double lmax = -__builtin_inf();
      for (int32_t j = 0; j < m && smooth; j++) {
        const double theta = ixn + G[j] / xs;
        double s = 0.0;
        for (int32_t i = 0; i < n; i++) {
          const double x = y[(ptrdiff_t)i * ystride] - r_cut;
          const double tx = theta * x;
          s += sr_log_m(1.0 - tx, tb);
        }
        const double kj = s / nd;
        const double q = -theta / kj;
        const double l = nd * ((sr_log_m(q, tb) - kj) - 1.0);
        if (!sr_psis_finite(l)) smooth = 0;
        lj[j] = l;
        if (l > lmax) lmax = l;
      }
      if (smooth) {
        double z = 0.0;
        for (int32_t j = 0; j < m; j++) z += sr_exp_m(lj[j] - lmax, tb);
        double th = 0.0;
        for (int32_t j = 0; j < m; j++) {
          const double theta = ixn + G[j] / xs;
          const double w = sr_exp_m(lj[j] - lmax, tb) / z;
          const double tw = theta * w;
          th += tw;
        }
        double s = 0.0;
        for (int32_t i = 0; i < n; i++) {
          const double x = y[(ptrdiff_t)i * ystride] - r_cut;
          const double tx = th * x;
          s += sr_log_m(1.0 - tx, tb);
        }
        const double k0 = s / nd;
        sigma = -k0 / th;
        const double kn = k0 * nd;
        k = (kn + 5.0) / (nd + 10.0);
        smooth = sr_psis_finite(th) && sr_psis_finite(k0) && sr_psis_finite(sigma) && sr_psis_finite(k);
      }
    }
  }
  if (!smooth) {
    *k_out = __builtin_inf();
    *elpd_out = sr_log_m((double)T / Sr, tb);
    return;
  }
  const double yn = y[(ptrdiff_t)(n - 1) * ystride];
  double St = 0.0, Sw = 0.0, Nn = 0.0;
  for (int32_t j = 0; j < n; j++) {
    const double yj = y[(ptrdiff_t)j * ystride];
    double sj;
    if (k == 0.0) {
      const double sl = sigma * L[j];
      sj = r_cut - sl;
    } else {
      const double e = sr_exp_m(-k * L[j], tb) - 1.0;
      const double se = sigma * e;
      sj = r_cut + se / k;
    }
    const double wt = sj < yn ? sj : yn;   /* a NaN or an overflowed s_j is truncated too */
    St += yj;
    Sw += wt;
    Nn += wt / yj;
  }
  const double D = (Sr - St) + Sw;
  *k_out = k;
  *elpd_out = sr_log_m(((double)(T - (int64_t)n) + Nn) / D, tb);
}

#endif
