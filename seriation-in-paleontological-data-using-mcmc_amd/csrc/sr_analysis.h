/*
 * sr_analysis.h -- what the host code of the analysis units shares.  HIP only: included by sr_records.hip and the
 * eleven analysis .hip files (sr_post, sr_diag, sr_marg, sr_rel, sr_waic, sr_loo, sr_agree, sr_central, sr_ppc, sr_occ,
 * sr_place), by nothing else.
 */
#ifndef SR_ANALYSIS_H
#define SR_ANALYSIS_H
#include <hip/hip_runtime.h>
#include <stdio.h>

/* inside a function with `int rc` and a `done:` label that frees what was allocated */
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  fprintf(stderr, "seriation: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); rc = -5; goto done; } } while (0)

#define SR_LDS_MAX (160 * 1024)   /* all the LDS one workgroup can have */
#define SR_GRID_CAP 65535         /* blocks along gridDim.y or .z */

/* `rows` of a sample stream cut into as many pieces as keep `resident` blocks busy in one round over `tiles` tiles
   (no tail), min_rows rows per piece at least and at most `cap` pieces: rows per piece, *pieces of them */
static inline long long sr_pieces(long long resident, long long tiles, long long rows, int min_rows, long long cap,
                                  long long *pieces)
{
  long long n = resident / tiles, nmax = rows / min_rows;
  if (n > nmax) n = nmax;
  if (n > cap) n = cap;
  if (n < 1) n = 1;
  const long long rpp = (rows + n - 1) / n;
  *pieces = (rows + rpp - 1) / rpp;
  return rpp;
}

/* log2 of the widest power-of-two tile, 64 columns at most, whose `bins` uint32 bins per column fit SR_LDS_MAX
   besides `fixed` bytes; *fits (optional) 0 when not even one column's bins do */
static inline int sr_lds_tile(size_t bins, size_t fixed, int *fits)
{
  int tcl = 6;
  while (tcl > 0 && fixed + (bins << tcl) * sizeof(unsigned) > SR_LDS_MAX) --tcl;
  if (fits) *fits = fixed + (bins << tcl) * sizeof(unsigned) <= SR_LDS_MAX;
  return tcl;
}

#endif
