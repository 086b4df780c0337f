/*
 * sr_marg.hip -- exact marginal histograms of the saved records and the order statistics read off them (no
 * counterpart in the reference: an extension, definitions in include/seriation.h "posterior marginals").
 *
 * Every column j of the record row (a | b | pi, W = 2M + N int16 entries) gets B = N + 1 bins for the values
 * 0..N; hist[j][v] counts the n_sel x count samples whose value is v, a flagged chain's rows reflected first
 * (a <- N - b, b <- N - a, pi <- N - 1 - pi).  From the histogram: the Q quantiles min{v : C(v) >= k}, the
 * first-max mode and the mean (exact int64 numerator, one f64 division).  Integers throughout, so the result
 * does not depend on the order of the adds.
 *
 * Histogram kernel: a block owns a tile of tc columns with all B bins in LDS, laid out [bin][col]: with lane =
 * column the atomic of lane l goes to bank (v * tc + l) mod 32 = l mod 32 whatever the values are (tc = 64 or
 * 32: conflict-free within each 32-lane group, where [col][bin] would put the banks at the mercy of the data),
 * and the int16 row loads coalesce.  tc is the largest power of two whose tile fits the 160 KB of a workgroup:
 * 64 up to N = 639, one column at N = 32767 (128 KB); a wave of a narrower tile takes 64 / tc rows at a time.
 * The 8 waves stride over the sample stream, SRM_U rows in flight per lane (the pass is bound by the latency of
 * the row loads: 2 blocks x 8 waves x 16 rows x 128 bytes = 32 KB in flight per compute unit).  When the tiles
 * alone would leave compute units idle the stream is cut into gridDim.y pieces, as many as stay resident in one
 * round; every block adds its non-zero bins into the zeroed device histogram [col][bin] with vector atomics.
 * The per-chain sums of the raw pi columns (pi_sum) and the counts of out-of-range values come from the same
 * pass.
 *
 * Summary kernel: one wave per column over the device histogram: a first pass for the total, the mode and the
 * weighted sum, a second one scanning the bins 64 at a time (__shfl_up, the running count carried from chunk
 * to chunk) that stores the bin at which the cumulative count first reaches each rank.
 *
 * The columns are processed in batches whose device histogram stays below SRM_BATCH_BYTES; a batch reads only
 * its own columns, so every record entry is read once.
 *
 * The rows are addressed through a record view (sr_records.h: chain k's rows start at rec + chain_off[k], row_stride
 * apart); srm_marginals is the unit's one entry point.  The cut of the stream and the pick of tc are sr_analysis.h's.
 */
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_records.h"
#include "sr_analysis.h"

#define SRM_THREADS 512
#define SRM_WAVES (SRM_THREADS / 64)
#define SRM_SUM_THREADS 256              /* summary kernel: one wave per column */
#define SRM_SUM_WAVES (SRM_SUM_THREADS / 64)
#define SRM_U 16                         /* rows in flight per lane */
#define SRM_BATCH_BYTES ((size_t)256 << 20)   /* device histogram of one column batch (as DIAG_BATCH_BYTES) */
#define SRM_MIN_ROWS 64                  /* rows of the sample stream a block takes at least */
#define SRM_QMAX 16

struct MargArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *flip;           /* [n_sel] or NULL */
  int n_sel, count, N, M;
  int col0, ncol;                /* this batch: columns [col0, col0 + ncol) */
  int tcl;                       /* log2 of the tile width */
  long long total, rows_per_y;   /* rows of the sample stream, rows per gridDim.y piece */
  unsigned *hist;                /* [ncol][N+1] of this batch, zeroed */
  unsigned *outside;             /* [W], zeroed */
  unsigned long long *pi_sum;    /* [n_sel][N], zeroed, or NULL */
};

__global__ __launch_bounds__(SRM_THREADS) void sr_marg_hist_kernel(MargArgs A)
{
  extern __shared__ unsigned srm_bins[];   /* [N+1][tc] */
  const int N = A.N, M = A.M, B = N + 1, tcl = A.tcl, tc = 1 << tcl, nw = B << tcl;
  for (int i = threadIdx.x; i < nw; i += SRM_THREADS) srm_bins[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = lane & (tc - 1), sub = lane >> tcl, R = 64 >> tcl;
  const int bcol = (blockIdx.x << tcl) + lc;
  const bool cok = bcol < A.ncol;
  const int cc = A.col0 + (cok ? bcol : 0);
  /* a flagged chain: a reads its taxon's b, b its a, both reflected about N; pi about N - 1 */
  const int kind = cc < M ? 0 : (cc < 2 * M ? 1 : 2);
  const int fsrc = kind == 0 ? cc + M : (kind == 1 ? cc - M : cc);
  const int fbase = kind == 2 ? N - 1 : N;
  const int slot = wave * R + sub, nslot = SRM_WAVES * R;
  const long long g0 = (long long)blockIdx.y * A.rows_per_y;
  const long long g1 = min(g0 + A.rows_per_y, A.total);
  unsigned out = 0;
  if (g0 < g1) {
    const int k1 = (int)((g1 - 1) / A.count);
    for (int k = (int)(g0 / A.count); k <= k1; ++k) {
      const long long cs = (long long)k * A.count;
      const int t0 = (int)(max(g0, cs) - cs), t1 = (int)(min(g1, cs + A.count) - cs);
      const bool f = A.flip && A.flip[k];
      const int16_t *base = A.rec + A.chain_off[k] + (f ? fsrc : cc);
      long long ps = 0;
      for (long long t = (long long)t0 + slot; t < t1; t += SRM_U * nslot) {
        int x[SRM_U];
#pragma unroll
        for (int u = 0; u < SRM_U; ++u) {
          const long long tt = t + u * nslot;
          x[u] = tt < t1 ? (int)base[tt * A.row_stride] : 0;
        }
#pragma unroll
        for (int u = 0; u < SRM_U; ++u) {
          if (t + u * nslot < t1 && cok) {
            ps += x[u];
            const int v = f ? fbase - x[u] : x[u];
            if ((unsigned)v <= (unsigned)N) atomicAdd(&srm_bins[(v << tcl) + lc], 1u);
            else ++out;
          }
        }
      }
      if (A.pi_sum && cok && kind == 2 && ps != 0)
        atomicAdd(&A.pi_sum[(size_t)k * N + (cc - 2 * M)], (unsigned long long)ps);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nw; i += SRM_THREADS) {
    const unsigned c = srm_bins[i];
    const int bc = (blockIdx.x << tcl) + (i & (tc - 1));
    if (c && bc < A.ncol) atomicAdd(&A.hist[(size_t)bc * B + (i >> tcl)], c);
  }
  if (cok && out) atomicAdd(&A.outside[cc], out);
}

struct MargSumArgs {
  const unsigned *hist;   /* [ncol][N+1] of this batch */
  int N, W, col0, ncol, Q;
  double probs[SRM_QMAX];
  int *quant, *mode;      /* [Q][W], [W]; either may be NULL */
  double *mean;           /* [W] or NULL */
};

__global__ __launch_bounds__(SRM_SUM_THREADS) void sr_marg_sum_kernel(MargSumArgs A)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bc = blockIdx.x * SRM_SUM_WAVES + wave;
  if (bc >= A.ncol) return;   /* the whole wave */
  const int B = A.N + 1, col = A.col0 + bc;
  const unsigned *h = A.hist + (size_t)bc * B;
  /* the total, the weighted sum, the first largest bin */
  unsigned long long T = 0;
  long long ws = 0;
  unsigned best = 0;
  int bestv = INT_MAX;
  for (int v = lane; v < B; v += 64) {
    const unsigned c = h[v];
    T += c;
    ws += (long long)v * c;
    if (c > best) { best = c; bestv = v; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    T += __shfl_xor(T, d);
    ws += __shfl_xor(ws, d);
    const unsigned ob = __shfl_xor(best, d);
    const int ov = __shfl_xor(bestv, d);
    if (ob > best || (ob == best && ov < bestv)) { best = ob; bestv = ov; }
  }
  if (T == 0) {
    if (lane == 0) {
      if (A.mode) A.mode[col] = -1;
      if (A.mean) A.mean[col] = __builtin_nan("");
      if (A.quant)
        for (int q = 0; q < A.Q; ++q) A.quant[(size_t)q * A.W + col] = -1;
    }
    return;
  }
  if (lane == 0) {
    if (A.mode) A.mode[col] = bestv;
    if (A.mean) A.mean[col] = (double)ws / (double)T;
  }
  if (!A.quant || A.Q == 0) return;
  /* rank k = clamp(ceil(p T), 1, T): the bin at which the cumulative count first reaches it */
  unsigned long long kq[SRM_QMAX];
#pragma unroll
  for (int q = 0; q < SRM_QMAX; ++q) {
    const double r = ceil(A.probs[q] * (double)T);
    unsigned long long k = r < 1.0 ? 1ull : (unsigned long long)r;
    kq[q] = k > T ? T : k;
  }
  unsigned long long carry = 0;
  for (int v0 = 0; v0 < B; v0 += 64) {
    const int v = v0 + lane;
    const unsigned c = v < B ? h[v] : 0u;
    unsigned incl = c;   /* a chunk's counts sum to at most T < 2^31 */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    const unsigned long long hi = carry + incl, lo = hi - c;
    if (c) {
#pragma unroll
      for (int q = 0; q < SRM_QMAX; ++q)
        if (q < A.Q && lo < kq[q] && kq[q] <= hi) A.quant[(size_t)q * A.W + col] = v;
    }
    carry += __shfl(incl, 63);
  }
}

/* The marginals of the n_sel chains of a record view.  flip [n_sel] and probs [Q] are host inputs (flip may be
   NULL); hist [W][N+1], outside [W], pi_sum [n_sel][N], quant [Q][W], mode [W], mean [W] are host buffers, each
   optional. */
extern "C" int srm_marginals(const sr_recview *v, int N, int M, const uint8_t *flip, const double *probs, int Q,
                             uint32_t *hist, uint32_t *outside, long long *pi_sum, int32_t *quant, int32_t *mode,
                             double *mean, float *ms)
{
  int rc = 0;
  uint8_t *d_flip = nullptr;
  unsigned *d_hist = nullptr, *d_outside = nullptr;
  unsigned long long *d_pisum = nullptr;
  int *d_quant = nullptr, *d_mode = nullptr;
  double *d_mean = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || n_sel <= 0 || count < 1 || N < 1 || N > 32767 || M < 0 || Q < 0 || Q > SRM_QMAX ||
      (Q > 0 && !probs) || (long long)n_sel * count >= (1LL << 31))
    return -1;
  if (ms) *ms = 0.0f;
  const int W = 2 * M + N, B = N + 1;
  const long long total = (long long)n_sel * count;
  const bool need_sum = (quant && Q > 0) || mode || mean;
  const int tcl = sr_lds_tile(B, 0, nullptr), tc = 1 << tcl;
  const size_t lds = ((size_t)B << tcl) * sizeof(unsigned);
  /* columns per batch: whole tiles, the device histogram within SRM_BATCH_BYTES */
  size_t cb = SRM_BATCH_BYTES / ((size_t)B * sizeof(unsigned));
  cb = cb / tc * tc;
  if (cb < (size_t)tc) cb = tc;
  if (cb > (size_t)W) cb = W;
  {
    int ncu = 0, per_cu = 0;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    if (ncu < 1) ncu = 1;
    if (flip) {
      HIPCHK(hipMalloc(&d_flip, n_sel));
      HIPCHK(hipMemcpy(d_flip, flip, n_sel, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&d_hist, cb * B * sizeof(unsigned)));
    HIPCHK(hipMalloc(&d_outside, sizeof(unsigned) * W));
    HIPCHK(hipMemsetAsync(d_outside, 0, sizeof(unsigned) * W, st));
    if (pi_sum) {
      HIPCHK(hipMalloc(&d_pisum, sizeof(unsigned long long) * (size_t)n_sel * N));
      HIPCHK(hipMemsetAsync(d_pisum, 0, sizeof(unsigned long long) * (size_t)n_sel * N, st));
    }
    if (quant && Q > 0) HIPCHK(hipMalloc(&d_quant, sizeof(int) * (size_t)Q * W));
    if (mode) HIPCHK(hipMalloc(&d_mode, sizeof(int) * W));
    if (mean) HIPCHK(hipMalloc(&d_mean, sizeof(double) * W));
    HIPCHK(hipFuncSetAttribute((const void *)sr_marg_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_marg_hist_kernel, SRM_THREADS, lds));
    if (per_cu < 1) per_cu = 1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int col0 = 0; col0 < W; col0 += (int)cb) {
      const int ncol = W - col0 < (int)cb ? W - col0 : (int)cb;
      const int tiles = (ncol + tc - 1) / tc;
      long long ny;
      const long long rpy = sr_pieces((long long)ncu * per_cu, tiles, total, SRM_MIN_ROWS, SR_GRID_CAP, &ny);
      MargArgs A;
      A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride; A.flip = d_flip;
      A.n_sel = n_sel; A.count = count; A.N = N; A.M = M;
      A.col0 = col0; A.ncol = ncol; A.tcl = tcl; A.total = total; A.rows_per_y = rpy;
      A.hist = d_hist; A.outside = d_outside; A.pi_sum = d_pisum;
      HIPCHK(hipEventRecord(e0, st));
      HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)ncol * B * sizeof(unsigned), st));
      hipLaunchKernelGGL(sr_marg_hist_kernel, dim3(tiles, (unsigned)ny), dim3(SRM_THREADS), lds, st, A);
      HIPCHK(hipGetLastError());
      if (need_sum) {
        MargSumArgs S;
        S.hist = d_hist; S.N = N; S.W = W; S.col0 = col0; S.ncol = ncol; S.Q = Q;
        for (int q = 0; q < SRM_QMAX; ++q) S.probs[q] = q < Q ? probs[q] : 0.0;
        S.quant = d_quant; S.mode = d_mode; S.mean = d_mean;
        hipLaunchKernelGGL(sr_marg_sum_kernel, dim3((ncol + SRM_SUM_WAVES - 1) / SRM_SUM_WAVES), dim3(SRM_SUM_THREADS), 0, st, S);
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipEventRecord(e1, st));
      HIPCHK(hipStreamSynchronize(st));
      float bms = 0.0f;
      HIPCHK(hipEventElapsedTime(&bms, e0, e1));
      if (ms) *ms += bms;
      if (hist)
        HIPCHK(hipMemcpy(hist + (size_t)col0 * B, d_hist, (size_t)ncol * B * sizeof(unsigned), hipMemcpyDeviceToHost));
    }
    if (outside) HIPCHK(hipMemcpy(outside, d_outside, sizeof(unsigned) * W, hipMemcpyDeviceToHost));
    if (pi_sum) HIPCHK(hipMemcpy(pi_sum, d_pisum, sizeof(long long) * (size_t)n_sel * N, hipMemcpyDeviceToHost));
    if (d_quant) HIPCHK(hipMemcpy(quant, d_quant, sizeof(int) * (size_t)Q * W, hipMemcpyDeviceToHost));
    if (mode) HIPCHK(hipMemcpy(mode, d_mode, sizeof(int) * W, hipMemcpyDeviceToHost));
    if (mean) HIPCHK(hipMemcpy(mean, d_mean, sizeof(double) * W, hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_flip) (void)hipFree(d_flip);
  if (d_hist) (void)hipFree(d_hist);
  if (d_outside) (void)hipFree(d_outside);
  if (d_pisum) (void)hipFree(d_pisum);
  if (d_quant) (void)hipFree(d_quant);
  if (d_mode) (void)hipFree(d_mode);
  if (d_mean) (void)hipFree(d_mean);
  return rc;
}
