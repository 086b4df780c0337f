/*
 * sr_diag.hip -- the integer moments behind split-R-hat and the effective sample size of the saved
 * records (no counterpart in the reference: an extension, DESIGN.md "Convergence diagnostics").
 *
 * Every selected chain's `count` records are split into two sequences of h = count / 2 rows (rows
 * [0, h) and [count - h, count)); sequence s = 2 * chain + half.  For every sequence, integer column j of
 * the record row (a | b | pi, W = 2M + N int16 entries) and lag k = 0..L, with x_t the h values:
 *   P[s][k][j] = sum_{t = 0}^{h-1-k} x_t * x_{t+k}
 *   F[s][k][j] = sum_{t < k} x_t            B[s][k][j] = sum_{t >= h-k} x_t            S1[s][j] = sum_t x_t
 * exact in int64 for any int16 content.  The host (sr_host.c) turns them into centred autocovariances in
 * __int128 and runs the f64 tail; there is no floating point here.
 *
 * Layout: a block owns one sequence x a tile of 64 columns, lane = column (row loads coalesce, LDS reads
 * are conflict-free).  The h x 64 tile is staged in LDS once, followed by KL + U rows of zeros, so a lag's
 * sum may run past its last term without a ragged tail.  The 4 waves split the lags in passes of KL = 16
 * consecutive lags; a pass walks t in steps of U = 16 rows and feeds 16 + 31 LDS reads into 256
 * multiply-adds held in registers.  The products are accumulated in 32 bits over runs that cannot overflow
 * for the tile's largest |x| (positions and limits below 2^9: 8176 rows per run, i.e. never flushed at 1000
 * draws) and flushed into 64 bits between runs; tiles whose values allow no run of U rows (|x| > 11585)
 * accumulate in 64 bits.  All LDS is dynamic: the tile with its zero rows, then SRD_TAIL bytes for the block's
 * largest |x|; (h + 32) * 128 + 16 <= 163840 holds up to h = 1247.  Longer sequences (h >= 1248) read their
 * rows from global memory (L2-resident: a tile is h x 128 bytes) through the same loops.
 *
 * The rows are addressed through a record view (sr_records.h: chain k's rows start at rec + chain_off[k],
 * row_stride apart); srd_moments is the unit's one entry point, and a batch of a session's chains is a slice of
 * the session's view.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "sr_records.h"
#include "sr_analysis.h"

#define TCOL 64   /* columns per block (lanes) */
#define KL 16     /* lags per pass */
#define U 16      /* rows per unrolled step */
#define PADR (KL + U)   /* zero rows behind the tile */
#define SRD_TAIL 16      /* dynamic LDS behind the tile: the block's largest |x| (kept 16-byte aligned) */
#define SRD_LDS_MAX (160 * 1024)   /* all the LDS one workgroup can have; the kernels declare no static LDS */

struct DiagArgs {
  const int16_t *rec;
  const long long *chain_off;   /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  int count, h, L, W;
  long long *P, *F, *B, *S1;    /* [S][L+1][W] x 3, [S][W] */
};

/* One pass: lags k0 .. k0 + KL - 1 of this thread's column; X(t) is row t of the column, 0 for t >= h.
   ACC = int32_t: at most `fe` steps of U rows between flushes into 64 bits. */
template <typename ACC, typename XF>
__device__ __forceinline__ void srd_pass(XF X, int h, int k0, int fe, long long (&tot)[KL])
{
  ACC acc[KL];
#pragma unroll
  for (int k = 0; k < KL; ++k) { acc[k] = 0; tot[k] = 0; }
  const int n = h - k0;   /* terms of the longest lag of the pass */
  for (int t0 = 0; t0 < n;) {
    const int tend = (int)min((long long)n, (long long)t0 + (long long)fe * U);
    for (int t = t0; t < tend; t += U) {
      int xv[U], yv[U + KL - 1];
#pragma unroll
      for (int i = 0; i < U; ++i) xv[i] = X(t + i);
#pragma unroll
      for (int i = 0; i < U + KL - 1; ++i) yv[i] = X(t + k0 + i);
#pragma unroll
      for (int i = 0; i < U; ++i) {
#pragma unroll
        for (int k = 0; k < KL; ++k) acc[k] += (ACC)xv[i] * (ACC)yv[i + k];
      }
    }
    t0 += ((tend - t0 + U - 1) / U) * U;
    if (sizeof(ACC) == 4) {
#pragma unroll
      for (int k = 0; k < KL; ++k) { tot[k] += (long long)acc[k]; acc[k] = 0; }
    }
  }
  if (sizeof(ACC) == 8) {
#pragma unroll
    for (int k = 0; k < KL; ++k) tot[k] = (long long)acc[k];
  }
}

template <bool INLDS>
__global__ __launch_bounds__(256) void sr_diag_kernel(DiagArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char srd_smem[];
  int16_t(*tile)[TCOL] = (int16_t(*)[TCOL])srd_smem;
  int *smax = (int *)(srd_smem + (INLDS ? (size_t)(A.h + PADR) * TCOL * sizeof(int16_t) : 0));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * TCOL + lane;
  const bool cok = col < A.W;
  const int cc = cok ? col : A.W - 1;
  const int s = blockIdx.y, h = A.h, L = A.L;
  const long long stride = A.row_stride;
  const int16_t *base = A.rec + A.chain_off[s >> 1] + (long long)((s & 1) ? A.count - h : 0) * stride + cc;

  /* stage the tile (wave w: rows w, w + 4, ..) and find the tile's largest |x| */
  if (threadIdx.x == 0) *smax = 0;
  __syncthreads();
  int mx = 0;
  for (int t = wave; t < h; t += 4) {
    const int v = base[(long long)t * stride];
    if (INLDS) tile[t][lane] = (int16_t)v;
    mx = max(mx, v < 0 ? -v : v);
  }
  if (INLDS)
    for (int t = h + wave; t < h + PADR; t += 4) tile[t][lane] = 0;
  atomicMax(smax, mx);
  __syncthreads();
  mx = max(*smax, 1);
  /* steps of U rows a 32-bit accumulator takes without overflow: fe * U * mx^2 <= 2^31 - 1 */
  const int fe = (int)(2147483647LL / ((long long)mx * mx) / U);

  auto X = [&](int t) -> int {
    if (INLDS) return tile[t][lane];
    return t < h ? (int)base[(long long)t * stride] : 0;
  };

  const size_t lw = (size_t)(L + 1) * A.W;
  long long *Ps = A.P + (size_t)s * lw + col;
  const int npass = L / KL + 1;
  for (int p = wave; p < npass; p += 4) {
    const int k0 = p * KL;
    long long tot[KL];
    if (fe >= 1) srd_pass<int32_t>(X, h, k0, fe, tot);
    else srd_pass<long long>(X, h, k0, 1 << 20, tot);
    if (cok) {
#pragma unroll
      for (int k = 0; k < KL; ++k)
        if (k0 + k <= L) Ps[(size_t)(k0 + k) * A.W] = tot[k];
    }
  }
  /* the prefix, suffix and whole sums: one wave each (the waves with the shorter passes) */
  if (!cok) return;
  if (wave == 3) {
    long long run = 0, *Fs = A.F + (size_t)s * lw + col;
    for (int k = 0; k <= L; ++k) { Fs[(size_t)k * A.W] = run; run += X(k); }
  } else if (wave == 2) {
    long long run = 0, *Bs = A.B + (size_t)s * lw + col;
    for (int k = 0; k <= L; ++k) { Bs[(size_t)k * A.W] = run; run += X(h - 1 - k); }
  } else if (wave == 1) {
    long long run = 0;
    for (int t = 0; t < h; ++t) run += X(t);
    A.S1[(size_t)s * A.W + col] = run;
  }
}

/* The moments of the n_sel chains of a record view (S = 2 n_sel sequences, h = count / 2, lags 0..L);
   P, F, B [S][L+1][W] and S1 [S][W] are host buffers. */
extern "C" int srd_moments(const sr_recview *v, int W, int L, long long *P, long long *F, long long *B, long long *S1,
                           float *ms)
{
  int rc = 0;
  long long *d_out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  const int h = count / 2;
  if (!v->rec || !v->chain_off || !P || !F || !B || !S1 || n_sel <= 0 || count < 4 || W < 1 || L < 1 || L >= h) return -1;
  if (2LL * n_sel > 65535) return -1;   /* one grid row per sequence */
  const size_t S = 2 * (size_t)n_sel, lw = (size_t)(L + 1) * W, nP = S * lw, nS = S * (size_t)W;
  {
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMalloc(&d_out, sizeof(long long) * (3 * nP + nS)));
    DiagArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride;
    A.count = count; A.h = h; A.L = L; A.W = W;
    A.P = d_out; A.F = d_out + nP; A.B = d_out + 2 * nP; A.S1 = d_out + 3 * nP;
    const size_t tile = (size_t)(h + PADR) * TCOL * sizeof(int16_t);
    const bool inlds = tile + SRD_TAIL <= SRD_LDS_MAX;
    const size_t lds = (inlds ? tile : 0) + SRD_TAIL;
    dim3 grid((W + TCOL - 1) / TCOL, (unsigned)S);
    if (inlds)
      HIPCHK(hipFuncSetAttribute((const void *)sr_diag_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    if (inlds) hipLaunchKernelGGL(sr_diag_kernel<true>, grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL(sr_diag_kernel<false>, grid, dim3(256), lds, st, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) HIPCHK(hipEventElapsedTime(ms, e0, e1));
    HIPCHK(hipMemcpy(P, A.P, sizeof(long long) * nP, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(F, A.F, sizeof(long long) * nP, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(B, A.B, sizeof(long long) * nP, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(S1, A.S1, sizeof(long long) * nS, hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_out) (void)hipFree(d_out);
  return rc;
}
