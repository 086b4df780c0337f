/*
 * sr_rel.hip -- exact counts of the relations between taxa over the saved records (no counterpart in the
 * reference: an extension, definitions in include/seriation.h "taxon-pair relations").
 *
 * Only the limits a | b of a record row are read (2M int16 entries); a flagged chain's limits are reflected while
 * they are read (a <- N - b, b <- N - a), in int32, so nothing downstream knows of orientation and nothing wraps.
 * Unsigned integer counts throughout: the result does not depend on the order of the adds.
 *
 * Pair kernel: a comparison "GEMM".  A block of 4 waves owns a 64 x 64 tile of the M x M pair space and a piece of
 * the sample stream.  For a chunk of SRR_CH samples it stages the tile's a_i, b_i, a_j, b_j into LDS as int32 (lane
 * = column: a row's 64 limits are 128 contiguous bytes; columns beyond M are staged as 0 and never written back).
 * Inner loop: lane = j, wave w owns the 16 rows i = 16 w .. 16 w + 15, whose limits every lane reads from the same
 * LDS address (a broadcast); the four predicates accumulate in 4 x 16 registers per lane.  The kernel always forms
 * all four predicates (ten vector instructions per pair and sample); an output that was not asked for has no
 * device matrix, is not added to and not copied.  overlap is computed in full: mirroring the i <= j tiles would
 * save a fifth of the compares and cost a second write pattern.  When the tiles alone would leave compute units
 * idle the stream is cut into gridDim.z pieces; every block adds its non-zero counts into the zeroed device
 * matrices with vector atomics, as the marginals' histogram kernel does.  The loop is bound by vector-instruction
 * issue (185 per sample and wave); two other inner loops, rows in scalar registers through v_readlane and the sign
 * bit of the difference added without lane masks, measured slower and are not kept ("Taxon-pair
 * relations").  (lane = sample with a scalar population count of the compare mask was not built: it needs a
 * 64-bit mask and a scalar add per pair where this shape needs a compare and an add-with-carry per lane, and its
 * accumulators would have to live in scalar registers.)
 *
 * Duration kernel: sr_marg_hist_kernel's layout -- a block owns a tile of tc taxa with all N + 1 bins in LDS as
 * [bin][taxon], lane = taxon, so the atomics of a 32-lane group never meet on a bank -- over the value b - a, which
 * a reflection leaves unchanged ((N - a) - (N - b)): the flip is not even read.
 *
 * Richness kernel: per sample a difference array over positions, built in LDS, then a prefix scan, because that
 * costs O(M + N) per sample where counting the taxa alive at each position costs O(M N), and because it needs no
 * scratch buffer of per-sample rows and no second pass over them.  A block owns a tile of tc positions with all
 * M + 1 bins in LDS as [bin][position]; each of its 8 waves takes a sample at a time: its lanes walk the taxa and
 * add +1 at max(a, 0) and -1 at min(b, N), both clipped to the tile (a taxon alive before the tile adds its +1 at
 * the tile's first position), where that interval is non-empty; then lane = position reads its entry, clears it,
 * and an inclusive __shfl_up scan gives the number alive, which is counted into the bins.  The difference array is
 * private to the wave, whose LDS operations execute in order, so the loop holds no barrier.  tc is the largest
 * power of two (at most 64) whose bins fit the 160 KB of a workgroup; when not even one position's M + 1 bins fit
 * (M > 40000 or so) the waves add straight into the device histogram.  Every tile reads all the limits again, so
 * the pass costs N / tc readings of the records: one or a few for the shapes of the bench matrix.
 *
 * The rows are addressed through a record view (sr_records.h: chain k's rows start at rec + chain_off[k], row_stride
 * apart); srr_relations is the unit's one entry point.  The cut of the stream into pieces and the pick of tc are
 * sr_analysis.h's, shared with the marginals and the agreement.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_records.h"
#include "sr_analysis.h"

#define SRR_TILE 64                      /* pair kernel: the tile is SRR_TILE x SRR_TILE pairs */
#define SRR_PWAVES 4
#define SRR_PTHREADS (64 * SRR_PWAVES)
#define SRR_RI (SRR_TILE / SRR_PWAVES)   /* rows i per wave */
#define SRR_CH 32                        /* samples staged per chunk: 4 x 32 x 64 int32 = 32 KB */
#define SRR_THREADS 512                  /* duration and richness kernels */
#define SRR_WAVES (SRR_THREADS / 64)
#define SRR_U 8                          /* duration kernel: rows in flight per lane */
#define SRR_MIN_ROWS 64                  /* rows of the sample stream a block takes at least */

struct RelArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *flip;           /* [n_sel] or NULL */
  int count, N, M;
  int total, rows_per_piece;     /* rows of the sample stream (< 2^31), rows per grid piece */
  int tcl, direct;               /* duration, richness: log2 of the tile width; richness: no LDS bins */
  unsigned *pair[4];             /* [M][M] each, zeroed, or NULL: orig_before, ext_before, precedes, overlap */
  unsigned *hist;                /* duration: [M][N+1] (or NULL: outside only), richness: [N][M+1]; zeroed */
  unsigned *outside;             /* duration: [M], zeroed */
};

__global__ __launch_bounds__(SRR_PTHREADS) void sr_rel_pair_kernel(RelArgs A)
{
  __shared__ int sai[SRR_CH][SRR_TILE], sbi[SRR_CH][SRR_TILE], saj[SRR_CH][SRR_TILE], sbj[SRR_CH][SRR_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N, M = A.M;
  const int i0 = blockIdx.y * SRR_TILE, ci = i0 + lane, cj = blockIdx.x * SRR_TILE + lane;
  const bool iok = ci < M, jok = cj < M;
  /* the stream indices are unsigned: total < 2^31, so g0 + rows_per_piece and g + SRR_CH stay below 2^32 */
  const unsigned g0 = blockIdx.z * (unsigned)A.rows_per_piece;
  const unsigned g1 = min(g0 + (unsigned)A.rows_per_piece, (unsigned)A.total);
  unsigned ob[SRR_RI], eb[SRR_RI], pr[SRR_RI], ov[SRR_RI];
#pragma unroll
  for (int r = 0; r < SRR_RI; ++r) ob[r] = eb[r] = pr[r] = ov[r] = 0;
  for (unsigned g = g0; g < g1; g += SRR_CH) {
    const int n = (int)min((unsigned)SRR_CH, g1 - g);
    for (int s = wave; s < n; s += SRR_PWAVES) {
      const int k = (int)((g + s) / (unsigned)A.count), t = (int)((g + s) - (unsigned)k * (unsigned)A.count);
      const int16_t *row = A.rec + A.chain_off[k] + (long long)t * A.row_stride;
      int ai = iok ? (int)row[ci] : 0, bi = iok ? (int)row[M + ci] : 0;
      int aj = jok ? (int)row[cj] : 0, bj = jok ? (int)row[M + cj] : 0;
      if (A.flip && A.flip[k]) {
        const int ti = N - bi, tj = N - bj;
        bi = N - ai; ai = ti;
        bj = N - aj; aj = tj;
      }
      sai[s][lane] = ai; sbi[s][lane] = bi;
      saj[s][lane] = aj; sbj[s][lane] = bj;
    }
    __syncthreads();
    for (int s = 0; s < n; ++s) {
      const int aj = saj[s][lane], bj = sbj[s][lane];
#pragma unroll
      for (int r = 0; r < SRR_RI; ++r) {
        const int ai = sai[s][wave * SRR_RI + r], bi = sbi[s][wave * SRR_RI + r];
        ob[r] += ai < aj;
        eb[r] += bi < bj;
        pr[r] += bi <= aj;
        ov[r] += max(ai, aj) < min(bi, bj);
      }
    }
    __syncthreads();
  }
  if (!jok) return;
#pragma unroll
  for (int r = 0; r < SRR_RI; ++r) {
    const int i = i0 + wave * SRR_RI + r;
    if (i < M) {
      const size_t e = (size_t)i * M + cj;
      if (A.pair[0] && ob[r]) atomicAdd(&A.pair[0][e], ob[r]);
      if (A.pair[1] && eb[r]) atomicAdd(&A.pair[1][e], eb[r]);
      if (A.pair[2] && pr[r]) atomicAdd(&A.pair[2][e], pr[r]);
      if (A.pair[3] && ov[r]) atomicAdd(&A.pair[3][e], ov[r]);
    }
  }
}

__global__ __launch_bounds__(SRR_THREADS) void sr_rel_dur_kernel(RelArgs A)
{
  extern __shared__ unsigned srr_bins[];   /* [N+1][tc] */
  const int N = A.N, M = A.M, B = N + 1, tcl = A.tcl, tc = 1 << tcl, nw = B << tcl;
  for (int i = threadIdx.x; i < nw; i += SRR_THREADS) srr_bins[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = lane & (tc - 1), sub = lane >> tcl, R = 64 >> tcl;
  const int m = (blockIdx.x << tcl) + lc;
  const bool mok = m < M;
  const int mm = mok ? m : 0;
  const int slot = wave * R + sub, nslot = SRR_WAVES * R;
  const long long g0 = (long long)blockIdx.y * A.rows_per_piece;
  const long long g1 = min(g0 + A.rows_per_piece, (long long)A.total);
  unsigned out = 0;
  if (g0 < g1) {
    const int k1 = (int)((g1 - 1) / A.count);
    for (int k = (int)(g0 / A.count); k <= k1; ++k) {
      const long long cs = (long long)k * A.count;
      const int t0 = (int)(max(g0, cs) - cs), t1 = (int)(min(g1, cs + A.count) - cs);
      const int16_t *base = A.rec + A.chain_off[k] + mm;
      for (long long t = (long long)t0 + slot; t < t1; t += SRR_U * nslot) {
        int x[SRR_U];
#pragma unroll
        for (int u = 0; u < SRR_U; ++u) {
          const long long tt = t + u * nslot;
          x[u] = tt < t1 ? (int)base[tt * A.row_stride + M] - (int)base[tt * A.row_stride] : 0;
        }
#pragma unroll
        for (int u = 0; u < SRR_U; ++u) {
          if (t + u * nslot < t1 && mok) {
            if ((unsigned)x[u] > (unsigned)N) ++out;
            else if (A.hist) atomicAdd(&srr_bins[(x[u] << tcl) + lc], 1u);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nw && A.hist; i += SRR_THREADS) {
    const unsigned c = srr_bins[i];
    const int bm = (blockIdx.x << tcl) + (i & (tc - 1));
    if (c && bm < M) atomicAdd(&A.hist[(size_t)bm * B + (i >> tcl)], c);
  }
  if (A.outside && mok && out) atomicAdd(&A.outside[m], out);
}

__global__ __launch_bounds__(SRR_THREADS) void sr_rel_rich_kernel(RelArgs A)
{
  extern __shared__ unsigned srr_bins[];   /* [SRR_WAVES][64] difference arrays, then [M+1][tc] bins */
  const int N = A.N, M = A.M, B = M + 1, tcl = A.tcl, tc = 1 << tcl;
  const int nw = A.direct ? 0 : B << tcl;
  unsigned *bins = srr_bins + SRR_WAVES * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int *d = (int *)srr_bins + wave * 64;
  d[lane] = 0;
  for (int i = threadIdx.x; i < nw; i += SRR_THREADS) bins[i] = 0;
  __syncthreads();
  const int p0 = blockIdx.x << tcl, p1 = min(p0 + tc, N);   /* this tile: positions [p0, p1) */
  const unsigned g0 = blockIdx.y * (unsigned)A.rows_per_piece;
  const unsigned g1 = min(g0 + (unsigned)A.rows_per_piece, (unsigned)A.total);
  for (unsigned g = g0 + wave; g < g1; g += SRR_WAVES) {
    const int k = (int)(g / (unsigned)A.count), t = (int)(g - (unsigned)k * (unsigned)A.count);
    const int16_t *row = A.rec + A.chain_off[k] + (long long)t * A.row_stride;
    const bool f = A.flip && A.flip[k];
    for (int m = lane; m < M; m += 64) {
      int a = row[m], b = row[M + m];
      if (f) { const int ta = N - b; b = N - a; a = ta; }
      const int l = max(a, p0), h = min(b, p1);   /* p0 >= 0 and p1 <= N: the clamp to [0, N] is in the clip */
      if (l < h) {
        atomicAdd(&d[l - p0], 1);
        if (h < p1) atomicAdd(&d[h - p0], -1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int r = d[lane];   /* 0 beyond the tile */
    d[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int o = __shfl_up(r, s);
      if (lane >= s) r += o;
    }
    if (p0 + lane < p1) {
      if (A.direct) atomicAdd(&A.hist[(size_t)(p0 + lane) * B + r], 1u);
      else atomicAdd(&bins[(r << tcl) + lane], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nw; i += SRR_THREADS) {
    const unsigned c = bins[i];
    const int p = p0 + (i & (tc - 1));
    if (c && p < N) atomicAdd(&A.hist[(size_t)p * B + (i >> tcl)], c);
  }
}

/* The relations of the n_sel chains of a record view.  flip [n_sel] is a host input (may be NULL); pair[4]
   ([M][M] each), dur_hist [M][N+1], dur_outside [M], rich_hist [N][M+1] are host buffers, each optional. */
extern "C" int srr_relations(const sr_recview *v, int N, int M, const uint8_t *flip, uint32_t *const pair[4],
                             uint32_t *dur_hist, uint32_t *dur_outside, uint32_t *rich_hist, float *ms)
{
  int rc = 0;
  uint8_t *d_flip = nullptr;
  unsigned *d_pair[4] = {nullptr, nullptr, nullptr, nullptr}, *d_dur = nullptr, *d_out = nullptr, *d_rich = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || !pair || n_sel <= 0 || count < 1 || N < 1 || N > 32767 || M < 1 ||
      (long long)n_sel * count >= (1LL << 31))
    return -1;
  if (ms) *ms = 0.0f;
  const int total = n_sel * count;
  const bool want_pair = pair[0] || pair[1] || pair[2] || pair[3];
  const bool want_dur = dur_hist || dur_outside;
  const size_t mm = (size_t)M * M * sizeof(unsigned), dur_bytes = (size_t)M * (N + 1) * sizeof(unsigned);
  const size_t rich_bytes = (size_t)N * ((size_t)M + 1) * sizeof(unsigned);
  {
    int ncu = 0, per_cu = 0;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    if (ncu < 1) ncu = 1;
    if (flip) {
      HIPCHK(hipMalloc(&d_flip, n_sel));
      HIPCHK(hipMemcpy(d_flip, flip, n_sel, hipMemcpyHostToDevice));
    }
    for (int q = 0; q < 4; ++q)
      if (pair[q]) HIPCHK(hipMalloc(&d_pair[q], mm));
    if (dur_hist) HIPCHK(hipMalloc(&d_dur, dur_bytes));
    if (want_dur) HIPCHK(hipMalloc(&d_out, sizeof(unsigned) * M));
    if (rich_hist) HIPCHK(hipMalloc(&d_rich, rich_bytes));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    RelArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride; A.flip = d_flip;
    A.count = count; A.N = N; A.M = M; A.total = total;
    HIPCHK(hipEventRecord(e0, st));
    if (want_pair) {
      const int nt = (M + SRR_TILE - 1) / SRR_TILE;
      long long ny;
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_rel_pair_kernel, SRR_PTHREADS, 0));
      if (per_cu < 1) per_cu = 1;
      A.rows_per_piece = (int)sr_pieces((long long)ncu * per_cu, (long long)nt * nt, total, SRR_MIN_ROWS, SR_GRID_CAP, &ny);
      A.tcl = 0; A.direct = 0; A.hist = nullptr; A.outside = nullptr;
      for (int q = 0; q < 4; ++q) {
        A.pair[q] = d_pair[q];
        if (d_pair[q]) HIPCHK(hipMemsetAsync(d_pair[q], 0, mm, st));
      }
      hipLaunchKernelGGL(sr_rel_pair_kernel, dim3(nt, nt, (unsigned)ny), dim3(SRR_PTHREADS), 0, st, A);
      HIPCHK(hipGetLastError());
    }
    for (int q = 0; q < 4; ++q) A.pair[q] = nullptr;
    if (want_dur) {
      const int tcl = sr_lds_tile((size_t)N + 1, 0, nullptr);
      long long ny;
      const size_t lds = ((size_t)(N + 1) << tcl) * sizeof(unsigned);
      const int tiles = (M + (1 << tcl) - 1) >> tcl;
      HIPCHK(hipFuncSetAttribute((const void *)sr_rel_dur_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_rel_dur_kernel, SRR_THREADS, lds));
      if (per_cu < 1) per_cu = 1;
      A.rows_per_piece = (int)sr_pieces((long long)ncu * per_cu, tiles, total, SRR_MIN_ROWS, SR_GRID_CAP, &ny);
      A.tcl = tcl; A.direct = 0; A.hist = d_dur; A.outside = d_out;
      if (d_dur) HIPCHK(hipMemsetAsync(d_dur, 0, dur_bytes, st));
      HIPCHK(hipMemsetAsync(d_out, 0, sizeof(unsigned) * M, st));
      hipLaunchKernelGGL(sr_rel_dur_kernel, dim3(tiles, (unsigned)ny), dim3(SRR_THREADS), lds, st, A);
      HIPCHK(hipGetLastError());
    }
    if (rich_hist) {
      const size_t wd = SRR_WAVES * 64 * sizeof(int);
      int fits;
      int tcl = sr_lds_tile((size_t)M + 1, wd, &fits);
      long long ny;
      const int direct = !fits;
      if (direct) tcl = 6;
      const size_t lds = wd + (direct ? 0 : (((size_t)M + 1) << tcl) * sizeof(unsigned));
      const int tiles = (N + (1 << tcl) - 1) >> tcl;
      HIPCHK(hipFuncSetAttribute((const void *)sr_rel_rich_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_rel_rich_kernel, SRR_THREADS, lds));
      if (per_cu < 1) per_cu = 1;
      A.rows_per_piece = (int)sr_pieces((long long)ncu * per_cu, tiles, total, SRR_MIN_ROWS, SR_GRID_CAP, &ny);
      A.tcl = tcl; A.direct = direct; A.hist = d_rich; A.outside = nullptr;
      HIPCHK(hipMemsetAsync(d_rich, 0, rich_bytes, st));
      hipLaunchKernelGGL(sr_rel_rich_kernel, dim3(tiles, (unsigned)ny), dim3(SRR_THREADS), lds, st, A);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) HIPCHK(hipEventElapsedTime(ms, e0, e1));
    for (int q = 0; q < 4; ++q)
      if (pair[q]) HIPCHK(hipMemcpy(pair[q], d_pair[q], mm, hipMemcpyDeviceToHost));
    if (dur_hist) HIPCHK(hipMemcpy(dur_hist, d_dur, dur_bytes, hipMemcpyDeviceToHost));
    if (dur_outside) HIPCHK(hipMemcpy(dur_outside, d_out, sizeof(unsigned) * M, hipMemcpyDeviceToHost));
    if (rich_hist) HIPCHK(hipMemcpy(rich_hist, d_rich, rich_bytes, hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_flip) (void)hipFree(d_flip);
  for (int q = 0; q < 4; ++q)
    if (d_pair[q]) (void)hipFree(d_pair[q]);
  if (d_dur) (void)hipFree(d_dur);
  if (d_out) (void)hipFree(d_out);
  if (d_rich) (void)hipFree(d_rich);
  return rc;
}
