/*
 * sr_occ.hip -- cell occupancy and the per-site, per-taxon error tallies over the saved records (no counterpart in
 * the reference: an extension, definitions in include/seriation.h "cell occupancy").
 *
 * Cell (n, m) is alive in a sample when a_m <= pi_n < b_m, compared in int32.  Unsigned integer counts throughout:
 * the result does not depend on the order of the adds.  No flip is read: a reflection changes no alive bit.
 *
 * Cell kernel (alive [N][M]): sr_rel.hip's pair kernel with one predicate.  A block of 4 waves owns a tile of
 * SRO_TS sites x 64 taxa and a piece of the sample stream.  For a chunk of SRO_CH samples it stages the tile's a, b
 * (lane = taxon: a row's 64 limits are 128 contiguous bytes) and the tile's pi into LDS as int32; taxa beyond M are
 * staged as the empty interval (0, 0) and sites beyond N at INT_MAX, where nothing is alive, and neither is written
 * back.  Inner loop: lane = taxon, wave w owns the SRO_SI sites 16 w .. 16 w + 15, whose positions every lane reads
 * from one LDS address (a broadcast); the counts stay in SRO_SI registers per lane.  When the tiles alone would
 * leave compute units idle the stream is cut into gridDim.z pieces; every block adds its non-zero counts into the
 * zeroed device matrix with vector atomics.
 *
 * Margin kernel (the six histograms): one kernel in two roles, launched once per margin that was asked for.  In the
 * site role a lane owns a site (its pi in a register) and walks the taxa; in the taxon role it owns a taxon (a, b in
 * registers) and walks the sites.  What it walks comes through LDS: the tc lanes that share a sample each load one
 * of the next tc entries of the row, store it, and all read them back one by one (a broadcast within the group;
 * entries beyond the row are staged as never alive).  X comes bit-packed, once per call and on the host, along the
 * walked dimension: one 64-bit word per owned column and 64 steps, shifted down a bit a step, padding bits zero.  A
 * lane keeps two counters, A (alive) and AX (alive with x = 1); f0 = A - AX and f1 = (the column's ones) - AX.
 * Bins are sr_marg_hist_kernel's: a block owns a tile of tc owned columns with the bins of every histogram asked
 * for in LDS as [hist][bin][column], tc the largest power of two that fits (sr_lds_tile), the 64 / tc groups of a
 * wave taking a sample each; where not one column's bins fit, the lanes add straight into the device histograms
 * (direct, tc = 64), as sr_rel.hip's richness kernel does.  The staging slots belong to one wave, whose LDS
 * operations execute in order, so the walk holds no barrier.
 *
 * The shape first proposed took both margins from one pass: lane = taxon, the alive predicate as a 64-bit ballot, the
 * site's counts as scalar population counts added into a per-wave [N][3] array in LDS.  That array is 12 N bytes a
 * wave -- 384 KB at the largest legal N, more than a workgroup has -- so it needs a second design for large N
 * anyway; the two-role kernel has no such bound, needs no scratch buffer in HBM (hence no SR_OCC_SCRATCH knob), and a
 * call that asks for one margin pays for one.  It forms every predicate twice when both margins are asked for.  The
 * ballot loop was not built, so there is no measured comparison of the two.  Measured on one MI355X, 8 chains x 1000
 * samples of 256 x 512 ("Cell occupancy"): cell kernel 0.15 ms, the two margin launches 0.73 ms.
 *
 * The rows are addressed through a record view (sr_records.h); sro_occupancy is the unit's one entry point.  The cut
 * of the stream into pieces and the pick of tc are sr_analysis.h's.
 */
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_records.h"
#include "sr_analysis.h"

#define SRO_TS 64                        /* cell kernel: sites per tile (the taxa per tile are a wave's 64 lanes) */
#define SRO_CWAVES 4
#define SRO_CTHREADS (64 * SRO_CWAVES)
#define SRO_SI (SRO_TS / SRO_CWAVES)     /* sites per wave */
#define SRO_CH 32                        /* samples staged per chunk: 3 x 32 x 64 int32 = 24 KB */
#define SRO_THREADS 512                  /* margin kernel */
#define SRO_WAVES (SRO_THREADS / 64)
#define SRO_MIN_ROWS 64                  /* rows of the sample stream a block takes at least */

struct OccArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  int count, N, M;
  int total, rows_per_piece;     /* rows of the sample stream (< 2^31), rows per grid piece */
  unsigned *alive;               /* cell kernel: [N][M], zeroed */
  /* margin kernel: C owned columns, O walked entries; xbits [C][(O + 63) / 64], bit o of column c's words is x */
  int C, O, tcl, direct, nh;
  const unsigned long long *xbits;
  unsigned *hist[3];             /* the nh histograms asked for, [C][O+1] each, zeroed */
  int which[3];                  /* what each counts: 0 alive, 1 f0, 2 f1 */
};

__global__ __launch_bounds__(SRO_CTHREADS) void sr_occ_cell_kernel(OccArgs A)
{
  __shared__ int sa[SRO_CH][64], sb[SRO_CH][64], sp[SRO_CH][SRO_TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N, M = A.M;
  const int n0 = blockIdx.y * SRO_TS, cn = n0 + lane, cm = blockIdx.x * 64 + lane;
  const bool nok = cn < N, mok = cm < M;
  /* the stream indices are unsigned: total < 2^31, so g0 + rows_per_piece and g + SRO_CH stay below 2^32 */
  const unsigned g0 = blockIdx.z * (unsigned)A.rows_per_piece;
  const unsigned g1 = min(g0 + (unsigned)A.rows_per_piece, (unsigned)A.total);
  unsigned cnt[SRO_SI];
#pragma unroll
  for (int r = 0; r < SRO_SI; ++r) cnt[r] = 0;
  for (unsigned g = g0; g < g1; g += SRO_CH) {
    const int n = (int)min((unsigned)SRO_CH, g1 - g);
    for (int s = wave; s < n; s += SRO_CWAVES) {
      const int k = (int)((g + s) / (unsigned)A.count), t = (int)((g + s) - (unsigned)k * (unsigned)A.count);
      const int16_t *row = A.rec + A.chain_off[k] + (long long)t * A.row_stride;
      sa[s][lane] = mok ? (int)row[cm] : 0;
      sb[s][lane] = mok ? (int)row[M + cm] : 0;
      sp[s][lane] = nok ? (int)row[2 * (long long)M + cn] : INT_MAX;
    }
    __syncthreads();
    for (int s = 0; s < n; ++s) {
      const int a = sa[s][lane], b = sb[s][lane];
#pragma unroll
      for (int r = 0; r < SRO_SI; ++r) {
        const int p = sp[s][wave * SRO_SI + r];
        cnt[r] += (a <= p) & (p < b);
      }
    }
    __syncthreads();
  }
  if (!mok) return;
#pragma unroll
  for (int r = 0; r < SRO_SI; ++r) {
    const int n = n0 + wave * SRO_SI + r;
    if (n < N && cnt[r]) atomicAdd(&A.alive[(size_t)n * M + cm], cnt[r]);
  }
}

template <bool SITE>
__global__ __launch_bounds__(SRO_THREADS) void sr_occ_margin_kernel(OccArgs A)
{
  extern __shared__ unsigned sro_lds[];   /* [SRO_THREADS] int2 staging slots, then [nh][O+1][tc] bins */
  const int M = A.M, C = A.C, O = A.O, B = O + 1, tcl = A.tcl, tc = 1 << tcl;
  const int nw = A.direct ? 0 : (A.nh * B) << tcl;
  int2 *stage = (int2 *)sro_lds;
  unsigned *bins = sro_lds + 2 * SRO_THREADS;
  for (int i = threadIdx.x; i < nw; i += SRO_THREADS) bins[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = lane & (tc - 1), sub = lane >> tcl, R = 64 >> tcl;
  const int c = (blockIdx.x << tcl) + lc;
  const bool cok = c < C;
  const int cc = cok ? c : 0;
  const int wO = (O + 63) >> 6;
  const unsigned long long *xcol = A.xbits + (size_t)cc * wO;
  int2 *grp = stage + wave * 64 + sub * tc;   /* this group's tc slots; the lane's own is grp[lc] */
  unsigned ones = 0;                          /* the column's sum of x */
  for (int w = 0; w < wO; ++w) ones += (unsigned)__popcll(xcol[w]);
  const unsigned g0 = blockIdx.y * (unsigned)A.rows_per_piece;
  const unsigned g1 = min(g0 + (unsigned)A.rows_per_piece, (unsigned)A.total);
  /* every lane of a wave makes the same trips: a group past the end walks the last row again and bins nothing */
  for (unsigned gb = g0 + wave * R; gb < g1; gb += SRO_WAVES * R) {
    const bool live = gb + sub < g1;
    const unsigned g = live ? gb + sub : g1 - 1;
    const int k = (int)(g / (unsigned)A.count), t = (int)(g - (unsigned)k * (unsigned)A.count);
    const int16_t *row = A.rec + A.chain_off[k] + (long long)t * A.row_stride;
    int p = 0, a = 0, b = 0;
    if (SITE) p = row[2 * (long long)M + cc];
    else { a = row[cc]; b = row[M + cc]; }
    unsigned cA = 0, cAX = 0;
    for (int o0 = 0; o0 < O; o0 += tc) {
      const int o = o0 + lc;
      int2 e;
      if (SITE) e = o < O ? make_int2(row[o], row[M + o]) : make_int2(0, 0);
      else e = make_int2(o < O ? (int)row[2 * (long long)M + o] : INT_MAX, 0);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      grp[lc] = e;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      unsigned long long xs = xcol[o0 >> 6] >> (o0 & 63);   /* tc divides 64: a stage stays inside one word */
#pragma unroll 8
      for (int j = 0; j < tc; ++j) {
        const int2 q = grp[j];
        const unsigned al = SITE ? (unsigned)((q.x <= p) & (p < q.y)) : (unsigned)((a <= q.x) & (q.x < b));
        cA += al;
        cAX += al & (unsigned)xs;
        xs >>= 1;
      }
    }
    if (live && cok) {
#pragma unroll
      for (int h = 0; h < 3; ++h) {   /* unrolled: the argument arrays are indexed by constants */
        if (h >= A.nh) break;
        const unsigned val = A.which[h] == 0 ? cA : (A.which[h] == 1 ? cA - cAX : ones - cAX);
        if (A.direct) atomicAdd(&A.hist[h][(size_t)c * B + val], 1u);
        else atomicAdd(&bins[((h * B + (int)val) << tcl) + lc], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nw; i += SRO_THREADS) {
    const unsigned n = bins[i];
    const int col = (blockIdx.x << tcl) + (i & (tc - 1)), q = i >> tcl, h = q / B;
    unsigned *dst = h == 0 ? A.hist[0] : (h == 1 ? A.hist[1] : A.hist[2]);
    if (n && col < C) atomicAdd(&dst[(size_t)col * B + (q - h * B)], n);
  }
}

/* X [R][Cn] (row-major bytes, non-zero = 1) packed along `walk`: out [own][(walked + 63) / 64] words */
static unsigned long long *sro_pack(const uint8_t *X, int N, int M, bool own_site, size_t *words)
{
  const int C = own_site ? N : M, O = own_site ? M : N;
  const size_t wO = ((size_t)O + 63) >> 6;
  unsigned long long *w = (unsigned long long *)calloc((size_t)C * wO, sizeof(unsigned long long));
  if (!w) return nullptr;
  for (int n = 0; n < N; ++n)
    for (int m = 0; m < M; ++m)
      if (X[(size_t)n * M + m]) {
        const int c = own_site ? n : m, o = own_site ? m : n;
        w[(size_t)c * wO + (o >> 6)] |= 1ull << (o & 63);
      }
  *words = (size_t)C * wO;
  return w;
}

/* The occupancy counts of the n_sel chains of a record view.  X [N][M] is a host input; alive [N][M], site[3]
   (alive, f0, f1: [N][M+1] each) and taxon[3] ([M][N+1] each) are host buffers, each optional. */
extern "C" int sro_occupancy(const sr_recview *v, int N, int M, const uint8_t *X, uint32_t *alive,
                             uint32_t *const site[3], uint32_t *const taxon[3], float *ms)
{
  int rc = 0;
  unsigned *d_alive = nullptr, *d_hist[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  unsigned long long *d_x[2] = {nullptr, nullptr}, *h_x = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || !X || !site || !taxon || n_sel <= 0 || count < 1 || N < 1 || N > 32767 || M < 1 ||
      (long long)n_sel * count >= (1LL << 31))
    return -1;
  if (ms) *ms = 0.0f;
  const int total = n_sel * count;
  uint32_t *const *const want[2] = {site, taxon};   /* role 0: a lane owns a site; role 1: a taxon */
  const size_t cells = (size_t)N * M * sizeof(unsigned);
  const size_t hbytes[2] = {(size_t)N * ((size_t)M + 1) * sizeof(unsigned), (size_t)M * ((size_t)N + 1) * sizeof(unsigned)};
  {
    int ncu = 0, per_cu = 0;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    if (ncu < 1) ncu = 1;
    if (alive) HIPCHK(hipMalloc(&d_alive, cells));
    for (int r = 0; r < 2; ++r) {
      if (!want[r][0] && !want[r][1] && !want[r][2]) continue;
      size_t words;
      h_x = sro_pack(X, N, M, r == 0, &words);
      if (!h_x) { rc = -4; goto done; }
      HIPCHK(hipMalloc(&d_x[r], words * sizeof(unsigned long long)));
      HIPCHK(hipMemcpy(d_x[r], h_x, words * sizeof(unsigned long long), hipMemcpyHostToDevice));
      free(h_x);
      h_x = nullptr;
      for (int q = 0; q < 3; ++q)
        if (want[r][q]) HIPCHK(hipMalloc(&d_hist[r][q], hbytes[r]));
    }
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    OccArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride;
    A.count = count; A.N = N; A.M = M; A.total = total;
    A.alive = nullptr; A.C = 0; A.O = 0; A.tcl = 0; A.direct = 0; A.nh = 0; A.xbits = nullptr;
    for (int q = 0; q < 3; ++q) { A.hist[q] = nullptr; A.which[q] = 0; }
    HIPCHK(hipEventRecord(e0, st));
    if (alive) {
      const int tx = (M + 63) / 64, ty = (N + SRO_TS - 1) / SRO_TS;
      long long nz;
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_occ_cell_kernel, SRO_CTHREADS, 0));
      if (per_cu < 1) per_cu = 1;
      A.rows_per_piece = (int)sr_pieces((long long)ncu * per_cu, (long long)tx * ty, total, SRO_MIN_ROWS, SR_GRID_CAP, &nz);
      A.alive = d_alive;
      HIPCHK(hipMemsetAsync(d_alive, 0, cells, st));
      hipLaunchKernelGGL(sr_occ_cell_kernel, dim3(tx, ty, (unsigned)nz), dim3(SRO_CTHREADS), 0, st, A);
      HIPCHK(hipGetLastError());
      A.alive = nullptr;
    }
    for (int r = 0; r < 2; ++r) {
      if (!d_x[r]) continue;
      const void *kern = r == 0 ? (const void *)sr_occ_margin_kernel<true> : (const void *)sr_occ_margin_kernel<false>;
      const size_t fixed = sizeof(int2) * SRO_THREADS;
      int fits, nh = 0;
      long long ny;
      A.C = r == 0 ? N : M; A.O = r == 0 ? M : N; A.xbits = d_x[r];
      for (int q = 0; q < 3; ++q)
        if (d_hist[r][q]) {
          A.hist[nh] = d_hist[r][q];
          A.which[nh++] = q;
          HIPCHK(hipMemsetAsync(d_hist[r][q], 0, hbytes[r], st));
        }
      int tcl = sr_lds_tile((size_t)nh * ((size_t)A.O + 1), fixed, &fits);
      const int direct = !fits;
      if (direct) tcl = 6;
      const size_t lds = fixed + (direct ? 0 : (((size_t)nh * ((size_t)A.O + 1)) << tcl) * sizeof(unsigned));
      const int tiles = (A.C + (1 << tcl) - 1) >> tcl;
      HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      if (r == 0) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_occ_margin_kernel<true>, SRO_THREADS, lds));
      else HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_occ_margin_kernel<false>, SRO_THREADS, lds));
      if (per_cu < 1) per_cu = 1;
      A.rows_per_piece = (int)sr_pieces((long long)ncu * per_cu, tiles, total, SRO_MIN_ROWS, SR_GRID_CAP, &ny);
      A.tcl = tcl; A.direct = direct; A.nh = nh;
      if (r == 0) hipLaunchKernelGGL(sr_occ_margin_kernel<true>, dim3(tiles, (unsigned)ny), dim3(SRO_THREADS), lds, st, A);
      else hipLaunchKernelGGL(sr_occ_margin_kernel<false>, dim3(tiles, (unsigned)ny), dim3(SRO_THREADS), lds, st, A);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) HIPCHK(hipEventElapsedTime(ms, e0, e1));
    if (alive) HIPCHK(hipMemcpy(alive, d_alive, cells, hipMemcpyDeviceToHost));
    for (int r = 0; r < 2; ++r)
      for (int q = 0; q < 3; ++q)
        if (want[r][q]) HIPCHK(hipMemcpy(want[r][q], d_hist[r][q], hbytes[r], hipMemcpyDeviceToHost));
  }
done:
  free(h_x);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_alive) (void)hipFree(d_alive);
  for (int r = 0; r < 2; ++r) {
    if (d_x[r]) (void)hipFree(d_x[r]);
    for (int q = 0; q < 3; ++q)
      if (d_hist[r][q]) (void)hipFree(d_hist[r][q]);
  }
  return rc;
}
