/*
 * sr_central.hip -- the central sampled state: the saved record with the smallest posterior expected loss, the
 * medoid of the draws (no counterpart in the reference: an extension, definitions in include/seriation.h "the
 * central sampled state").
 *
 * Reflection without arithmetic: a flagged chain's pi' = N - 1 - pi is only ever compared, and x -> ~x (= -x - 1)
 * reverses the order of int16 values exactly as x -> N - 1 - x does, ties included, without leaving int16's range.
 * Both order kernels stage ~pi for a flagged chain's rows and compare staged values; the limits, whose values matter,
 * are reflected in int32 (a' = N - b, b' = N - a).  Unsigned integer counts and sums throughout, no floating point:
 * the result does not depend on the order of the adds.
 *
 * Pooled pair-count kernel: sr_agree_pair_kernel's comparison "GEMM" (4 waves, one 64 x 64 tile (I, J), I <= J, lane =
 * column j, wave w owns rows i = 16 w .. 16 w + 15, SRC_CH rows staged per chunk), but over the pooled stream of all
 * T = n_sel x count rows, cut into gridDim.y pieces, and into one set of counts.  The counts go to the band scratch
 * the loss kernel reads and, when asked for, to the caller's [N][N] matrix (lt at [i][j], gt at [j][i]).
 *
 * Band scratch: [tiles][64][64][2] uint32; entry (li, lj) of a tile holds {C[i][j], C[j][i]} of one pair i < j.  The
 * entries that are no such pair (i >= j on a diagonal tile, columns beyond N) are never written and stay 0, so they
 * add 0 to every loss.  A band is a run of whole tile rows I with all their tiles J >= I, as many as keep the scratch
 * within SR_CENTRAL_SCRATCH bytes (one tile row at least); the losses simply accumulate over the bands.
 *
 * Order-loss kernel (the hot path): lane = record.  A block of 4 waves owns 64 rows and a run of the band's tiles.
 * For a tile it stages the rows' pi_i and pi_j transposed into LDS, [site][row]: a wave loads one row's 64 sites
 * coalesced (128 bytes) and stores them down a column of a 65-dword-pitch array (bank = (site + row) mod 32: no
 * conflict), and reads them back with lane = row from consecutive addresses.  Wave w takes the tile's rows i = 16 w ..
 * 16 w + 15: 16 pi_i in registers, the pi_j eight at a time, and per pair two subtractions, two shifts that spread
 * their sign bits into masks, two ANDs with the pair's counts and an add.
 * The two counts of a pair are the same address for every lane: the index is built from blockIdx, loop counters and
 * the wave number made uniform, so they are scalar loads of 16 dwords (8 pairs) off the scratch.  Lane = site pair
 * would instead need a 64-bit cross-lane reduction per (row, tile), which costs more than the tile's work.
 * Widths: a wave's share of a tile is 1024 pairs; when every count is at most 2^22 - 1 (always for pooled counts of
 * fewer than 2^22 rows) the share's sum stays below 2^32 and is accumulated in 32 bits, then added to the lane's
 * 64-bit total (NARROW); otherwise every add is 64-bit.  Fewer than 2^29 pairs and counts below 2^32: no total
 * exceeds 2^61.  The four waves' totals meet in LDS and go out as one 64-bit integer atomic per (block, row).  When
 * the rows are few the band's tiles are cut across gridDim.y so that the compute units are used.
 * On a diagonal tile the groups of eight j that lie wholly at or below a row i are skipped; the rest of the lower
 * triangle reads zeros.
 *
 * Limit loss: per batch of limit columns a histogram of the clamped, reflected values ([column][bin]; lane = column,
 * so the int16 row loads coalesce; global vector atomics), then one wave per column the table D[v] = sum_u hist[u]
 * |v - u| from the prefix sums of hist[u] and u hist[u] in int64 (shuffle scans, 64 bins at a time), then one wave
 * per row: lane = column gathers D at the row's values, a 64-bit shuffle reduction and one atomic per (row, batch).
 * A batch's histogram and table stay within the same SR_CENTRAL_SCRATCH bytes.
 *
 * The argmin over the T (order loss, limit loss) pairs and the reflection of the central row are host code.  The rows
 * are addressed through a record view (sr_records.h); src_central is the unit's entry point over records,
 * src_order_loss the order loss alone against counts in host memory.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sr_records.h"
#include "sr_analysis.h"

#define SRC_TILE 64                      /* the tile is SRC_TILE x SRC_TILE site pairs; the loss kernel's rows per block */
#define SRC_TE (SRC_TILE * SRC_TILE)     /* pairs of a tile; the scratch holds two counts each */
#define SRC_WAVES 4
#define SRC_THREADS (64 * SRC_WAVES)
#define SRC_RI (SRC_TILE / SRC_WAVES)    /* rows i per wave */
#define SRC_CH 32                        /* pair kernel: rows staged per chunk */
#define SRC_MIN_ROWS 64                  /* pair kernel: rows a block takes at least */
#define SRC_HU 4                         /* histogram kernel: rows in flight per lane */
#define SRC_HIST_ROWS 16                 /* histogram kernel: rows a block takes at least */
#define SRC_PITCH (SRC_TILE + 1)         /* loss kernel: dwords between two sites of the transposed staging */
#define SRC_JC 8                         /* loss kernel: pi_j in registers at a time */
#define SRC_NARROW_MAX 4194303u          /* 2^22 - 1: SRC_RI * SRC_TILE = 1024 such counts sum to less than 2^32 */
#define SRC_SCRATCH_DEFAULT (256LL << 20)

struct CentralRows {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *flip;           /* [n_sel] or NULL */
  unsigned count, total;         /* rows per chain, T = n_sel * count < 2^31 */
  int N, M;
};

/* S: the band's scratch, zeroed; pc [N][N], zeroed, or NULL */
__global__ __launch_bounds__(SRC_THREADS) void sr_central_pair_kernel(CentralRows A, int nt, int I0, unsigned rows_per_piece,
                                                                      unsigned *S, unsigned *pc)
{
  __shared__ int spi[SRC_CH][SRC_TILE], spj[SRC_CH][SRC_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N;
  /* the band's tiles in order: row I0 with J = I0 .. nt - 1, then row I0 + 1 with J = I0 + 1 .. nt - 1, ... */
  int I = I0, q = blockIdx.x;
  while (I < nt - 1 && q >= nt - I) { q -= nt - I; ++I; }
  const int J = I + q;
  const int i0 = I * SRC_TILE, ci = i0 + lane, cj = J * SRC_TILE + lane;
  const bool iok = ci < N, jok = cj < N;
  /* total < 2^31, so r0 + rows_per_piece and g + SRC_CH stay below 2^32 */
  const unsigned r0 = blockIdx.y * rows_per_piece;
  const unsigned r1 = min(r0 + rows_per_piece, A.total);
  const int16_t *base = A.rec + 2 * A.M;
  unsigned lt[SRC_RI], gt[SRC_RI];
#pragma unroll
  for (int r = 0; r < SRC_RI; ++r) lt[r] = gt[r] = 0;
  for (unsigned g = r0; g < r1; g += SRC_CH) {
    const int n = (int)min((unsigned)SRC_CH, r1 - g);
    for (int s = wave; s < n; s += SRC_WAVES) {
      const unsigned k = (g + s) / A.count, t = (g + s) - k * A.count;
      const bool f = A.flip && A.flip[k];
      const int16_t *row = base + A.chain_off[k] + (long long)t * A.row_stride;
      const int xi = iok ? (int)row[ci] : 0, xj = jok ? (int)row[cj] : 0;
      spi[s][lane] = iok && f ? ~xi : xi;
      spj[s][lane] = jok && f ? ~xj : xj;
    }
    __syncthreads();
    for (int s = 0; s < n; ++s) {
      const int pj = spj[s][lane];
#pragma unroll
      for (int r = 0; r < SRC_RI; ++r) {
        const int pi = spi[s][wave * SRC_RI + r];
        lt[r] += pi < pj;
        gt[r] += pi > pj;
      }
    }
    __syncthreads();
  }
  if (!jok) return;
  unsigned *tile = S + (size_t)blockIdx.x * SRC_TE * 2;
#pragma unroll
  for (int r = 0; r < SRC_RI; ++r) {
    const int li = wave * SRC_RI + r, i = i0 + li;
    if (i < N && i < cj) {   /* a pair i < j: every entry of a tile above the diagonal, half of a diagonal tile */
      if (lt[r]) atomicAdd(&tile[(li * SRC_TILE + lane) * 2], lt[r]);
      if (gt[r]) atomicAdd(&tile[(li * SRC_TILE + lane) * 2 + 1], gt[r]);
      if (pc) {
        if (lt[r]) atomicAdd(&pc[(size_t)i * N + cj], lt[r]);
        if (gt[r]) atomicAdd(&pc[(size_t)cj * N + i], gt[r]);
      }
    }
  }
}

/* S: the band's scratch [tiles][64][64][2]; loss [T], added to.  Block (x, y): rows 64 x .. 64 x + 63, the band's
   tiles [y tiles_per_piece, (y + 1) tiles_per_piece). */
template <bool NARROW>
__global__ __launch_bounds__(SRC_THREADS) void sr_central_loss_kernel(CentralRows A, int nt, int I0, int tiles,
                                                                      int tiles_per_piece,
                                                                      const unsigned *__restrict__ S,
                                                                      unsigned long long *loss)
{
  __shared__ int spi[SRC_TILE][SRC_PITCH], spj[SRC_TILE][SRC_PITCH];   /* [site][row] */
  __shared__ unsigned long long red[SRC_WAVES][SRC_TILE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = A.N;
  const unsigned g0 = blockIdx.x * (unsigned)SRC_TILE;
  /* the rows this wave stages, s = wave, wave + 4, ...: where they start, whether they are reflected */
  const int16_t *rowp[SRC_RI];
  bool rowf[SRC_RI];
#pragma unroll
  for (int x = 0; x < SRC_RI; ++x) {
    const unsigned g = g0 + wave + x * SRC_WAVES;
    rowp[x] = nullptr;
    rowf[x] = false;
    if (g < A.total) {
      const unsigned k = g / A.count, t = g - k * A.count;
      rowp[x] = A.rec + 2 * A.M + A.chain_off[k] + (long long)t * A.row_stride;
      rowf[x] = A.flip && A.flip[k];
    }
  }
  const int q0 = blockIdx.y * tiles_per_piece, q1 = min(q0 + tiles_per_piece, tiles);
  int I = I0, J;
  {
    int q = q0;
    while (I < nt - 1 && q >= nt - I) { q -= nt - I; ++I; }
    J = I + q;
  }
  unsigned long long acc = 0;
  for (int q = q0; q < q1; ++q) {
    const int ci = I * SRC_TILE + lane, cj = J * SRC_TILE + lane;
#pragma unroll
    for (int x = 0; x < SRC_RI; ++x) {
      const int s = wave + x * SRC_WAVES;
      int xi = 0, xj = 0;   /* rows beyond T and columns beyond N: ties, which add nothing */
      if (rowp[x]) {
        if (ci < N) { xi = rowp[x][ci]; if (rowf[x]) xi = ~xi; }
        if (cj < N) { xj = rowp[x][cj]; if (rowf[x]) xj = ~xj; }
      }
      spi[lane][s] = xi;
      spj[lane][s] = xj;
    }
    __syncthreads();
    int pi[SRC_RI];
#pragma unroll
    for (int r = 0; r < SRC_RI; ++r) pi[r] = spi[wave * SRC_RI + r][lane];
    const bool diag = I == J;
    const unsigned *tile = S + ((size_t)q * SRC_TE + (size_t)wave * SRC_RI * SRC_TILE) * 2;
    unsigned a32 = 0;
    for (int jc = 0; jc < SRC_TILE; jc += SRC_JC) {
      int pj[SRC_JC];
#pragma unroll
      for (int u = 0; u < SRC_JC; ++u) pj[u] = spj[jc + u][lane];
#pragma unroll
      for (int r = 0; r < SRC_RI; ++r) {
        if (diag && jc + SRC_JC - 1 <= wave * SRC_RI + r) continue;   /* no j > i among these eight */
        /* all 16 counts loaded before any is chosen: 64 bytes at a 64-byte boundary, the same for every lane */
        const uint4 *e = (const uint4 *)(tile + (r * SRC_TILE + jc) * 2);
        const uint4 e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
        const unsigned c[2 * SRC_JC] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w,
                                        e2.x, e2.y, e2.z, e2.w, e3.x, e3.y, e3.z, e3.w};
#pragma unroll
        for (int u = 0; u < SRC_JC; ++u) {
          const unsigned cij = c[2 * u], cji = c[2 * u + 1];
          /* staged values are int16's: the differences cannot wrap, and their sign bits spread are the two masks.
             The empty asm keeps them differences: as compares and selects each count, a scalar register, would
             first have to be moved into a vector register, since a select's condition takes the one scalar operand */
          int dlt = pi[r] - pj[u], dgt = pj[u] - pi[r];
          asm("" : "+v"(dlt), "+v"(dgt));
          const unsigned v = ((unsigned)(dlt >> 31) & cji) | ((unsigned)(dgt >> 31) & cij);
          if (NARROW) a32 += v;
          else acc += v;
        }
      }
    }
    if (NARROW) acc += a32;
    __syncthreads();
    if (++J == nt) { ++I; J = I; }
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < SRC_TILE) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < SRC_WAVES; ++w) v += red[w][lane];
    if (g0 + lane < A.total && v) atomicAdd(&loss[g0 + lane], v);
  }
}

/* the reflected, clamped value of limit column cc (0 .. 2M - 1) in a row of a chain with flag f, read from src */
__device__ __forceinline__ int src_limit(int x, bool f, int N) { return min(max(f ? N - x : x, 0), N); }

/* hist [ncol][N+1] of the batch's columns [col0, col0 + ncol), zeroed.  Block (x, y): columns 256 x .. 256 x + 255,
   rows [y rows_per_piece, (y + 1) rows_per_piece) of the pooled stream, SRC_HU rows' loads in flight per lane. */
__global__ __launch_bounds__(SRC_THREADS) void sr_central_hist_kernel(CentralRows A, int col0, int ncol,
                                                                      unsigned rows_per_piece, unsigned *hist)
{
  const int c = blockIdx.x * SRC_THREADS + threadIdx.x;
  if (c >= ncol) return;
  const int N = A.N, M = A.M, cc = col0 + c;
  const int fsrc = cc < M ? cc + M : cc - M;   /* a flagged chain: a reads its taxon's b, b its a */
  const unsigned r0 = blockIdx.y * rows_per_piece, r1 = min(r0 + rows_per_piece, A.total);
  if (r0 >= r1) return;
  unsigned *bins = hist + (size_t)c * (N + 1);
  for (unsigned k = r0 / A.count; k <= (r1 - 1) / A.count; ++k) {
    const unsigned cs = k * A.count;
    const unsigned t0 = max(r0, cs) - cs, t1 = min(r1, cs + A.count) - cs;
    const bool f = A.flip && A.flip[k];
    const int16_t *base = A.rec + A.chain_off[k] + (f ? fsrc : cc);
    for (unsigned t = t0; t < t1; t += SRC_HU) {
      int x[SRC_HU];
#pragma unroll
      for (unsigned u = 0; u < SRC_HU; ++u) x[u] = t + u < t1 ? (int)base[(long long)(t + u) * A.row_stride] : 0;
#pragma unroll
      for (unsigned u = 0; u < SRC_HU; ++u)
        if (t + u < t1) atomicAdd(&bins[src_limit(x[u], f, N)], 1u);
    }
  }
}

/* D [ncol][N+1]: D[c][v] = sum_u hist[c][u] |v - u| = v cle - sle + (S - sle) - v (T - cle), with cle and sle the
   sums of hist[c][u] and u hist[c][u] over u <= v and S that of u hist[c][u] over all u; every row lies in one bin, so
   a column's bins sum to T.  One wave per column: 64 bins at a time, the prefix sums by shuffles, the running sums
   carried from chunk to chunk.  cle <= T < 2^31 and v, u < 2^15: every term is below 2^46. */
__global__ __launch_bounds__(SRC_THREADS) void sr_central_table_kernel(const unsigned *__restrict__ hist, int N, int ncol,
                                                                       long long T, long long *__restrict__ D)
{
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * SRC_WAVES + (threadIdx.x >> 6);
  if (c >= ncol) return;   /* the whole wave */
  const int B = N + 1;
  const unsigned *h = hist + (size_t)c * B;
  long long S = 0;
  for (int u = lane; u < B; u += 64) S += (long long)u * h[u];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) S += __shfl_xor(S, d);
  long long carry_c = 0, carry_s = 0;
  for (int v0 = 0; v0 < B; v0 += 64) {
    const int v = v0 + lane;
    const long long x = v < B ? h[v] : 0;
    long long ic = x, is = x * v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long oc = __shfl_up(ic, d), os = __shfl_up(is, d);
      if (lane >= d) { ic += oc; is += os; }
    }
    const long long cle = carry_c + ic, sle = carry_s + is;
    if (v < B) D[(size_t)c * B + v] = v * cle - sle + (S - sle) - v * (T - cle);
    carry_c += __shfl(ic, 63);
    carry_s += __shfl(is, 63);
  }
}

/* one wave per row: loss [T], added to */
__global__ __launch_bounds__(SRC_THREADS) void sr_central_limit_kernel(CentralRows A, int col0, int ncol,
                                                                       const long long *D, unsigned long long *loss)
{
  const int lane = threadIdx.x & 63;
  const unsigned long long gl = (unsigned long long)blockIdx.x * SRC_WAVES + (threadIdx.x >> 6);
  if (gl >= A.total) return;   /* the whole wave */
  const unsigned g = (unsigned)gl, k = g / A.count, t = g - k * A.count;
  const int N = A.N, M = A.M;
  const bool f = A.flip && A.flip[k];
  const int16_t *row = A.rec + A.chain_off[k] + (long long)t * A.row_stride;
  unsigned long long sum = 0;
  for (int c = lane; c < ncol; c += 64) {
    const int cc = col0 + c;
    const int x = row[f ? (cc < M ? cc + M : cc - M) : cc];
    sum += (unsigned long long)D[(size_t)c * (N + 1) + src_limit(x, f, N)];
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) sum += __shfl_down(sum, s);
  if (lane == 0 && sum) atomicAdd(&loss[g], sum);
}

static long long src_scratch_limit(void)
{
  const char *e = getenv("SR_CENTRAL_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? v : SRC_SCRATCH_DEFAULT;
}

/* the tile rows [I0, *I1) of the band that starts at I0: as many as keep the counts within `limit` bytes, one at
   least; returns the band's tiles */
static long long src_band(int nt, int I0, long long limit, int *I1)
{
  const long long per_tile = 2LL * SRC_TE * sizeof(unsigned);
  long long tiles = nt - I0;
  int I = I0 + 1;
  while (I < nt && (tiles + nt - I) * per_tile <= limit) { tiles += nt - I; ++I; }
  *I1 = I;
  return tiles;
}

static long long src_max_band(int nt, long long limit)
{
  long long max_tiles = 0;
  for (int I0 = 0, I1; I0 < nt; I0 = I1) {
    const long long tiles = src_band(nt, I0, limit, &I1);
    if (tiles > max_tiles) max_tiles = tiles;
  }
  return max_tiles;
}

static void src_rows_of(CentralRows *A, const sr_recview *v, const uint8_t *d_flip, int N, int M)
{
  A->rec = v->rec; A->chain_off = v->chain_off; A->row_stride = v->row_stride; A->flip = d_flip;
  A->count = (unsigned)v->count; A->total = (unsigned)((long long)v->n_sel * v->count);
  A->N = N; A->M = M;
}

/* the loss kernel over one band's scratch, the tiles cut so that `resident` blocks are busy */
static hipError_t src_loss_launch(hipStream_t st, long long resident, const CentralRows &A, int nt, int I0,
                                  long long tiles, bool narrow, const unsigned *d_S, unsigned long long *d_loss)
{
  const long long groups = ((long long)A.total + SRC_TILE - 1) / SRC_TILE;
  long long np;
  const int tpp = (int)sr_pieces(resident, groups, tiles, 1, SR_GRID_CAP, &np);
  const dim3 grid((unsigned)groups, (unsigned)np);
  if (narrow)
    hipLaunchKernelGGL(sr_central_loss_kernel<true>, grid, dim3(SRC_THREADS), 0, st, A, nt, I0, (int)tiles, tpp, d_S, d_loss);
  else
    hipLaunchKernelGGL(sr_central_loss_kernel<false>, grid, dim3(SRC_THREADS), 0, st, A, nt, I0, (int)tiles, tpp, d_S, d_loss);
  return hipGetLastError();
}

static bool src_view_ok(const sr_recview *v, int N, int M)
{
  return v && v->rec && v->chain_off && v->n_sel > 0 && v->count >= 1 && N >= 1 && N <= 32767 && M >= 1 &&
         (long long)v->n_sel * v->count < (1LL << 31);
}

/* The central state of the n_sel chains of a record view.  flip [n_sel] is a host input (may be NULL); order_loss,
   limit_loss [n_sel][count], pair_counts [N][N], best [n_sel], state [2M+N] are host buffers, each optional. */
extern "C" int src_central(const sr_recview *v, int N, int M, const uint8_t *flip, long long *order_loss,
                           long long *limit_loss, uint32_t *pair_counts, int32_t *best, int32_t *state, int32_t *chain,
                           int32_t *row, float *ms)
{
  int rc = 0;
  uint8_t *d_flip = nullptr;
  unsigned *d_S = nullptr, *d_pc = nullptr, *d_hist = nullptr;
  long long *d_D = nullptr;
  unsigned long long *d_loss = nullptr;   /* order loss [T], then limit loss [T] */
  long long *h_ol = nullptr, *h_ll = nullptr;
  int16_t *h_row = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!src_view_ok(v, N, M) || !chain || !row) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (ms) *ms = 0.0f;
  const long long T = (long long)n_sel * count, W = 2LL * M + N;
  const int nt = (N + SRC_TILE - 1) / SRC_TILE;
  const long long limit = src_scratch_limit();
  const long long max_tiles = src_max_band(nt, limit);
  const size_t pc_bytes = (size_t)N * N * sizeof(unsigned), B = (size_t)N + 1;
  /* limit columns per batch: histogram and table within the scratch bound, one column at least */
  long long cb = limit / (long long)(B * (sizeof(unsigned) + sizeof(long long)));
  if (cb < 1) cb = 1;
  if (cb > 2LL * M) cb = 2LL * M;
  const long long *ol = order_loss, *ll = limit_loss;
  if (!order_loss) { h_ol = (long long *)malloc(sizeof(long long) * (size_t)T); ol = h_ol; }
  if (!limit_loss) { h_ll = (long long *)malloc(sizeof(long long) * (size_t)T); ll = h_ll; }
  h_row = (int16_t *)malloc(sizeof(int16_t) * (size_t)W);
  if (!ol || !ll || !h_row) { rc = -4; goto done; }
  {
    int ncu = 0, per_cu_p = 0, per_cu_l = 0;
    const bool narrow = T <= (long long)SRC_NARROW_MAX;   /* a pooled count is at most T */
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    if (ncu < 1) ncu = 1;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_p, sr_central_pair_kernel, SRC_THREADS, 0));
    if (narrow) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_l, sr_central_loss_kernel<true>, SRC_THREADS, 0));
    else HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_l, sr_central_loss_kernel<false>, SRC_THREADS, 0));
    if (per_cu_p < 1) per_cu_p = 1;
    if (per_cu_l < 1) per_cu_l = 1;
    if (flip) {
      HIPCHK(hipMalloc(&d_flip, n_sel));
      HIPCHK(hipMemcpy(d_flip, flip, n_sel, hipMemcpyHostToDevice));
    }
    if (pair_counts) HIPCHK(hipMalloc(&d_pc, pc_bytes));
    HIPCHK(hipMalloc(&d_S, (size_t)max_tiles * SRC_TE * 2 * sizeof(unsigned)));
    HIPCHK(hipMalloc(&d_hist, (size_t)cb * B * sizeof(unsigned)));
    HIPCHK(hipMalloc(&d_D, (size_t)cb * B * sizeof(long long)));
    HIPCHK(hipMalloc(&d_loss, 2 * (size_t)T * sizeof(unsigned long long)));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    CentralRows A;
    src_rows_of(&A, v, d_flip, N, M);
    HIPCHK(hipEventRecord(e0, st));
    HIPCHK(hipMemsetAsync(d_loss, 0, 2 * (size_t)T * sizeof(unsigned long long), st));
    if (d_pc) HIPCHK(hipMemsetAsync(d_pc, 0, pc_bytes, st));
    for (int I0 = 0, I1; I0 < nt; I0 = I1) {
      const long long tiles = src_band(nt, I0, limit, &I1);
      long long ny;   /* pieces of the pooled rows */
      const unsigned rpp = (unsigned)sr_pieces((long long)ncu * per_cu_p, tiles, T, SRC_MIN_ROWS, SR_GRID_CAP, &ny);
      HIPCHK(hipMemsetAsync(d_S, 0, (size_t)tiles * SRC_TE * 2 * sizeof(unsigned), st));
      hipLaunchKernelGGL(sr_central_pair_kernel, dim3((unsigned)tiles, (unsigned)ny), dim3(SRC_THREADS), 0, st, A, nt, I0,
                         rpp, d_S, d_pc);
      HIPCHK(hipGetLastError());
      HIPCHK(src_loss_launch(st, (long long)ncu * per_cu_l, A, nt, I0, tiles, narrow, d_S, d_loss));
    }
    for (long long col0 = 0; col0 < 2LL * M; col0 += cb) {
      const int ncol = (int)(2LL * M - col0 < cb ? 2LL * M - col0 : cb);
      const int cblocks = (ncol + SRC_THREADS - 1) / SRC_THREADS;
      long long ny;
      const unsigned rpp = (unsigned)sr_pieces(8LL * ncu, cblocks, T, SRC_HIST_ROWS, SR_GRID_CAP, &ny);
      HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)ncol * B * sizeof(unsigned), st));
      hipLaunchKernelGGL(sr_central_hist_kernel, dim3(cblocks, (unsigned)ny), dim3(SRC_THREADS), 0, st, A, (int)col0, ncol,
                         rpp, d_hist);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(sr_central_table_kernel, dim3((ncol + SRC_WAVES - 1) / SRC_WAVES), dim3(SRC_THREADS), 0, st,
                         d_hist, N, ncol, T, d_D);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(sr_central_limit_kernel, dim3((unsigned)((T + SRC_WAVES - 1) / SRC_WAVES)), dim3(SRC_THREADS), 0,
                         st, A, (int)col0, ncol, d_D, d_loss + T);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) HIPCHK(hipEventElapsedTime(ms, e0, e1));
    HIPCHK(hipMemcpy((void *)ol, d_loss, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy((void *)ll, d_loss + T, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost));
    if (pair_counts) HIPCHK(hipMemcpy(pair_counts, d_pc, pc_bytes, hipMemcpyDeviceToHost));
    /* the smallest (order loss, limit loss, k, t): ascending k and t, strict improvement only */
    int ck = 0, ct = 0;
    for (int k = 0; k < n_sel; ++k) {
      const long long *o = ol + (size_t)k * count, *l = ll + (size_t)k * count;
      int bt = 0;
      for (int t = 1; t < count; ++t)
        if (o[t] < o[bt] || (o[t] == o[bt] && l[t] < l[bt])) bt = t;
      if (best) best[k] = bt;
      const long long *co = ol + (size_t)ck * count, *cl = ll + (size_t)ck * count;
      if (k == 0 || o[bt] < co[ct] || (o[bt] == co[ct] && l[bt] < cl[ct])) { ck = k; ct = bt; }
    }
    *chain = ck;
    *row = ct;
    if (state) {
      long long off = 0;
      HIPCHK(hipMemcpy(&off, v->chain_off + ck, sizeof(off), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(h_row, v->rec + off + (long long)ct * v->row_stride, sizeof(int16_t) * (size_t)W,
                       hipMemcpyDeviceToHost));
      const bool f = flip && flip[ck];
      for (int m = 0; m < M; ++m) {
        state[m] = f ? N - (int)h_row[M + m] : (int)h_row[m];
        state[M + m] = f ? N - (int)h_row[m] : (int)h_row[M + m];
      }
      for (int n = 0; n < N; ++n) state[2 * M + n] = f ? N - 1 - (int)h_row[2 * M + n] : (int)h_row[2 * M + n];
    }
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_flip) (void)hipFree(d_flip);
  if (d_S) (void)hipFree(d_S);
  if (d_pc) (void)hipFree(d_pc);
  if (d_hist) (void)hipFree(d_hist);
  if (d_D) (void)hipFree(d_D);
  if (d_loss) (void)hipFree(d_loss);
  free(h_ol);
  free(h_ll);
  free(h_row);
  return rc;
}

/* The order loss alone, against counts in host memory: against [N][N], any uint32 values.  The host packs a band of
   the matrix into the scratch layout (both counts of every pair i < j, the other entries 0); the bands and the loss
   kernel are those of src_central. */
extern "C" int src_order_loss(const sr_recview *v, int N, int M, const uint8_t *flip, const uint32_t *against,
                              long long *order_loss, float *ms)
{
  int rc = 0;
  uint8_t *d_flip = nullptr;
  unsigned *h_S = nullptr, *d_S = nullptr;
  unsigned long long *d_loss = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!src_view_ok(v, N, M) || !against || !order_loss) return -1;
  if (ms) *ms = 0.0f;
  const int n_sel = v->n_sel;
  const long long T = (long long)n_sel * v->count;
  const int nt = (N + SRC_TILE - 1) / SRC_TILE;
  const long long limit = src_scratch_limit();
  const size_t s_bytes = (size_t)src_max_band(nt, limit) * SRC_TE * 2 * sizeof(unsigned);
  unsigned maxc = 0;
  for (size_t x = 0; x < (size_t)N * N; ++x)
    if (against[x] > maxc) maxc = against[x];
  h_S = (unsigned *)malloc(s_bytes);
  if (!h_S) return -4;
  {
    int ncu = 0, per_cu = 0;
    float total = 0.0f;
    const bool narrow = maxc <= SRC_NARROW_MAX;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    if (ncu < 1) ncu = 1;
    if (narrow) HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_central_loss_kernel<true>, SRC_THREADS, 0));
    else HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_central_loss_kernel<false>, SRC_THREADS, 0));
    if (per_cu < 1) per_cu = 1;
    if (flip) {
      HIPCHK(hipMalloc(&d_flip, n_sel));
      HIPCHK(hipMemcpy(d_flip, flip, n_sel, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&d_S, s_bytes));
    HIPCHK(hipMalloc(&d_loss, (size_t)T * sizeof(unsigned long long)));
    HIPCHK(hipMemset(d_loss, 0, (size_t)T * sizeof(unsigned long long)));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    CentralRows A;
    src_rows_of(&A, v, d_flip, N, M);
    hipStream_t st = (hipStream_t)v->stream;
    for (int I0 = 0, I1; I0 < nt; I0 = I1) {
      const long long tiles = src_band(nt, I0, limit, &I1);
      const size_t band_bytes = (size_t)tiles * SRC_TE * 2 * sizeof(unsigned);
      memset(h_S, 0, band_bytes);
      unsigned *tile = h_S;
      for (int I = I0; I < I1; ++I)
        for (int J = I; J < nt; ++J, tile += SRC_TE * 2)
          for (int li = 0; li < SRC_TILE && I * SRC_TILE + li < N; ++li) {
            const int i = I * SRC_TILE + li;
            for (int lj = 0; lj < SRC_TILE && J * SRC_TILE + lj < N; ++lj) {
              const int j = J * SRC_TILE + lj;
              if (i < j) {
                tile[(li * SRC_TILE + lj) * 2] = against[(size_t)i * N + j];
                tile[(li * SRC_TILE + lj) * 2 + 1] = against[(size_t)j * N + i];
              }
            }
          }
      float band_ms = 0.0f;
      HIPCHK(hipMemcpy(d_S, h_S, band_bytes, hipMemcpyHostToDevice));
      HIPCHK(hipEventRecord(e0, st));
      HIPCHK(src_loss_launch(st, (long long)ncu * per_cu, A, nt, I0, tiles, narrow, d_S, d_loss));
      HIPCHK(hipEventRecord(e1, st));
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipEventElapsedTime(&band_ms, e0, e1));
      total += band_ms;
    }
    if (ms) *ms = total;
    HIPCHK(hipMemcpy(order_loss, d_loss, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_flip) (void)hipFree(d_flip);
  if (d_S) (void)hipFree(d_S);
  if (d_loss) (void)hipFree(d_loss);
  free(h_S);
  return rc;
}
