/*
 * sr_agree.hip -- chain agreement: per chain the exact counts of the site pairs' orders over its saved records, and
 * the L1 distances between every two chains' counts, plain and against the mirror image (no counterpart in the
 * reference: an extension, definitions in include/seriation.h "chain agreement").
 *
 * Only the pi part of a record row is read (N int16 entries at offset 2M), and its values are only compared, in
 * int32.  Unsigned integer counts and sums throughout, no floating point: the result does not depend on the order
 * of the adds.
 *
 * Pair-count kernel: sr_rel_pair_kernel's comparison "GEMM", per chain.  A block of 4 waves owns one chain, one
 * 64 x 64 tile (I, J) of the N x N site-pair space and a piece of that chain's rows.  For a chunk of SRA_CH rows it
 * stages the tile's pi_i and pi_j into LDS as int32 (lane = column: a row's 64 positions are 128 contiguous bytes).
 * Inner loop: lane = j, wave w owns the 16 rows i = 16 w .. 16 w + 15, whose positions every lane reads from the
 * same LDS address (a broadcast); lt = pi_i < pi_j and gt = pi_i > pi_j accumulate in 2 x 16 registers per lane.
 * gt is O[j][i], so only the tiles with I <= J are launched; it is counted, not derived as count - lt, because host
 * records may hold ties.  Columns beyond N are staged as 0; what their rows and lanes count stays in registers and
 * is never added anywhere.  When tiles x chains would leave compute units idle the chain's rows are cut into
 * gridDim.z pieces; every block adds its non-zero counts with vector atomics into zeroed device memory, as
 * sr_rel.hip does.  The counts go to two places, each optional: the caller's pair_counts matrix ([n_sel][N][N]: lt
 * at [i][j], gt at [j][i]) and the band scratch the distance kernel reads.
 *
 * Band scratch: [n_sel][2][E] uint32, E = 4096 x the band's tiles; entry p of a chain holds at [0][p] O[i][j] and at
 * [1][p] O[j][i] of one pair i < j.  The entries of a tile that are no such pair (i >= j on a diagonal tile, columns
 * beyond N) are never written and stay 0 in every chain, so they add |0 - 0| to every distance.  A band is a run of
 * whole tile rows I with all their tiles J >= I, as many as keep the scratch within SR_AGREE_SCRATCH bytes (one tile
 * row at least); since a band holds both orders of its pairs, dist_mirror needs nothing from another band, and the
 * distances simply accumulate over the bands.
 *
 * Distance kernel: a block of 4 waves owns SRA_TK x SRA_TL (k, l) chain pairs and a run of scratch entries; lane =
 * entry.  A lane loads O_k[i][j] of its 8 k chains and O_l[i][j], O_l[j][i] of its 4 l chains once and forms the
 * 32 + 32 absolute differences |O_k[i][j] - O_l[i][j]| (dist) and |O_k[i][j] - O_l[j][i]| (dist_mirror).  The whole
 * (k, l) square is computed, not its upper triangle: dist_mirror is symmetric only for permutation rows.
 * Widths: one |difference| of two uint32 can reach 2^32 - 1 (2^31 - 1 for counts), so every partial sum is 64-bit
 * from the first add on: per lane, per wave (shuffles), per block (LDS), and the one 64-bit integer atomic add per
 * (k, l) and block.  Fewer than 2^29 pairs i < j exist (N <= 32767), so no sum, partial or final, over any set of
 * pairs exceeds 2^29 (2^32 - 1) < 2^61.
 *
 * The rows are addressed through a record view (sr_records.h: chain k's rows start at rec + chain_off[k], row_stride
 * apart); sra_agreement is the unit's entry point over records, sra_distances_host the reduction alone.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sr_records.h"
#include "sr_analysis.h"

#define SRA_TILE 64                      /* pair kernel: the tile is SRA_TILE x SRA_TILE site pairs */
#define SRA_TE (SRA_TILE * SRA_TILE)     /* scratch entries of a tile, per order */
#define SRA_WAVES 4
#define SRA_THREADS (64 * SRA_WAVES)
#define SRA_RI (SRA_TILE / SRA_WAVES)    /* rows i per wave */
#define SRA_CH 32                        /* rows staged per chunk: 2 x 32 x 64 int32 = 16 KB */
#define SRA_MIN_ROWS 64                  /* rows of a chain a block takes at least */
#define SRA_TK 8                         /* distance kernel: k chains x l chains of a block */
#define SRA_TL 4
#define SRA_MIN_ENTRIES (8 * SRA_THREADS) /* scratch entries a distance block takes at least */
#define SRA_SCRATCH_DEFAULT (256LL << 20)

struct AgreeArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  int count, N, pi_off;          /* rows per chain, sites, offset of pi in a row (2M) */
  int rows_per_piece;
  int nt, I0;                    /* tiles per side; the band's first tile row */
  long long E;                   /* scratch entries of the band, per chain and order */
  unsigned *scratch;             /* [n_sel][2][E], zeroed, or NULL */
  unsigned *pc;                  /* [n_sel][N][N], zeroed, or NULL */
};

__global__ __launch_bounds__(SRA_THREADS) void sr_agree_pair_kernel(AgreeArgs A)
{
  __shared__ int spi[SRA_CH][SRA_TILE], spj[SRA_CH][SRA_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N, k = blockIdx.y;
  /* the band's tiles in order: row I0 with J = I0 .. nt - 1, then row I0 + 1 with J = I0 + 1 .. nt - 1, ... */
  int I = A.I0, t = blockIdx.x;
  while (t >= A.nt - I) { t -= A.nt - I; ++I; }
  const int J = I + t;
  const int i0 = I * SRA_TILE, ci = i0 + lane, cj = J * SRA_TILE + lane;
  const bool iok = ci < N, jok = cj < N;
  /* the row indices are unsigned: count < 2^31, so r0 + rows_per_piece and g + SRA_CH stay below 2^32 */
  const unsigned r0 = blockIdx.z * (unsigned)A.rows_per_piece;
  const unsigned r1 = min(r0 + (unsigned)A.rows_per_piece, (unsigned)A.count);
  const int16_t *base = A.rec + A.chain_off[k] + A.pi_off;
  unsigned lt[SRA_RI], gt[SRA_RI];
#pragma unroll
  for (int r = 0; r < SRA_RI; ++r) lt[r] = gt[r] = 0;
  for (unsigned g = r0; g < r1; g += SRA_CH) {
    const int n = (int)min((unsigned)SRA_CH, r1 - g);
    for (int s = wave; s < n; s += SRA_WAVES) {
      const int16_t *row = base + (long long)(g + s) * A.row_stride;
      spi[s][lane] = iok ? (int)row[ci] : 0;
      spj[s][lane] = jok ? (int)row[cj] : 0;
    }
    __syncthreads();
    for (int s = 0; s < n; ++s) {
      const int pj = spj[s][lane];
#pragma unroll
      for (int r = 0; r < SRA_RI; ++r) {
        const int pi = spi[s][wave * SRA_RI + r];
        lt[r] += pi < pj;
        gt[r] += pi > pj;
      }
    }
    __syncthreads();
  }
  if (!jok) return;
  unsigned *slt = A.scratch ? A.scratch + (size_t)k * 2 * A.E + (size_t)blockIdx.x * SRA_TE : nullptr;
  unsigned *pc = A.pc ? A.pc + (size_t)k * N * N : nullptr;
#pragma unroll
  for (int r = 0; r < SRA_RI; ++r) {
    const int li = wave * SRA_RI + r, i = i0 + li;
    if (i < N && i < cj) {   /* a pair i < j: every entry of a tile above the diagonal, half of a diagonal tile */
      if (slt) {
        if (lt[r]) atomicAdd(&slt[li * SRA_TILE + lane], lt[r]);
        if (gt[r]) atomicAdd(&slt[A.E + li * SRA_TILE + lane], gt[r]);
      }
      if (pc) {
        if (lt[r]) atomicAdd(&pc[(size_t)i * N + cj], lt[r]);
        if (gt[r]) atomicAdd(&pc[(size_t)cj * N + i], gt[r]);
      }
    }
  }
}

__device__ __forceinline__ unsigned long long sra_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

/* S [n_sel][2][E]; dist, mir [n_sel][n_sel], added to */
__global__ __launch_bounds__(SRA_THREADS) void sr_agree_dist_kernel(const unsigned *S, long long E, long long per_block,
                                                                    int n_sel, unsigned long long *dist,
                                                                    unsigned long long *mir)
{
  __shared__ unsigned long long red[SRA_WAVES][2 * SRA_TK * SRA_TL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K0 = blockIdx.y * SRA_TK, L0 = blockIdx.z * SRA_TL;
  const long long p0 = blockIdx.x * per_block, p1 = min(p0 + per_block, E);
  /* chains beyond n_sel read the last chain's entries; their sums are not written */
  const unsigned *ka[SRA_TK], *la[SRA_TL];
#pragma unroll
  for (int x = 0; x < SRA_TK; ++x) ka[x] = S + (size_t)min(K0 + x, n_sel - 1) * 2 * E;
#pragma unroll
  for (int y = 0; y < SRA_TL; ++y) la[y] = S + (size_t)min(L0 + y, n_sel - 1) * 2 * E;
  unsigned long long d[SRA_TK][SRA_TL], m[SRA_TK][SRA_TL];   /* 64-bit from the first add (see the head comment) */
#pragma unroll
  for (int x = 0; x < SRA_TK; ++x)
#pragma unroll
    for (int y = 0; y < SRA_TL; ++y) d[x][y] = m[x][y] = 0;
  for (long long p = p0 + threadIdx.x; p < p1; p += SRA_THREADS) {
    unsigned a[SRA_TK], bl[SRA_TL], bg[SRA_TL];
#pragma unroll
    for (int x = 0; x < SRA_TK; ++x) a[x] = ka[x][p];
#pragma unroll
    for (int y = 0; y < SRA_TL; ++y) { bl[y] = la[y][p]; bg[y] = la[y][E + p]; }
#pragma unroll
    for (int x = 0; x < SRA_TK; ++x)
#pragma unroll
      for (int y = 0; y < SRA_TL; ++y) {
        d[x][y] += sra_absdiff(a[x], bl[y]);
        m[x][y] += sra_absdiff(a[x], bg[y]);
      }
  }
#pragma unroll
  for (int x = 0; x < SRA_TK; ++x)
#pragma unroll
    for (int y = 0; y < SRA_TL; ++y) {
      unsigned long long vd = d[x][y], vm = m[x][y];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        vd += __shfl_down(vd, s);
        vm += __shfl_down(vm, s);
      }
      if (lane == 0) {
        red[wave][x * SRA_TL + y] = vd;
        red[wave][SRA_TK * SRA_TL + x * SRA_TL + y] = vm;
      }
    }
  __syncthreads();
  if (threadIdx.x < 2 * SRA_TK * SRA_TL) {
    const int e = threadIdx.x % (SRA_TK * SRA_TL), k = K0 + e / SRA_TL, l = L0 + e % SRA_TL;
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < SRA_WAVES; ++w) v += red[w][threadIdx.x];
    if (k < n_sel && l < n_sel && v)
      atomicAdd(threadIdx.x < SRA_TK * SRA_TL ? &dist[(size_t)k * n_sel + l] : &mir[(size_t)k * n_sel + l], v);
  }
}

static long long sra_scratch_limit(void)
{
  const char *e = getenv("SR_AGREE_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? v : SRA_SCRATCH_DEFAULT;
}

/* the tile rows [I0, *I1) of the band that starts at I0: as many as keep n_sel chains' counts within `limit` bytes,
   one at least; returns the band's tiles */
static long long sra_band(int nt, int I0, int n_sel, long long limit, int *I1)
{
  const long long per_tile = (long long)n_sel * 2 * SRA_TE * sizeof(unsigned);
  long long tiles = nt - I0;
  int I = I0 + 1;
  while (I < nt && (tiles + nt - I) * per_tile <= limit) { tiles += nt - I; ++I; }
  *I1 = I;
  return tiles;
}

static hipError_t sra_dist_launch(hipStream_t st, int resident, const unsigned *d_S, long long E, int n_sel,
                                  unsigned long long *d_dist, unsigned long long *d_mir)
{
  const int nk = (n_sel + SRA_TK - 1) / SRA_TK, nl = (n_sel + SRA_TL - 1) / SRA_TL;
  long long nx = resident / ((long long)nk * nl), nmax = E / SRA_MIN_ENTRIES;
  if (nx > nmax) nx = nmax;
  if (nx < 1) nx = 1;
  long long per_block = (E + nx - 1) / nx;
  per_block = (per_block + SRA_THREADS - 1) / SRA_THREADS * SRA_THREADS;
  nx = (E + per_block - 1) / per_block;
  hipLaunchKernelGGL(sr_agree_dist_kernel, dim3((unsigned)nx, nk, nl), dim3(SRA_THREADS), 0, st, d_S, E, per_block,
                     n_sel, d_dist, d_mir);
  return hipGetLastError();
}

/* The agreement of the n_sel chains of a record view.  pair_counts [n_sel][N][N], dist and dist_mirror
   [n_sel][n_sel] are host buffers, each optional. */
extern "C" int sra_agreement(const sr_recview *v, int N, int M, uint32_t *pair_counts, long long *dist,
                             long long *dist_mirror, float *ms)
{
  int rc = 0;
  unsigned *d_S = nullptr, *d_pc = nullptr;
  unsigned long long *d_dm = nullptr;   /* dist, then dist_mirror */
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || n_sel <= 0 || n_sel > 4096 || count < 1 || N < 1 || N > 32767 || M < 1) return -1;
  if (ms) *ms = 0.0f;
  const bool want_d = dist || dist_mirror;
  const int nt = (N + SRA_TILE - 1) / SRA_TILE;
  const size_t nn = (size_t)n_sel * n_sel, pc_bytes = (size_t)n_sel * N * N * sizeof(unsigned);
  /* without distances there is no scratch to bound: one band of all tile rows */
  const long long limit = want_d ? sra_scratch_limit() : (long long)((~0ull) >> 1);
  long long max_tiles = 0;
  for (int I0 = 0, I1; I0 < nt; I0 = I1) {
    const long long tiles = sra_band(nt, I0, n_sel, limit, &I1);
    if (tiles > max_tiles) max_tiles = tiles;
  }
  {
    int ncu = 0, per_cu = 0, per_cu_d = 0;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, v->device));
    if (ncu < 1) ncu = 1;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sr_agree_pair_kernel, SRA_THREADS, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, sr_agree_dist_kernel, SRA_THREADS, 0));
    if (per_cu < 1) per_cu = 1;
    if (per_cu_d < 1) per_cu_d = 1;
    if (pair_counts) HIPCHK(hipMalloc(&d_pc, pc_bytes));
    if (want_d) {
      HIPCHK(hipMalloc(&d_S, (size_t)n_sel * 2 * max_tiles * SRA_TE * sizeof(unsigned)));
      HIPCHK(hipMalloc(&d_dm, 2 * nn * sizeof(unsigned long long)));
    }
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    AgreeArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride;
    A.count = count; A.N = N; A.pi_off = 2 * M; A.nt = nt;
    A.scratch = d_S; A.pc = d_pc;
    HIPCHK(hipEventRecord(e0, st));
    if (d_pc) HIPCHK(hipMemsetAsync(d_pc, 0, pc_bytes, st));
    if (d_dm) HIPCHK(hipMemsetAsync(d_dm, 0, 2 * nn * sizeof(unsigned long long), st));
    for (int I0 = 0, I1; I0 < nt; I0 = I1) {
      const long long tiles = sra_band(nt, I0, n_sel, limit, &I1);
      long long nz;   /* pieces of a chain's rows */
      A.rows_per_piece = (int)sr_pieces((long long)ncu * per_cu, tiles * n_sel, count, SRA_MIN_ROWS, SR_GRID_CAP, &nz);
      A.I0 = I0;
      A.E = tiles * SRA_TE;
      if (d_S) HIPCHK(hipMemsetAsync(d_S, 0, (size_t)n_sel * 2 * A.E * sizeof(unsigned), st));
      hipLaunchKernelGGL(sr_agree_pair_kernel, dim3((unsigned)tiles, n_sel, (unsigned)nz), dim3(SRA_THREADS), 0, st, A);
      HIPCHK(hipGetLastError());
      if (d_S) HIPCHK(sra_dist_launch(st, ncu * per_cu_d, d_S, A.E, n_sel, d_dm, d_dm + nn));
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) HIPCHK(hipEventElapsedTime(ms, e0, e1));
    if (pair_counts) HIPCHK(hipMemcpy(pair_counts, d_pc, pc_bytes, hipMemcpyDeviceToHost));
    if (dist) HIPCHK(hipMemcpy(dist, d_dm, nn * sizeof(long long), hipMemcpyDeviceToHost));
    if (dist_mirror) HIPCHK(hipMemcpy(dist_mirror, d_dm + nn, nn * sizeof(long long), hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_S) (void)hipFree(d_S);
  if (d_pc) (void)hipFree(d_pc);
  if (d_dm) (void)hipFree(d_dm);
  return rc;
}

/* The distances alone, from pair counts in host memory: pair_counts [n_sel][N][N], any uint32 values.  The host
   packs a band of the matrices into the scratch layout (both orders of every pair i < j, the other entries 0); the
   bands and the distance kernel are those of sra_agreement. */
extern "C" int sra_distances_host(int device, int N, int n_sel, const uint32_t *pair_counts, long long *dist,
                                  long long *dist_mirror, float *ms)
{
  int rc = 0;
  unsigned *h_S = nullptr, *d_S = nullptr;
  unsigned long long *d_dm = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!pair_counts || n_sel <= 0 || n_sel > 4096 || N < 1 || N > 32767) return -1;
  if (ms) *ms = 0.0f;
  const int nt = (N + SRA_TILE - 1) / SRA_TILE;
  const size_t nn = (size_t)n_sel * n_sel;
  const long long limit = sra_scratch_limit();
  long long max_tiles = 0;
  for (int I0 = 0, I1; I0 < nt; I0 = I1) {
    const long long tiles = sra_band(nt, I0, n_sel, limit, &I1);
    if (tiles > max_tiles) max_tiles = tiles;
  }
  const size_t s_bytes = (size_t)n_sel * 2 * max_tiles * SRA_TE * sizeof(unsigned);
  h_S = (unsigned *)malloc(s_bytes);
  if (!h_S) return -4;
  {
    int ncu = 0, per_cu_d = 0;
    float total = 0.0f;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    if (ncu < 1) ncu = 1;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, sr_agree_dist_kernel, SRA_THREADS, 0));
    if (per_cu_d < 1) per_cu_d = 1;
    HIPCHK(hipMalloc(&d_S, s_bytes));
    HIPCHK(hipMalloc(&d_dm, 2 * nn * sizeof(unsigned long long)));
    HIPCHK(hipMemset(d_dm, 0, 2 * nn * sizeof(unsigned long long)));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int I0 = 0, I1; I0 < nt; I0 = I1) {
      const long long tiles = sra_band(nt, I0, n_sel, limit, &I1), E = tiles * SRA_TE;
      const size_t band_bytes = (size_t)n_sel * 2 * E * sizeof(unsigned);
      memset(h_S, 0, band_bytes);
      for (int k = 0; k < n_sel; ++k) {
        const uint32_t *O = pair_counts + (size_t)k * N * N;
        unsigned *slt = h_S + (size_t)k * 2 * E;
        for (int I = I0; I < I1; ++I)
          for (int J = I; J < nt; ++J, slt += SRA_TE)
            for (int li = 0; li < SRA_TILE && I * SRA_TILE + li < N; ++li) {
              const int i = I * SRA_TILE + li;
              for (int lj = 0; lj < SRA_TILE && J * SRA_TILE + lj < N; ++lj) {
                const int j = J * SRA_TILE + lj;
                if (i < j) {
                  slt[li * SRA_TILE + lj] = O[(size_t)i * N + j];
                  slt[E + li * SRA_TILE + lj] = O[(size_t)j * N + i];
                }
              }
            }
      }
      float band_ms = 0.0f;
      HIPCHK(hipMemcpy(d_S, h_S, band_bytes, hipMemcpyHostToDevice));
      HIPCHK(hipEventRecord(e0, nullptr));
      HIPCHK(sra_dist_launch(nullptr, ncu * per_cu_d, d_S, E, n_sel, d_dm, d_dm + nn));
      HIPCHK(hipEventRecord(e1, nullptr));
      HIPCHK(hipStreamSynchronize(nullptr));
      HIPCHK(hipEventElapsedTime(&band_ms, e0, e1));
      total += band_ms;
    }
    if (ms) *ms = total;
    if (dist) HIPCHK(hipMemcpy(dist, d_dm, nn * sizeof(long long), hipMemcpyDeviceToHost));
    if (dist_mirror) HIPCHK(hipMemcpy(dist_mirror, d_dm + nn, nn * sizeof(long long), hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_S) (void)hipFree(d_S);
  if (d_dm) (void)hipFree(d_dm);
  free(h_S);
  return rc;
}
