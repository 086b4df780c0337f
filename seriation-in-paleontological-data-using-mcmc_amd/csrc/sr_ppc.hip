/*
 * sr_ppc.hip -- posterior predictive checks over the saved records (no counterpart in the reference: an extension,
 * definitions in include/seriation.h "Posterior predictive checks").
 *
 * For every saved sample and replicate a 0/1 matrix is drawn from the model at the sample's (pi, a, b, c, d) -- one
 * Philox4x32-10 call per site and four consecutive taxa, counter {site, taxon >> 2, sample, replicate} -- and five
 * discrepancies per taxon, the row sums per site and the totals are compared with the same discrepancies of X under
 * the same sample.  Everything is an integer: the only floating point is the table of thresholds, and the tallies
 * are integer atomics, exact in any order.
 *
 * Table kernel: one thread per sample and taxon evaluates sr_exp_m on the c, d rows copied from the host and writes
 * the two 64-bit thresholds [sample][alive, dead][Mt], Mt = 1 (shared rates) or M.
 *
 * Main kernel: a workgroup is one wave; a lane owns one quad of taxa (SRQ_TILE = 256 taxa per workgroup) and walks
 * the sites, for a piece of the batch's samples (sr_pieces).  Per sample it keeps its four taxa's limits and
 * thresholds in registers; the observed pass reads one byte per site (X packed four taxa to a byte, [N][MQ], lanes on
 * consecutive bytes) and pi_n (one address for the whole wave), the replicate passes read pi_n alone and make one
 * Philox call per site.  Per taxon it counts ones, alive-and-one and the smallest and largest position of a one;
 * false zeros and false ones follow from the sample's alive count.  gt, eq and the sums stay in registers for the
 * whole piece and leave in one atomic each at its end.  The row sums of a replicate need every taxon tile: each wave
 * adds the population counts of its four compare masks to an HBM scratch [sample][replicate][N]; the per-sample
 * totals are reduced across the wave and added to [sample][1 + replicates][4].  The tally kernels then compare the
 * row sums with X's and the totals with the observed ones.
 *
 * The scratch and the tables are bounded: the samples are taken in batches of at most SR_PPC_SCRATCH bytes (256 MiB
 * unless the environment says otherwise); nothing depends on the batching.
 *
 * The rows are addressed through a record view (sr_records.h); srq_ppc is the unit's one entry point.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sr_records.h"
#include "sr_analysis.h"
#include "sr_math.h"
#include "sr_rng.h"

#define SRQ_QUADS 64                     /* quads of taxa per workgroup: one per lane */
#define SRQ_TILE (4 * SRQ_QUADS)         /* taxa per workgroup */
#define SRQ_MIN_ROWS 4                   /* samples per piece at least */
#define SRQ_RESIDENT 2048                /* waves in flight the pieces are cut for: 256 CUs x 4 SIMDs x 2 */
#define SRQ_TAB_THREADS 256
#define SRQ_TALLY_THREADS 256
#define SRQ_TALLY_ROWS 64                /* scratch rows (sample, replicate) per site-tally block */
#define SRQ_KEY1 0x50504331u             /* "PPC1": apart from SR_PHILOX_KEY1, the sampler's */
#define SRQ_SCRATCH_DEFAULT (256LL << 20)

typedef unsigned long long u64;

__constant__ uint64_t q_exp_tab[256] = SR_EXP_TAB_INIT;

/* thr [ns][2][Mt] from cd [ns][cdw]: c at [m], d at [Mt + m]; alive then dead */
__global__ __launch_bounds__(SRQ_TAB_THREADS) void sr_ppc_table_kernel(const double *cd, int cdw, int Mt, long long ns,
                                                                        u64 *thr)
{
  const long long i = (long long)blockIdx.x * SRQ_TAB_THREADS + threadIdx.x;
  if (i >= ns * Mt) return;
  const long long s = i / Mt;
  const int m = (int)(i - s * Mt);
  sr_mtab tb;
  tb.exp_tab = q_exp_tab; tb.log_tab = nullptr;
  const double ec = sr_exp_m(cd[s * cdw + m], &tb), ed = sr_exp_m(cd[s * cdw + Mt + m], &tb);
  thr[(size_t)s * 2 * Mt + m] = (u64)((1.0 - ed) * 4294967296.0);
  thr[(size_t)s * 2 * Mt + Mt + m] = (u64)(ec * 4294967296.0);
}

struct PpcArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *Xq;             /* [N][MQ]: bit j of a byte is X[n][4 q + j] != 0 */
  const u64 *thr;                /* [ns][2][Mt]: this batch's */
  unsigned *rich;                /* [ns][reps][N] zeroed, or NULL: no site output is wanted */
  u64 *tot;                      /* [ns][1 + reps][4] zeroed: ones, span, f0, f1 of X, then of each replicate */
  unsigned *tgt, *teq;           /* [5][M] */
  u64 *tso, *tsr;                /* [4][M]: ones, span, f0, f1 */
  long long t0;                  /* the batch's first sample */
  int N, M, MQ, count, reps, ns, rpp;
  uint32_t key0, key1;
};

__device__ __forceinline__ int srq_wave_sum(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* ones, span, gaps, f0, f1 from the counts of one taxon */
__device__ __forceinline__ void srq_stats(int ones, int mn, int mx, int alive, int both, int st[5])
{
  st[0] = ones;
  st[1] = ones ? mx - mn + 1 : 0;
  st[2] = st[1] - ones;
  st[3] = alive - both;
  st[4] = ones - both;
}

template <bool MANY>
__global__ __launch_bounds__(64) void sr_ppc_kernel(PpcArgs A)
{
  const int lane = threadIdx.x, q = blockIdx.x * SRQ_QUADS + lane, m0 = 4 * q;
  const int N = A.N, M = A.M, MQ = A.MQ, Mt = MANY ? M : 1, reps = A.reps;
  const bool qok = q < MQ;
  const int s0 = blockIdx.y * A.rpp, s1 = min(A.ns, s0 + A.rpp);
  unsigned gt[4][5], eq[4][5];
  long long so[4][4], sr[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 5; ++i) gt[j][i] = eq[j][i] = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) so[j][i] = sr[j][i] = 0;
  }
  for (int s = s0; s < s1; ++s) {
    const long long t = A.t0 + s;
    const int k = (int)(t / A.count), r = (int)(t - (long long)k * A.count);
    const int16_t *row = A.rec + A.chain_off[k] + (long long)r * A.row_stride;
    const int16_t *pi = row + 2 * M;
    const u64 *th = A.thr + (size_t)s * 2 * Mt;
    int a[4], b[4];
    u64 ta[4], td[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + j;
      const bool ok = m < M;      /* a taxon beyond M: never alive, never one */
      a[j] = ok ? (int)row[m] : 0;
      b[j] = ok ? (int)row[M + m] : 0;
      ta[j] = ok ? th[MANY ? m : 0] : 0ull;
      td[j] = ok ? th[Mt + (MANY ? m : 0)] : 0ull;
    }
    /* X under this sample */
    int obs[4][5], nal[4];
    {
      int c1[4], cb[4], mn[4], mx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { c1[j] = cb[j] = nal[j] = 0; mn[j] = 32768; mx[j] = -32769; }
      for (int n = 0; n < N; ++n) {
        const int p = pi[n];
        const int xq = qok ? (int)A.Xq[(size_t)n * MQ + q] : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool alive = a[j] <= p && p < b[j], x = (xq >> j) & 1;
          c1[j] += x;
          cb[j] += alive && x;
          nal[j] += alive;
          mn[j] = x ? min(mn[j], p) : mn[j];
          mx[j] = x ? max(mx[j], p) : mx[j];
        }
      }
      int tt[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        srq_stats(c1[j], mn[j], mx[j], nal[j], cb[j], obs[j]);
        tt[0] += obs[j][0]; tt[1] += obs[j][1]; tt[2] += obs[j][3]; tt[3] += obs[j][4];
        so[j][0] += (long long)reps * obs[j][0]; so[j][1] += (long long)reps * obs[j][1];
        so[j][2] += (long long)reps * obs[j][3]; so[j][3] += (long long)reps * obs[j][4];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int w = srq_wave_sum(tt[i]);
        if (lane == 0 && w) atomicAdd(A.tot + ((size_t)s * (1 + reps)) * 4 + i, (u64)w);
      }
    }
    for (int rep = 0; rep < reps; ++rep) {
      int c1[4], cb[4], mn[4], mx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { c1[j] = cb[j] = 0; mn[j] = 32768; mx[j] = -32769; }
      unsigned *rich = A.rich ? A.rich + ((size_t)s * reps + rep) * N : nullptr;
      const uint32_t key[2] = {A.key0, A.key1};
      for (int n = 0; n < N; ++n) {
        const int p = pi[n];
        const uint32_t ctr[4] = {(uint32_t)n, (uint32_t)q, (uint32_t)t, (uint32_t)rep};
        uint32_t w[4];
        sr_philox4x32_10(ctr, key, w);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool alive = a[j] <= p && p < b[j];
          const bool y = (u64)w[j] < (alive ? ta[j] : td[j]);
          c1[j] += y;
          cb[j] += alive && y;
          mn[j] = y ? min(mn[j], p) : mn[j];
          mx[j] = y ? max(mx[j], p) : mx[j];
          if (rich) cnt += __popcll(__ballot(y));
        }
        if (rich && lane == 0 && cnt) atomicAdd(rich + n, (unsigned)cnt);
      }
      int tt[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int st[5];
        srq_stats(c1[j], mn[j], mx[j], nal[j], cb[j], st);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          gt[j][i] += st[i] > obs[j][i];
          eq[j][i] += st[i] == obs[j][i];
        }
        tt[0] += st[0]; tt[1] += st[1]; tt[2] += st[3]; tt[3] += st[4];
        sr[j][0] += st[0]; sr[j][1] += st[1]; sr[j][2] += st[3]; sr[j][3] += st[4];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int w = srq_wave_sum(tt[i]);
        if (lane == 0 && w) atomicAdd(A.tot + ((size_t)s * (1 + reps) + 1 + rep) * 4 + i, (u64)w);
      }
    }
  }
  if (s1 <= s0) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + j;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if (gt[j][i]) atomicAdd(A.tgt + (size_t)i * M + m, gt[j][i]);
      if (eq[j][i]) atomicAdd(A.teq + (size_t)i * M + m, eq[j][i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (so[j][i]) atomicAdd(A.tso + (size_t)i * M + m, (u64)so[j][i]);
      if (sr[j][i]) atomicAdd(A.tsr + (size_t)i * M + m, (u64)sr[j][i]);
    }
  }
}

/* the replicates' row sums rich [rows][N] against X's: block (x, y) takes sites x * 256.. and SRQ_TALLY_ROWS rows */
__global__ __launch_bounds__(SRQ_TALLY_THREADS) void sr_ppc_site_kernel(const unsigned *rich, const unsigned *rich_obs,
                                                                          long long rows, int N, unsigned *sgt,
                                                                          unsigned *seq, u64 *ssum)
{
  const int n = blockIdx.x * SRQ_TALLY_THREADS + threadIdx.x;
  if (n >= N) return;
  const long long e0 = (long long)blockIdx.y * SRQ_TALLY_ROWS, e1 = min(rows, e0 + SRQ_TALLY_ROWS);
  const unsigned ro = rich_obs[n];
  unsigned g = 0, q = 0;
  u64 sum = 0;
  for (long long e = e0; e < e1; ++e) {
    const unsigned v = rich[(size_t)e * N + n];
    g += v > ro;
    q += v == ro;
    sum += v;
  }
  if (g) atomicAdd(sgt + n, g);
  if (q) atomicAdd(seq + n, q);
  if (sum) atomicAdd(ssum + n, sum);
}

/* the per-sample totals tot [ns][1 + reps][4] as the interface's five, tobs [ns][5] and trep [ns][reps][5], and the
   tallies of replicate against X over the batch's (sample, replicate) pairs added to tgt[5], teq[5] */
__global__ __launch_bounds__(SRQ_TALLY_THREADS) void sr_ppc_total_kernel(const u64 *tot, long long ns, int reps,
                                                                           long long *tobs, long long *trep, u64 *tgt,
                                                                           u64 *teq)
{
  const long long e = (long long)blockIdx.x * SRQ_TALLY_THREADS + threadIdx.x;
  const bool ok = e < ns * reps;
  long long o[5] = {0, 0, 0, 0, 0}, v[5] = {0, 0, 0, 0, 0};
  if (ok) {
    const long long s = e / reps;
    const int rep = (int)(e - s * reps);
    const u64 *po = tot + (size_t)s * (1 + reps) * 4, *pv = po + (size_t)(1 + rep) * 4;
    o[0] = (long long)po[0]; o[1] = (long long)po[1]; o[2] = o[1] - o[0]; o[3] = (long long)po[2]; o[4] = (long long)po[3];
    v[0] = (long long)pv[0]; v[1] = (long long)pv[1]; v[2] = v[1] - v[0]; v[3] = (long long)pv[2]; v[4] = (long long)pv[3];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if (rep == 0) tobs[s * 5 + i] = o[i];
      trep[e * 5 + i] = v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int g = __popcll(__ballot(ok && v[i] > o[i])), q = __popcll(__ballot(ok && v[i] == o[i]));
    if ((threadIdx.x & 63) == 0) {
      if (g) atomicAdd(tgt + i, (u64)g);
      if (q) atomicAdd(teq + i, (u64)q);
    }
  }
}

static long long srq_scratch(void)
{
  const char *e = getenv("SR_PPC_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? v : SRQ_SCRATCH_DEFAULT;
}

/* Posterior predictive checks of the n_sel chains of a record view.  X [N][M] and cd [n_sel] (each chain's
   [count][cdw] rows: c at [m], d at [Mt + m], Mt = M when manycd, else 1) are host inputs, already checked; the
   outputs are host buffers, each optional but total_gt and total_eq [5]: taxon_gt, taxon_eq, taxon_sum_obs,
   taxon_sum_rep [5][M], site_gt, site_eq, site_sum_rep [N], total_obs [n_sel][count][5], total_rep
   [n_sel][count][reps][5]. */
extern "C" int srq_ppc(const sr_recview *v, int N, int M, const uint8_t *X, const double *const *cd, int cdw,
                       int manycd, uint64_t seed, int reps, uint32_t *taxon_gt, uint32_t *taxon_eq,
                       long long *taxon_sum_obs, long long *taxon_sum_rep, uint32_t *site_gt, uint32_t *site_eq,
                       long long *site_sum_rep, long long *total_obs, long long *total_rep, long long *total_gt,
                       long long *total_eq, float *ms)
{
  int rc = 0;
  uint8_t *h_xq = nullptr, *d_xq = nullptr;
  unsigned *h_ro = nullptr, *d_ro = nullptr, *d_rich = nullptr, *d_t32 = nullptr, *d_s32 = nullptr;
  u64 *d_thr = nullptr, *d_tot = nullptr, *d_t64 = nullptr, *d_s64 = nullptr, *d_g = nullptr;
  long long *d_t5 = nullptr, *h64 = nullptr;
  double *d_cd = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || !X || !cd || !total_gt || !total_eq || n_sel <= 0 || count < 1 || N < 1 ||
      N > 32767 || M < 1 || reps < 1 || reps > 64 || (long long)n_sel * count * reps >= (1LL << 31) ||
      (long long)N * M > (1LL << 27))
    return -1;
  if (ms) *ms = 0.0f;
  const long long T = (long long)n_sel * count;
  const int MQ = (M + 3) / 4, Mt = manycd ? M : 1;
  const bool sites = site_gt || site_eq || site_sum_rep;
  /* a batch's sample: its row sums, its totals (four kept, five given out), its thresholds and its c, d row */
  const long long per = (long long)reps * N * 4 + (1 + reps) * (4 + 5) * 8 + 2LL * Mt * 8 + (long long)cdw * 8;
  long long SB = srq_scratch() / per;
  if (SB > T) SB = T;
  if (SB > (1LL << 24)) SB = 1LL << 24;
  if (SB < 1) SB = 1;
  const unsigned tiles = (unsigned)((MQ + SRQ_QUADS - 1) / SRQ_QUADS);
  float total_ms = 0.0f;
  {
    /* X four taxa to a byte, and its row sums */
    h_xq = (uint8_t *)calloc((size_t)N * MQ, 1);
    h_ro = (unsigned *)calloc((size_t)N, sizeof(unsigned));
    h64 = (long long *)malloc(sizeof(long long) * 4 * (size_t)M);
    if (!h_xq || !h_ro || !h64) { rc = -4; goto done; }
    for (int n = 0; n < N; ++n)
      for (int m = 0; m < M; ++m)
        if (X[(size_t)n * M + m]) {
          h_xq[(size_t)n * MQ + (m >> 2)] |= (uint8_t)(1u << (m & 3));
          h_ro[n]++;
        }
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMalloc(&d_xq, (size_t)N * MQ));
    HIPCHK(hipMalloc(&d_ro, sizeof(unsigned) * N));
    HIPCHK(hipMemcpy(d_xq, h_xq, (size_t)N * MQ, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ro, h_ro, sizeof(unsigned) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&d_cd, sizeof(double) * SB * cdw));
    HIPCHK(hipMalloc(&d_thr, sizeof(u64) * SB * 2 * Mt));
    HIPCHK(hipMalloc(&d_tot, sizeof(u64) * SB * (1 + reps) * 4));
    HIPCHK(hipMalloc(&d_t5, sizeof(long long) * SB * (1 + reps) * 5));   /* tobs [SB][5], then trep [SB][reps][5] */
    if (sites) HIPCHK(hipMalloc(&d_rich, sizeof(unsigned) * SB * reps * N));
    HIPCHK(hipMalloc(&d_t32, sizeof(unsigned) * 10 * M));                /* taxon gt, eq [5][M] */
    HIPCHK(hipMalloc(&d_t64, sizeof(u64) * 8 * M));                      /* taxon sums of X, of replicates [4][M] */
    HIPCHK(hipMalloc(&d_s32, sizeof(unsigned) * 2 * N));                 /* site gt, eq */
    HIPCHK(hipMalloc(&d_s64, sizeof(u64) * N));
    HIPCHK(hipMalloc(&d_g, sizeof(u64) * 10));                           /* total gt, eq [5] */
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipMemsetAsync(d_t32, 0, sizeof(unsigned) * 10 * M, st));
    HIPCHK(hipMemsetAsync(d_t64, 0, sizeof(u64) * 8 * M, st));
    HIPCHK(hipMemsetAsync(d_s32, 0, sizeof(unsigned) * 2 * N, st));
    HIPCHK(hipMemsetAsync(d_s64, 0, sizeof(u64) * N, st));
    HIPCHK(hipMemsetAsync(d_g, 0, sizeof(u64) * 10, st));
    PpcArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride; A.Xq = d_xq; A.thr = d_thr;
    A.rich = d_rich; A.tot = d_tot; A.tgt = d_t32; A.teq = d_t32 + (size_t)5 * M; A.tso = d_t64;
    A.tsr = d_t64 + (size_t)4 * M; A.N = N; A.M = M; A.MQ = MQ; A.count = count; A.reps = reps;
    A.key0 = (uint32_t)seed; A.key1 = (uint32_t)(seed >> 32) ^ SRQ_KEY1;
    for (long long t0 = 0; t0 < T; t0 += SB) {
      const long long ns = SB < T - t0 ? SB : T - t0;
      /* the batch's c, d rows: sample t is row t % count of chain t / count */
      for (long long t = t0; t < t0 + ns;) {
        const long long k = t / count, r = t - k * count;
        const long long nr = count - r < t0 + ns - t ? count - r : t0 + ns - t;
        HIPCHK(hipMemcpyAsync(d_cd + (size_t)(t - t0) * cdw, cd[k] + (size_t)r * cdw, sizeof(double) * nr * cdw,
                              hipMemcpyHostToDevice, st));
        t += nr;
      }
      HIPCHK(hipMemsetAsync(d_tot, 0, sizeof(u64) * ns * (1 + reps) * 4, st));
      if (sites) HIPCHK(hipMemsetAsync(d_rich, 0, sizeof(unsigned) * ns * reps * N, st));
      long long pieces = 1;
      const long long rpp = sr_pieces(SRQ_RESIDENT, tiles, ns, SRQ_MIN_ROWS, SR_GRID_CAP, &pieces);
      A.t0 = t0; A.ns = (int)ns; A.rpp = (int)rpp;
      HIPCHK(hipEventRecord(e0, st));
      hipLaunchKernelGGL(sr_ppc_table_kernel, dim3((unsigned)((ns * Mt + SRQ_TAB_THREADS - 1) / SRQ_TAB_THREADS)),
                         dim3(SRQ_TAB_THREADS), 0, st, d_cd, cdw, Mt, ns, d_thr);
      HIPCHK(hipGetLastError());
      if (manycd) hipLaunchKernelGGL((sr_ppc_kernel<true>), dim3(tiles, (unsigned)pieces), dim3(64), 0, st, A);
      else hipLaunchKernelGGL((sr_ppc_kernel<false>), dim3(tiles, (unsigned)pieces), dim3(64), 0, st, A);
      HIPCHK(hipGetLastError());
      const long long rows = ns * reps;
      if (sites) {
        /* gridDim.y is capped: the rows in slabs of SR_GRID_CAP blocks */
        const long long slab = (long long)SR_GRID_CAP * SRQ_TALLY_ROWS;
        for (long long e = 0; e < rows; e += slab) {
          const long long nrow = slab < rows - e ? slab : rows - e;
          hipLaunchKernelGGL(sr_ppc_site_kernel,
                             dim3((unsigned)((N + SRQ_TALLY_THREADS - 1) / SRQ_TALLY_THREADS),
                                  (unsigned)((nrow + SRQ_TALLY_ROWS - 1) / SRQ_TALLY_ROWS)),
                             dim3(SRQ_TALLY_THREADS), 0, st, d_rich + (size_t)e * N, d_ro, nrow, N, d_s32, d_s32 + N,
                             d_s64);
          HIPCHK(hipGetLastError());
        }
      }
      hipLaunchKernelGGL(sr_ppc_total_kernel, dim3((unsigned)((rows + SRQ_TALLY_THREADS - 1) / SRQ_TALLY_THREADS)),
                         dim3(SRQ_TALLY_THREADS), 0, st, d_tot, ns, reps, d_t5, d_t5 + (size_t)ns * 5, d_g, d_g + 5);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(e1, st));
      HIPCHK(hipStreamSynchronize(st));   /* the next batch overwrites the tables and the scratch */
      float t = 0.0f;
      HIPCHK(hipEventElapsedTime(&t, e0, e1));
      total_ms += t;
      if (total_obs)
        HIPCHK(hipMemcpy(total_obs + (size_t)t0 * 5, d_t5, sizeof(long long) * ns * 5, hipMemcpyDeviceToHost));
      if (total_rep)
        HIPCHK(hipMemcpy(total_rep + (size_t)t0 * reps * 5, d_t5 + (size_t)ns * 5, sizeof(long long) * rows * 5,
                         hipMemcpyDeviceToHost));
    }
    if (ms) *ms = total_ms;
    if (taxon_gt) HIPCHK(hipMemcpy(taxon_gt, d_t32, sizeof(unsigned) * 5 * M, hipMemcpyDeviceToHost));
    if (taxon_eq) HIPCHK(hipMemcpy(taxon_eq, d_t32 + (size_t)5 * M, sizeof(unsigned) * 5 * M, hipMemcpyDeviceToHost));
    for (int which = 0; which < 2; ++which) {
      long long *dst = which ? taxon_sum_rep : taxon_sum_obs;
      if (!dst) continue;
      HIPCHK(hipMemcpy(h64, d_t64 + (size_t)which * 4 * M, sizeof(u64) * 4 * M, hipMemcpyDeviceToHost));
      for (int m = 0; m < M; ++m) {   /* ones, span, f0, f1 -> ones, span, gaps, f0, f1 */
        dst[m] = h64[m];
        dst[(size_t)M + m] = h64[(size_t)M + m];
        dst[(size_t)2 * M + m] = h64[(size_t)M + m] - h64[m];
        dst[(size_t)3 * M + m] = h64[(size_t)2 * M + m];
        dst[(size_t)4 * M + m] = h64[(size_t)3 * M + m];
      }
    }
    if (site_gt) HIPCHK(hipMemcpy(site_gt, d_s32, sizeof(unsigned) * N, hipMemcpyDeviceToHost));
    if (site_eq) HIPCHK(hipMemcpy(site_eq, d_s32 + N, sizeof(unsigned) * N, hipMemcpyDeviceToHost));
    if (site_sum_rep) HIPCHK(hipMemcpy(site_sum_rep, d_s64, sizeof(u64) * N, hipMemcpyDeviceToHost));
    long long g[10];
    HIPCHK(hipMemcpy(g, d_g, sizeof g, hipMemcpyDeviceToHost));
    memcpy(total_gt, g, sizeof(long long) * 5);
    memcpy(total_eq, g + 5, sizeof(long long) * 5);
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  free(h_xq); free(h_ro); free(h64);
  if (d_xq) (void)hipFree(d_xq);
  if (d_ro) (void)hipFree(d_ro);
  if (d_cd) (void)hipFree(d_cd);
  if (d_thr) (void)hipFree(d_thr);
  if (d_tot) (void)hipFree(d_tot);
  if (d_t5) (void)hipFree(d_t5);
  if (d_rich) (void)hipFree(d_rich);
  if (d_t32) (void)hipFree(d_t32);
  if (d_t64) (void)hipFree(d_t64);
  if (d_s32) (void)hipFree(d_s32);
  if (d_s64) (void)hipFree(d_s64);
  if (d_g) (void)hipFree(d_g);
  return rc;
}
