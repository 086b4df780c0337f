/*
 * sr_loo.hip -- PSIS-LOO cross-validation and the Pareto shape per cell over the saved records (no counterpart in
 * the reference: an extension, definitions in include/seriation.h "PSIS-LOO").
 *
 * As in sr_waic.hip a cell's term in one sample is one of four numbers that depend only on the sample's (the
 * taxon's) error rates, here the likelihood p and the importance ratio r = 1.0 / p.  Four kernels:
 *
 * Table kernel: sr_waic.hip's, extended: [sample][8][Mt], p[4] then r[4], Mt = 1 (shared rates) or M.
 *
 * Sum pass: sr_waic_pass_kernel<1>'s tiling and staging (a workgroup of 16 waves owns 64 taxa x 16 sites of one
 * chain, lanes along taxa, CH samples staged in LDS per chunk), accumulating Sp and Sr into per-chain partials in
 * HBM; the combine kernel adds them in chain order.  The order of the adds is the interface's and does not depend
 * on the batching of chains and rows.
 *
 * Selection pass: every cell keeps its K = n + 1 largest ratios.  One thread per cell, the same tile and staging, but
 * a workgroup walks every chain of a group (the selection is a multiset: no order to respect, no partials to
 * combine).  A cell's binary min-heap lives in HBM scratch, [slot][cell of the batch] so that the lanes of a wave
 * touch neighbouring words when they touch the same slot; its root is cached in a register and a sample is pushed
 * only when it beats the root (strictly: an equal value would replace an equal value).  The heap starts as K zeros
 * (every ratio is >= 1.0), so the first K samples are ordinary pushes.  Cells are taken in batches of whole tiles
 * whose heaps fit SR_LOO_SCRATCH; each batch re-reads the rows, in row batches whose table fits as much.
 *
 * Finish kernel: one thread per cell sorts its heap in place (heapsort on the min-heap: descending, so the tail
 * ascending is read with a negative stride) and calls sr_psis_tail (sr_psis.h), the source the host's sr_loo_tail
 * runs; it also forms lppd = log(Sp / T).
 *
 * The rows are addressed through a record view (sr_records.h); srl_loo is the unit's one entry point.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_records.h"
#include "sr_analysis.h"
#include "sr_math.h"
#include "sr_psis.h"

#define SRL_TILE 64                      /* taxa per workgroup: one per lane */
#define SRL_S 16                         /* sites per workgroup: one per wave */
#define SRL_THREADS (64 * SRL_S)
#define SRL_CH_SHARED 32                 /* samples staged per chunk, shared rates */
#define SRL_CH_MANY 8                    /* per-taxon rates: 8 x 8 x 64 doubles = 32 KB */
#define SRL_TAB_THREADS 256
#define SRL_FIN_THREADS 64               /* the finish kernel: one wave per block, the fit is long and uneven */
#define SRL_SCRATCH_DEFAULT (256LL << 20)

static __constant__ uint64_t l_exp_tab[256] = SR_EXP_TAB_INIT;
static __constant__ double l_log_tab[256] = SR_LOG_TAB_INIT;

/* tab [ns][8][Mt] from cd: row s of chain g at cd + (g * nr + s) * cdw, c at [m], d at [Mt + m] */
__global__ __launch_bounds__(SRL_TAB_THREADS) void sr_loo_table_kernel(const double *cd, int cdw, int Mt, long long ns,
                                                                        double *tab)
{
  const long long i = (long long)blockIdx.x * SRL_TAB_THREADS + threadIdx.x;
  if (i >= ns * Mt) return;
  const long long s = i / Mt;
  const int m = (int)(i - s * Mt);
  sr_mtab tb;
  tb.exp_tab = l_exp_tab; tb.log_tab = l_log_tab;
  const double c = cd[s * cdw + m], d = cd[s * cdw + Mt + m];
  const double ec = sr_exp_m(c, &tb), ed = sr_exp_m(d, &tb);
  const double p0 = 1.0 - ec, p2 = 1.0 - ed;
  double *o = tab + (size_t)s * 8 * Mt + m;
  o[0] = p0;
  o[(size_t)Mt] = ed;
  o[(size_t)2 * Mt] = p2;
  o[(size_t)3 * Mt] = ec;
  o[(size_t)4 * Mt] = 1.0 / p0;
  o[(size_t)5 * Mt] = 1.0 / ed;
  o[(size_t)6 * Mt] = 1.0 / p2;
  o[(size_t)7 * Mt] = 1.0 / ec;
}

struct LooArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *X;              /* [N][M] */
  const double *tab;             /* [G][nr][8][Mt]: this batch's rows */
  double *acc0, *acc1;           /* sum pass: [G][N][M] per-chain partials of Sp and Sr */
  double *heap;                  /* selection pass: [K][hstride] */
  long long hstride;             /* cells (tile slots) of this batch */
  int N, M, k0, r0, nr;          /* chains from k0, rows [r0, r0 + nr) */
  int ng;                        /* selection pass: chains k0 .. k0 + ng */
  int gx, tile0, K;              /* selection pass: tiles along taxa, the batch's first tile, the heap's size */
};

/* sr_waic_pass_kernel<1> with r in l's place: chain k0 + blockIdx.z */
template <bool MANY>
__global__ __launch_bounds__(SRL_THREADS) void sr_loo_sum_kernel(LooArgs A)
{
  constexpr int CH = MANY ? SRL_CH_MANY : SRL_CH_SHARED, TW = MANY ? SRL_TILE : 1;
  __shared__ int sa[CH][SRL_TILE], sb[CH][SRL_TILE], spi[CH][SRL_S];
  __shared__ double st[CH][8][TW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N, M = A.M, Mt = MANY ? M : 1;
  const int m = blockIdx.x * SRL_TILE + lane, n0 = blockIdx.y * SRL_S, n = n0 + wave, g = blockIdx.z;
  const bool mok = m < M, ok = mok && n < N;
  const size_t cell = (size_t)g * N * M + (size_t)(ok ? n : 0) * M + (ok ? m : 0);
  const int x = ok ? A.X[(size_t)n * M + m] : 0;
  const int tl = MANY ? lane : 0;
  const int16_t *base = A.rec + A.chain_off[A.k0 + g] + (long long)A.r0 * A.row_stride;
  const double *tab = A.tab + (size_t)g * A.nr * 8 * Mt;
  double s0 = 0.0, s1 = 0.0;
  if (ok) {
    s0 = A.acc0[cell];
    s1 = A.acc1[cell];
  }
  for (int c0 = 0; c0 < A.nr; c0 += CH) {
    const int nch = min(CH, A.nr - c0);
    for (int s = wave; s < nch; s += SRL_S) {
      const int16_t *row = base + (long long)(c0 + s) * A.row_stride;
      sa[s][lane] = mok ? (int)row[m] : 0;
      sb[s][lane] = mok ? (int)row[M + m] : 0;
      if (lane < SRL_S) spi[s][lane] = n0 + lane < N ? (int)row[2 * M + n0 + lane] : 0;
      const double *tr = tab + (size_t)(c0 + s) * 8 * Mt;
      if (MANY) {
#pragma unroll
        for (int j = 0; j < 8; ++j) st[s][j][tl] = mok ? tr[(size_t)j * Mt + m] : 0.0;
      } else if (lane < 8) {
        st[s][lane][0] = tr[lane];
      }
    }
    __syncthreads();
    for (int s = 0; s < nch; ++s) {
      const int a = sa[s][lane], b = sb[s][lane], p = spi[s][wave];
      const bool alive = a <= p && p < b;
      const int idx = x ? (alive ? 2 : 3) : (alive ? 1 : 0);
      s0 += st[s][idx][tl];
      s1 += st[s][4 + idx][tl];
    }
    __syncthreads();
  }
  if (ok) {
    A.acc0[cell] = s0;
    A.acc1[cell] = s1;
  }
}

/* tot += part[0] + ... in chain order, one add after the other */
__global__ void sr_loo_combine_kernel(double *tot0, double *tot1, const double *part0, const double *part1, int G,
                                      size_t nm)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nm) return;
  double t0 = tot0[i], t1 = tot1[i];
  for (int g = 0; g < G; ++g) {
    t0 += part0[(size_t)g * nm + i];
    t1 += part1[(size_t)g * nm + i];
  }
  tot0[i] = t0;
  tot1[i] = t1;
}

/* v replaces the root of the min-heap h[0..K) (slots hs apart), v > h[0]; returns the new root */
__device__ __forceinline__ double srl_push(double *h, long long hs, int K, double v)
{
  int i = 0;
  double root = v;
  for (;;) {
    int c = 2 * i + 1;
    if (c >= K) break;
    double cv = h[(long long)c * hs];
    if (c + 1 < K) {
      const double c2 = h[(long long)(c + 1) * hs];
      if (c2 < cv) { cv = c2; c = c + 1; }
    }
    if (!(cv < v)) break;
    h[(long long)i * hs] = cv;
    if (i == 0) root = cv;
    i = c;
  }
  h[(long long)i * hs] = v;
  return root;
}

/* block b owns tile tile0 + b and the heap columns [b * SRL_THREADS, (b + 1) * SRL_THREADS) */
template <bool MANY>
__global__ __launch_bounds__(SRL_THREADS) void sr_loo_select_kernel(LooArgs A)
{
  constexpr int CH = MANY ? SRL_CH_MANY : SRL_CH_SHARED, TW = MANY ? SRL_TILE : 1;
  __shared__ int sa[CH][SRL_TILE], sb[CH][SRL_TILE], spi[CH][SRL_S];
  __shared__ double st[CH][4][TW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N, M = A.M, Mt = MANY ? M : 1, K = A.K;
  const int tile = A.tile0 + blockIdx.x;
  const int m = (tile % A.gx) * SRL_TILE + lane, n0 = (tile / A.gx) * SRL_S, n = n0 + wave;
  const bool mok = m < M, ok = mok && n < N;
  const int x = ok ? A.X[(size_t)n * M + m] : 0;
  const int tl = MANY ? lane : 0;
  const long long hs = A.hstride;
  double *h = A.heap + (long long)blockIdx.x * SRL_THREADS + threadIdx.x;
  double root = ok ? h[0] : 0.0;
  for (int g = 0; g < A.ng; ++g) {
    const int16_t *base = A.rec + A.chain_off[A.k0 + g] + (long long)A.r0 * A.row_stride;
    const double *tab = A.tab + (size_t)g * A.nr * 8 * Mt;
    for (int c0 = 0; c0 < A.nr; c0 += CH) {
      const int nch = min(CH, A.nr - c0);
      for (int s = wave; s < nch; s += SRL_S) {
        const int16_t *row = base + (long long)(c0 + s) * A.row_stride;
        sa[s][lane] = mok ? (int)row[m] : 0;
        sb[s][lane] = mok ? (int)row[M + m] : 0;
        if (lane < SRL_S) spi[s][lane] = n0 + lane < N ? (int)row[2 * M + n0 + lane] : 0;
        const double *tr = tab + (size_t)(c0 + s) * 8 * Mt + (size_t)4 * Mt;
        if (MANY) {
#pragma unroll
          for (int j = 0; j < 4; ++j) st[s][j][tl] = mok ? tr[(size_t)j * Mt + m] : 0.0;
        } else if (lane < 4) {
          st[s][lane][0] = tr[lane];
        }
      }
      __syncthreads();
      for (int s = 0; s < nch; ++s) {
        const int a = sa[s][lane], b = sb[s][lane], p = spi[s][wave];
        const bool alive = a <= p && p < b;
        const int idx = x ? (alive ? 2 : 3) : (alive ? 1 : 0);
        const double v = st[s][idx][tl];
        if (ok && v > root) root = srl_push(h, hs, K, v);
      }
      __syncthreads();
    }
  }
}

struct FinArgs {
  double *heap;                  /* [K][hstride], NULL when the tail is not fitted (n < 5) */
  long long hstride;
  const double *sp, *sr;         /* [N][M] */
  const double *G, *L;           /* [m], [n] */
  double *lppd, *elpd, *pk;      /* [N][M] */
  long long T;
  int N, M, gx, tile0, ntiles, n, m;
};

__global__ __launch_bounds__(SRL_FIN_THREADS) void sr_loo_finish_kernel(FinArgs A)
{
  const long long col = (long long)blockIdx.x * SRL_FIN_THREADS + threadIdx.x;   /* the batch's tile slot */
  if (col >= (long long)A.ntiles * SRL_THREADS) return;
  const int tile = A.tile0 + (int)(col / SRL_THREADS), t = (int)(col % SRL_THREADS);
  const int mm = (tile % A.gx) * SRL_TILE + (t & 63), nn = (tile / A.gx) * SRL_S + (t >> 6);
  if (mm >= A.M || nn >= A.N) return;
  const size_t cell = (size_t)nn * A.M + mm;
  sr_mtab tb;
  tb.exp_tab = l_exp_tab; tb.log_tab = l_log_tab;
  const double Sr = A.sr[cell];
  A.lppd[cell] = sr_log_m(A.sp[cell] / (double)A.T, &tb);
  double k, e;
  if (!A.heap) {
    sr_psis_tail(nullptr, 0, 0, 0.0, Sr, A.T, A.G, A.m, A.L, &tb, &k, &e);
  } else {
    const long long hs = A.hstride;
    double *h = A.heap + col;
    const int n = A.n;
    /* heapsort: the minimum goes to the end of the shrinking heap, h[0] >= h[1] >= ... >= h[n] afterwards */
    for (int last = n; last > 0; --last) {
      const double v = h[(long long)last * hs];
      h[(long long)last * hs] = h[0];
      int i = 0;
      for (;;) {
        int c = 2 * i + 1;
        if (c >= last) break;
        double cv = h[(long long)c * hs];
        if (c + 1 < last) {
          const double c2 = h[(long long)(c + 1) * hs];
          if (c2 < cv) { cv = c2; c = c + 1; }
        }
        if (!(cv < v)) break;
        h[(long long)i * hs] = cv;
        i = c;
      }
      h[(long long)i * hs] = v;
    }
    sr_psis_tail(h + (long long)(n - 1) * hs, (ptrdiff_t)-hs, n, h[(long long)n * hs], Sr, A.T, A.G, A.m, A.L, &tb,
                 &k, &e);
  }
  A.pk[cell] = k;
  A.elpd[cell] = e;
}

static long long srl_scratch(void)
{
  const char *e = getenv("SR_LOO_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? v : SRL_SCRATCH_DEFAULT;
}

/* PSIS-LOO's pointwise terms of the n_sel chains of a record view.  X [N][M], cd [n_sel] (as srw_waic takes them,
   already checked) and the tables G [m], L [n] (n the tail length of T = n_sel * count, at most SR_PSIS_NMAX; not
   read when n < 5) are host inputs; lppd, elpd, pareto_k [N][M] are host buffers; ms3 (optional) receives the
   kernels' time of the sum, selection and finish phases. */
extern "C" int srl_loo(const sr_recview *v, int N, int M, const uint8_t *X, const double *const *cd, int cdw,
                       int manycd, int n, int m, const double *G, const double *L, double *lppd, double *elpd,
                       double *pareto_k, float *ms3)
{
  int rc = 0;
  uint8_t *d_X = nullptr;
  double *d_cd = nullptr, *d_tab = nullptr, *d_part = nullptr, *d_tot = nullptr, *d_heap = nullptr, *d_GL = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || !X || !cd || !lppd || !elpd || !pareto_k || n_sel <= 0 || count < 1 || N < 1 ||
      N > 32767 || M < 1 || (long long)n_sel * count >= (1LL << 31) || (long long)N * M > (1LL << 27) || n < 0 ||
      n > SR_PSIS_NMAX || (long long)n >= (long long)n_sel * count + (n == 0) || m < 0 || m > SR_PSIS_MMAX ||
      (n >= 5 && (!G || !L || m < 1)))
    return -1;
  if (ms3) ms3[0] = ms3[1] = ms3[2] = 0.0f;
  const bool fit = n >= 5;
  const size_t nm = (size_t)N * M;
  const int Mt = manycd ? M : 1;
  const long long T = (long long)n_sel * count;
  const long long scratch = srl_scratch();
  /* sum phase: chains per group (two partial planes of doubles) and rows per batch (the table, the c, d rows) */
  long long G1 = scratch / (long long)(nm * 2 * sizeof(double));
  if (G1 > n_sel) G1 = n_sel;
  if (G1 > SR_GRID_CAP) G1 = SR_GRID_CAP;
  if (G1 < 1) G1 = 1;
  long long RB1 = scratch / (G1 * (long long)Mt * 8 * (long long)sizeof(double));
  if (RB1 > count) RB1 = count;
  if (RB1 < 1) RB1 = 1;
  /* selection phase: tiles per batch (K heap slots per tile slot); one chain's rows per table batch */
  const int gx = (M + SRL_TILE - 1) / SRL_TILE, gy = (N + SRL_S - 1) / SRL_S;
  const long long tiles = (long long)gx * gy;
  const int K = n + 1;
  long long TB = scratch / ((long long)SRL_THREADS * K * (long long)sizeof(double));
  if (TB > tiles) TB = tiles;
  if (TB < 1) TB = 1;
  long long RB2 = scratch / ((long long)Mt * 8 * (long long)sizeof(double));
  if (RB2 > count) RB2 = count;
  if (RB2 < 1) RB2 = 1;
  long long G2 = RB2 == count ? scratch / ((long long)count * Mt * 8 * (long long)sizeof(double)) : 1;
  if (G2 > n_sel) G2 = n_sel;
  if (G2 < 1) G2 = 1;
  const long long RBmax = G1 * RB1 > G2 * RB2 ? G1 * RB1 : G2 * RB2;
  const unsigned nmb = (unsigned)((nm + 255) / 256);
  float ms_sum = 0.0f, ms_sel = 0.0f, ms_fin = 0.0f, t = 0.0f;
  {
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMalloc(&d_X, nm));
    HIPCHK(hipMemcpy(d_X, X, nm, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&d_cd, sizeof(double) * RBmax * cdw));
    HIPCHK(hipMalloc(&d_tab, sizeof(double) * RBmax * 8 * Mt));
    HIPCHK(hipMalloc(&d_part, sizeof(double) * G1 * 2 * nm));
    HIPCHK(hipMalloc(&d_tot, sizeof(double) * 5 * nm));   /* Sp, Sr, lppd, elpd, k */
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipMemsetAsync(d_tot, 0, sizeof(double) * 2 * nm, st));
    LooArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride; A.X = d_X; A.tab = d_tab;
    A.N = N; A.M = M; A.heap = nullptr; A.hstride = 0; A.ng = 0; A.gx = gx; A.tile0 = 0; A.K = K;
    A.acc0 = d_part;
    A.acc1 = d_part + (size_t)G1 * nm;
    for (int k0 = 0; k0 < n_sel; k0 += (int)G1) {
      const int ng = (int)(G1 < n_sel - k0 ? G1 : n_sel - k0);
      HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * G1 * 2 * nm, st));
      for (int r0 = 0; r0 < count; r0 += (int)RB1) {
        const int nr = (int)(RB1 < count - r0 ? RB1 : count - r0);
        for (int g = 0; g < ng; ++g)
          HIPCHK(hipMemcpyAsync(d_cd + (size_t)g * nr * cdw, cd[k0 + g] + (size_t)r0 * cdw, sizeof(double) * nr * cdw,
                                hipMemcpyHostToDevice, st));
        const long long ns = (long long)ng * nr;
        HIPCHK(hipEventRecord(e0, st));
        hipLaunchKernelGGL(sr_loo_table_kernel, dim3((unsigned)((ns * Mt + SRL_TAB_THREADS - 1) / SRL_TAB_THREADS)),
                           dim3(SRL_TAB_THREADS), 0, st, d_cd, cdw, Mt, ns, d_tab);
        HIPCHK(hipGetLastError());
        A.k0 = k0; A.r0 = r0; A.nr = nr;
        const dim3 gr(gx, gy, ng);
        if (manycd) hipLaunchKernelGGL((sr_loo_sum_kernel<true>), gr, dim3(SRL_THREADS), 0, st, A);
        else hipLaunchKernelGGL((sr_loo_sum_kernel<false>), gr, dim3(SRL_THREADS), 0, st, A);
        HIPCHK(hipGetLastError());
        if (r0 + nr == count) {
          hipLaunchKernelGGL(sr_loo_combine_kernel, dim3(nmb), dim3(256), 0, st, d_tot, d_tot + nm, d_part,
                             d_part + (size_t)G1 * nm, ng, nm);
          HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipStreamSynchronize(st));   /* the next batch overwrites d_cd and d_tab */
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        ms_sum += t;
      }
    }
    FinArgs F;
    F.heap = nullptr; F.hstride = 0; F.sp = d_tot; F.sr = d_tot + nm; F.G = nullptr; F.L = nullptr;
    F.lppd = d_tot + 2 * nm; F.elpd = d_tot + 3 * nm; F.pk = d_tot + 4 * nm;
    F.T = T; F.N = N; F.M = M; F.gx = gx; F.n = n; F.m = m;
    if (fit) {
      HIPCHK(hipMalloc(&d_heap, sizeof(double) * (size_t)K * TB * SRL_THREADS));
      HIPCHK(hipMalloc(&d_GL, sizeof(double) * ((size_t)m + n)));
      HIPCHK(hipMemcpyAsync(d_GL, G, sizeof(double) * m, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_GL + m, L, sizeof(double) * n, hipMemcpyHostToDevice, st));
      F.G = d_GL; F.L = d_GL + m;
    }
    for (long long t0 = 0; t0 < tiles; t0 += TB) {
      const int nt = (int)(TB < tiles - t0 ? TB : tiles - t0);
      if (fit) {
        const long long hs = (long long)nt * SRL_THREADS;
        HIPCHK(hipMemsetAsync(d_heap, 0, sizeof(double) * (size_t)K * hs, st));
        A.heap = d_heap; A.hstride = hs; A.tile0 = (int)t0;
        for (int k0 = 0; k0 < n_sel; k0 += (int)G2)
          for (int r0 = 0; r0 < count; r0 += (int)RB2) {
            const int ng = (int)(G2 < n_sel - k0 ? G2 : n_sel - k0);
            const int nr = (int)(RB2 < count - r0 ? RB2 : count - r0);
            for (int g = 0; g < ng; ++g)
              HIPCHK(hipMemcpyAsync(d_cd + (size_t)g * nr * cdw, cd[k0 + g] + (size_t)r0 * cdw,
                                    sizeof(double) * nr * cdw, hipMemcpyHostToDevice, st));
            const long long ns = (long long)ng * nr;
            HIPCHK(hipEventRecord(e0, st));
            hipLaunchKernelGGL(sr_loo_table_kernel,
                               dim3((unsigned)((ns * Mt + SRL_TAB_THREADS - 1) / SRL_TAB_THREADS)),
                               dim3(SRL_TAB_THREADS), 0, st, d_cd, cdw, Mt, ns, d_tab);
            HIPCHK(hipGetLastError());
            A.k0 = k0; A.r0 = r0; A.nr = nr; A.ng = ng;
            if (manycd) hipLaunchKernelGGL((sr_loo_select_kernel<true>), dim3(nt), dim3(SRL_THREADS), 0, st, A);
            else hipLaunchKernelGGL((sr_loo_select_kernel<false>), dim3(nt), dim3(SRL_THREADS), 0, st, A);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(e1, st));
            HIPCHK(hipStreamSynchronize(st));   /* the next batch overwrites d_cd and d_tab */
            HIPCHK(hipEventElapsedTime(&t, e0, e1));
            ms_sel += t;
          }
        F.heap = d_heap; F.hstride = hs;
      }
      F.tile0 = (int)t0; F.ntiles = nt;
      HIPCHK(hipEventRecord(e0, st));
      hipLaunchKernelGGL(sr_loo_finish_kernel, dim3((unsigned)(nt * (SRL_THREADS / SRL_FIN_THREADS))),
                         dim3(SRL_FIN_THREADS), 0, st, F);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(e1, st));
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipEventElapsedTime(&t, e0, e1));
      ms_fin += t;
    }
    if (ms3) { ms3[0] = ms_sum; ms3[1] = ms_sel; ms3[2] = ms_fin; }
    HIPCHK(hipMemcpy(lppd, d_tot + 2 * nm, sizeof(double) * nm, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(elpd, d_tot + 3 * nm, sizeof(double) * nm, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pareto_k, d_tot + 4 * nm, sizeof(double) * nm, hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_X) (void)hipFree(d_X);
  if (d_cd) (void)hipFree(d_cd);
  if (d_tab) (void)hipFree(d_tab);
  if (d_part) (void)hipFree(d_part);
  if (d_tot) (void)hipFree(d_tot);
  if (d_heap) (void)hipFree(d_heap);
  if (d_GL) (void)hipFree(d_GL);
  return rc;
}
