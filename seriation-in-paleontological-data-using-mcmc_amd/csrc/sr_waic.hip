/*
 * sr_waic.hip -- WAIC and the pointwise model fit over the saved records (no counterpart in the reference: an
 * extension, definitions in include/seriation.h "WAIC").
 *
 * The likelihood factorises over the N M cells of X, and for one sample a cell's term is one of four numbers that
 * depend only on the sample's (the taxon's) error rates.  So the work is a table of T (T M with per-taxon rates)
 * rows of eight doubles -- p[4] then l[4] -- and an N M T reduction in f64 that picks one p and one l per cell and
 * sample.  The order of the adds is part of the interface (rows ascending within a chain from +0.0, then chains
 * ascending from +0.0); there is no fma (-ffp-contract=off) and no floating-point atomic.
 *
 * Table kernel: one thread per sample and taxon evaluates sr_exp_m / sr_log_m (the tables in constant memory) on
 * the c, d rows copied from the host and writes [sample][8][Mt], Mt = 1 (shared rates) or M, so that the eight
 * entries of a tile's 64 taxa are eight runs of 64 contiguous doubles.
 *
 * Pass kernel: one thread per cell, lanes along taxa.  A workgroup of 16 waves owns 64 taxa x SRW_S = 16 sites of
 * one chain: a_m, b_m, X and the per-taxon table rows are per-lane reads, pi_n and the shared-rates row are
 * wave-uniform.  For a chunk of CH samples (32 with shared rates, 8 with per-taxon rates, whose table rows take
 * 4 KB of LDS each) it stages the tile's limits, its 16 site positions and the table rows in LDS -- the SRR_CH
 * pattern of sr_rel.hip -- so each record row and each table row is read once per workgroup and serves 16 sites.
 * The inner loop reads a, b, the broadcast pi, forms alive and the index, and adds the indexed LDS entries
 * ([chunk row][entry][lane]: consecutive lanes on consecutive banks whatever the index).  The accumulators are
 * loaded from and stored to per-chain partial sums in HBM, so a launch can cover any run of rows: the host loop
 * batches chains (partials of at most SR_WAIC_SCRATCH bytes, 256 MiB unless the environment says otherwise) and
 * rows (table of at most as much) and the order of the adds does not depend on the batching.  The first pass sums
 * p and l; the combine kernel adds a group's partials to the totals in chain order; the finish kernel forms
 * lppd = log(Sp / T) and mu = Sl / T; the second pass, the same kernel, sums (l - mu)^2 and stages only l[4].
 *
 * The rows are addressed through a record view (sr_records.h: chain k's rows start at rec + chain_off[k], row_stride
 * apart); srw_waic is the unit's one entry point.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_records.h"
#include "sr_analysis.h"
#include "sr_math.h"

#define SRW_TILE 64                      /* taxa per workgroup: one per lane */
#define SRW_S 16                         /* sites per workgroup: one per wave */
#define SRW_THREADS (64 * SRW_S)
#define SRW_CH_SHARED 32                 /* samples staged per chunk, shared rates */
#define SRW_CH_MANY 8                    /* per-taxon rates: 8 x 8 x 64 doubles = 32 KB */
#define SRW_TAB_THREADS 256
#define SRW_SCRATCH_DEFAULT (256LL << 20)

__constant__ uint64_t w_exp_tab[256] = SR_EXP_TAB_INIT;
__constant__ double w_log_tab[256] = SR_LOG_TAB_INIT;

/* tab [ns][8][Mt] from cd: row s of chain g at cd + (g * nr + s) * cdw, c at [m], d at [Mt + m] */
__global__ __launch_bounds__(SRW_TAB_THREADS) void sr_waic_table_kernel(const double *cd, int cdw, int Mt,
                                                                         long long ns, double *tab)
{
  const long long i = (long long)blockIdx.x * SRW_TAB_THREADS + threadIdx.x;
  if (i >= ns * Mt) return;
  const long long s = i / Mt;
  const int m = (int)(i - s * Mt);
  sr_mtab tb;
  tb.exp_tab = w_exp_tab; tb.log_tab = w_log_tab;
  const double c = cd[s * cdw + m], d = cd[s * cdw + Mt + m];
  const double ec = sr_exp_m(c, &tb), ed = sr_exp_m(d, &tb);
  double *o = tab + (size_t)s * 8 * Mt + m;
  o[0] = 1.0 - ec;
  o[(size_t)Mt] = ed;
  o[(size_t)2 * Mt] = 1.0 - ed;
  o[(size_t)3 * Mt] = ec;
  o[(size_t)4 * Mt] = sr_log_m(1.0 - ec, &tb);
  o[(size_t)5 * Mt] = d;
  o[(size_t)6 * Mt] = sr_log_m(1.0 - ed, &tb);
  o[(size_t)7 * Mt] = c;
}

struct WaicArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *X;              /* [N][M] */
  const double *tab;             /* [G][nr][8][Mt]: this batch's rows */
  const double *mu;              /* [N][M], second pass */
  double *acc0, *acc1;           /* [G][N][M] per-chain partials: Sp and Sl, or V (acc1 unused) */
  int N, M, k0, r0, nr;          /* chains k0 + blockIdx.z, rows [r0, r0 + nr) */
};

template <int PASS, bool MANY>
__global__ __launch_bounds__(SRW_THREADS) void sr_waic_pass_kernel(WaicArgs A)
{
  constexpr int CH = MANY ? SRW_CH_MANY : SRW_CH_SHARED, TW = MANY ? SRW_TILE : 1;
  constexpr int J0 = PASS == 1 ? 0 : 4;   /* the second pass reads l[4] only */
  __shared__ int sa[CH][SRW_TILE], sb[CH][SRW_TILE], spi[CH][SRW_S];
  __shared__ double st[CH][8][TW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = A.N, M = A.M, Mt = MANY ? M : 1;
  const int m = blockIdx.x * SRW_TILE + lane, n0 = blockIdx.y * SRW_S, n = n0 + wave, g = blockIdx.z;
  const bool mok = m < M, ok = mok && n < N;
  const size_t cell = (size_t)g * N * M + (size_t)(ok ? n : 0) * M + (ok ? m : 0);
  const int x = ok ? A.X[(size_t)n * M + m] : 0;
  const int tl = MANY ? lane : 0;
  const int16_t *base = A.rec + A.chain_off[A.k0 + g] + (long long)A.r0 * A.row_stride;
  const double *tab = A.tab + (size_t)g * A.nr * 8 * Mt;
  double s0 = 0.0, s1 = 0.0, mu = 0.0;
  if (ok) {
    s0 = A.acc0[cell];
    if (PASS == 1) s1 = A.acc1[cell];
    else mu = A.mu[(size_t)n * M + m];
  }
  for (int c0 = 0; c0 < A.nr; c0 += CH) {
    const int nch = min(CH, A.nr - c0);
    for (int s = wave; s < nch; s += SRW_S) {
      const int16_t *row = base + (long long)(c0 + s) * A.row_stride;
      sa[s][lane] = mok ? (int)row[m] : 0;
      sb[s][lane] = mok ? (int)row[M + m] : 0;
      if (lane < SRW_S) spi[s][lane] = n0 + lane < N ? (int)row[2 * M + n0 + lane] : 0;
      const double *tr = tab + (size_t)(c0 + s) * 8 * Mt;
      if (MANY) {
#pragma unroll
        for (int j = J0; j < 8; ++j) st[s][j][tl] = mok ? tr[(size_t)j * Mt + m] : 0.0;
      } else if (lane >= J0 && lane < 8) {
        st[s][lane][0] = tr[lane];
      }
    }
    __syncthreads();
    for (int s = 0; s < nch; ++s) {
      const int a = sa[s][lane], b = sb[s][lane], p = spi[s][wave];
      const bool alive = a <= p && p < b;
      const int idx = x ? (alive ? 2 : 3) : (alive ? 1 : 0);
      if (PASS == 1) {
        s0 += st[s][idx][tl];
        s1 += st[s][4 + idx][tl];
      } else {
        const double dl = st[s][4 + idx][tl] - mu;
        s0 += dl * dl;
      }
    }
    __syncthreads();
  }
  if (ok) {
    A.acc0[cell] = s0;
    if (PASS == 1) A.acc1[cell] = s1;
  }
}

/* tot += part[0] + ... in chain order, one add after the other */
__global__ void sr_waic_combine_kernel(double *tot0, double *tot1, const double *part0, const double *part1, int G,
                                       size_t nm)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nm) return;
  double t0 = tot0[i], t1 = tot1 ? tot1[i] : 0.0;
  for (int g = 0; g < G; ++g) {
    t0 += part0[(size_t)g * nm + i];
    if (tot1) t1 += part1[(size_t)g * nm + i];
  }
  tot0[i] = t0;
  if (tot1) tot1[i] = t1;
}

/* which 1: sp -> lppd = log(sp / T), sl -> mu = sl / T; which 2: v -> pwaic = v / (T - 1) */
__global__ void sr_waic_finish_kernel(double *v0, double *v1, int which, double T, size_t nm)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nm) return;
  if (which == 1) {
    sr_mtab tb;
    tb.exp_tab = w_exp_tab; tb.log_tab = w_log_tab;
    v0[i] = sr_log_m(v0[i] / T, &tb);
    v1[i] = v1[i] / T;
  } else {
    v0[i] = v0[i] / (T - 1.0);
  }
}

static long long srw_scratch(void)
{
  const char *e = getenv("SR_WAIC_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? v : SRW_SCRATCH_DEFAULT;
}

/* WAIC's pointwise terms of the n_sel chains of a record view.  X [N][M] and cd [n_sel] (each chain's
   [count][cdw] rows: c at [m], d at [Mt + m], Mt = M when manycd, else 1) are host inputs, already checked;
   lppd, ll_mean (may be NULL), pwaic [N][M] are host buffers. */
extern "C" int srw_waic(const sr_recview *v, int N, int M, const uint8_t *X, const double *const *cd, int cdw,
                        int manycd, double *lppd, double *ll_mean, double *pwaic, float *ms)
{
  int rc = 0;
  uint8_t *d_X = nullptr;
  double *d_cd = nullptr, *d_tab = nullptr, *d_part = nullptr, *d_tot = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || !X || !cd || !lppd || !pwaic || n_sel <= 0 || count < 1 || N < 1 || N > 32767 ||
      M < 1 || (long long)n_sel * count >= (1LL << 31) || (long long)n_sel * count < 2 ||
      (long long)N * M > (1LL << 27))
    return -1;
  if (ms) *ms = 0.0f;
  const size_t nm = (size_t)N * M;
  const int Mt = manycd ? M : 1;
  const double T = (double)((long long)n_sel * count);
  const long long scratch = srw_scratch();
  /* chains per group: two partial planes of doubles; rows per batch: the table and the c, d rows */
  long long G = scratch / (long long)(nm * 2 * sizeof(double));
  if (G > n_sel) G = n_sel;
  if (G > 65535) G = 65535;
  if (G < 1) G = 1;
  long long RB = scratch / (G * (long long)Mt * 8 * (long long)sizeof(double));
  if (RB > count) RB = count;
  if (RB < 1) RB = 1;
  const dim3 grid((M + SRW_TILE - 1) / SRW_TILE, (N + SRW_S - 1) / SRW_S, 1);
  const unsigned nmb = (unsigned)((nm + 255) / 256);
  float total_ms = 0.0f;
  {
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMalloc(&d_X, nm));
    HIPCHK(hipMemcpy(d_X, X, nm, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&d_cd, sizeof(double) * G * RB * cdw));
    HIPCHK(hipMalloc(&d_tab, sizeof(double) * G * RB * 8 * Mt));
    HIPCHK(hipMalloc(&d_part, sizeof(double) * G * 2 * nm));
    HIPCHK(hipMalloc(&d_tot, sizeof(double) * 3 * nm));   /* Sp -> lppd, Sl -> mu, V -> pwaic */
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipMemsetAsync(d_tot, 0, sizeof(double) * 3 * nm, st));
    WaicArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride; A.X = d_X; A.tab = d_tab;
    A.mu = d_tot + nm; A.N = N; A.M = M;
    for (int pass = 1; pass <= 2; ++pass) {
      A.acc0 = d_part;
      A.acc1 = pass == 1 ? d_part + (size_t)G * nm : nullptr;
      for (int k0 = 0; k0 < n_sel; k0 += (int)G) {
        const int ng = (int)(G < n_sel - k0 ? G : n_sel - k0);
        HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * G * 2 * nm, st));
        for (int r0 = 0; r0 < count; r0 += (int)RB) {
          const int nr = (int)(RB < count - r0 ? RB : count - r0);
          for (int g = 0; g < ng; ++g)
            HIPCHK(hipMemcpyAsync(d_cd + (size_t)g * nr * cdw, cd[k0 + g] + (size_t)r0 * cdw,
                                  sizeof(double) * nr * cdw, hipMemcpyHostToDevice, st));
          const long long ns = (long long)ng * nr;
          HIPCHK(hipEventRecord(e0, st));
          hipLaunchKernelGGL(sr_waic_table_kernel, dim3((unsigned)((ns * Mt + SRW_TAB_THREADS - 1) / SRW_TAB_THREADS)),
                             dim3(SRW_TAB_THREADS), 0, st, d_cd, cdw, Mt, ns, d_tab);
          HIPCHK(hipGetLastError());
          A.k0 = k0; A.r0 = r0; A.nr = nr;
          const dim3 gr(grid.x, grid.y, ng);
          if (pass == 1 && manycd) hipLaunchKernelGGL((sr_waic_pass_kernel<1, true>), gr, dim3(SRW_THREADS), 0, st, A);
          else if (pass == 1) hipLaunchKernelGGL((sr_waic_pass_kernel<1, false>), gr, dim3(SRW_THREADS), 0, st, A);
          else if (manycd) hipLaunchKernelGGL((sr_waic_pass_kernel<2, true>), gr, dim3(SRW_THREADS), 0, st, A);
          else hipLaunchKernelGGL((sr_waic_pass_kernel<2, false>), gr, dim3(SRW_THREADS), 0, st, A);
          HIPCHK(hipGetLastError());
          if (r0 + nr == count) {
            if (pass == 1)
              hipLaunchKernelGGL(sr_waic_combine_kernel, dim3(nmb), dim3(256), 0, st, d_tot, d_tot + nm, d_part,
                                 d_part + (size_t)G * nm, ng, nm);
            else
              hipLaunchKernelGGL(sr_waic_combine_kernel, dim3(nmb), dim3(256), 0, st, d_tot + 2 * nm,
                                 (double *)nullptr, d_part, (const double *)nullptr, ng, nm);
            HIPCHK(hipGetLastError());
            if (k0 + ng == n_sel) {
              if (pass == 1)
                hipLaunchKernelGGL(sr_waic_finish_kernel, dim3(nmb), dim3(256), 0, st, d_tot, d_tot + nm, 1, T, nm);
              else
                hipLaunchKernelGGL(sr_waic_finish_kernel, dim3(nmb), dim3(256), 0, st, d_tot + 2 * nm,
                                   (double *)nullptr, 2, T, nm);
              HIPCHK(hipGetLastError());
            }
          }
          HIPCHK(hipEventRecord(e1, st));
          HIPCHK(hipStreamSynchronize(st));   /* the next batch overwrites d_cd and d_tab */
          float t = 0.0f;
          HIPCHK(hipEventElapsedTime(&t, e0, e1));
          total_ms += t;
        }
      }
    }
    if (ms) *ms = total_ms;
    HIPCHK(hipMemcpy(lppd, d_tot, sizeof(double) * nm, hipMemcpyDeviceToHost));
    if (ll_mean) HIPCHK(hipMemcpy(ll_mean, d_tot + nm, sizeof(double) * nm, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pwaic, d_tot + 2 * nm, sizeof(double) * nm, hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_X) (void)hipFree(d_X);
  if (d_cd) (void)hipFree(d_cd);
  if (d_tab) (void)hipFree(d_tab);
  if (d_part) (void)hipFree(d_part);
  if (d_tot) (void)hipFree(d_tot);
  return rc;
}
