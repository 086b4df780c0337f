/*
 * sr_place.hip -- posterior placement of query rows in the seriation, over the saved records (no counterpart in the
 * reference: an extension, definitions in include/seriation.h "Placement").
 *
 * A query row y [M] (0 absent, 1 present, 2 not assessed) at candidate position p has, under one sample, the log
 * likelihood L[p] = sum over taxa of one of WAIC's four l terms, picked by (y_m, a_m <= p < b_m).  Normalised over
 * the positions it is the sample's placement w[p]; averaged over the samples it is pos[q][p], and read at the sites'
 * own positions, site[q][n].  The order of every add is part of the interface: L over taxa ascending, Z over 64
 * strided columns and then over the columns, the sums over samples rows ascending within a chain from +0.0 and then
 * chains ascending from +0.0; no fma outside sr_exp_m / sr_log_m (-ffp-contract=off) and no floating-point atomic.
 *
 * Table kernel: one thread per sample and taxon, l[4] = {log(1 - exp(c)), d, log(1 - exp(d)), c} as [sample][4][Mt],
 * Mt = 1 (shared rates) or M.
 *
 * Profile kernel, the N M T Q part: lanes along positions, a workgroup owns one sample, a tile of SRX_QT queries and
 * a tile of up to 256 positions.  For a chunk of SRX_MC taxa it stages a, b (int32, reflected when the chain is
 * flagged) and, per taxon and query of the tile, the two candidate terms as one double2 -- .x the term when alive
 * (y ? l[2] : l[1]), .y when not (y ? l[3] : l[0]), both +0.0 for y = 2 and for the tile's queries beyond Q -- in
 * LDS.  The inner loop reads a, b and the pair from one address for the whole wave (a broadcast), forms alive from
 * the lane's own p and adds the selected term to the query's accumulator: SRX_QT accumulators per thread, a and b
 * read once for the whole tile, no lane-dependent LDS address.  L goes to the slab [batch sample][Q][N].
 *
 * Normalise kernel: one wave per (sample, query).  Lane j walks p = j, j + 64, ...: first the maximum (exact in any
 * order: no NaN, no -0.0), then e = exp(L - mx) written over L and added to the lane's z_j, which is the
 * definition's strided sum; the 64 z_j are read lane by lane and added in order to Z; lse = mx + log(Z); a third walk
 * overwrites e with w = e / Z (an IEEE division).  A lane reads back only what it wrote itself.
 *
 * Accumulate kernel (sr_waic_pass_kernel's pattern): one thread per (chain, query, p) and, in the site role, per
 * (chain, query, n), loads its per-chain partial from HBM, walks the batch's rows in order adding w[p] (the site
 * role: w at the site's own reflected position, +0.0 when that lies outside 0..N-1) and stores the partial back, so
 * a launch covers any run of rows and no N needs LDS accumulators.  The combine kernel adds a group's partials to
 * the totals in chain order; the finish kernel divides by T.
 *
 * The host loop batches chains (partials) and rows (the slab) so that each takes at most SR_PLACE_SCRATCH bytes
 * (256 MiB unless the environment says otherwise; one chain and one row at the least); the order of the adds does
 * not depend on the batching.  The rows are addressed through a record view (sr_records.h); srx_place is the unit's
 * one entry point.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sr_records.h"
#include "sr_analysis.h"
#include "sr_math.h"

#define SRX_QT 8                         /* queries per workgroup of the profile kernel */
#define SRX_MC 128                       /* taxa staged per chunk: 128 x 8 double2 = 16 KB, a and b 1 KB */
#define SRX_PT 256                       /* positions per workgroup at most: one per thread */
#define SRX_TAB_THREADS 256
#define SRX_NWAVES 4                     /* normalise kernel: (sample, query) pairs per workgroup, one per wave */
#define SRX_ACC_THREADS 256
#define SRX_SCRATCH_DEFAULT (256LL << 20)
#define SRX_GRID_X_MAX (1LL << 30)       /* blocks along gridDim.x that a launch takes at most */

__constant__ uint64_t x_exp_tab[256] = SR_EXP_TAB_INIT;
__constant__ double x_log_tab[256] = SR_LOG_TAB_INIT;

/* tab [ns][4][Mt] from cd: row s at cd + s * cdw, c at [m], d at [Mt + m] */
__global__ __launch_bounds__(SRX_TAB_THREADS) void sr_place_table_kernel(const double *cd, int cdw, int Mt,
                                                                          long long ns, double *tab)
{
  const long long i = (long long)blockIdx.x * SRX_TAB_THREADS + threadIdx.x;
  if (i >= ns * Mt) return;
  const long long s = i / Mt;
  const int m = (int)(i - s * Mt);
  sr_mtab tb;
  tb.exp_tab = x_exp_tab; tb.log_tab = x_log_tab;
  const double c = cd[s * cdw + m], d = cd[s * cdw + Mt + m];
  double *o = tab + (size_t)s * 4 * Mt + m;
  o[0] = sr_log_m(1.0 - sr_exp_m(c, &tb), &tb);
  o[(size_t)Mt] = d;
  o[(size_t)2 * Mt] = sr_log_m(1.0 - sr_exp_m(d, &tb), &tb);
  o[(size_t)3 * Mt] = c;
}

struct PlaceArgs {
  const int16_t *rec;
  const long long *chain_off;    /* [n_sel] element offset of each chain's first row */
  long long row_stride;
  const uint8_t *Y;              /* [Q][M] */
  const uint8_t *flip;           /* [n_sel] or NULL */
  const double *tab;             /* [ng][nr][4][Mt]: this batch's samples */
  double *slab;                  /* [ng][nr][Q][N]: L, then e, then w */
  double *lse;                   /* [ng][nr][Q] */
  double *part;                  /* [ng][Q][N] per-chain partials of the role at hand */
  int N, M, Q, k0, r0, nr, ng;   /* chains k0 .. k0 + ng - 1, rows [r0, r0 + nr) */
  int qtiles, site;              /* query tiles of the profile kernel; the accumulate kernel's role */
};

template <bool MANY>
__global__ __launch_bounds__(SRX_PT) void sr_place_profile_kernel(PlaceArgs A)
{
  __shared__ int sa[SRX_MC], sb[SRX_MC];
  __shared__ double2 st[SRX_MC][SRX_QT];
  const int N = A.N, M = A.M, Q = A.Q, Mt = MANY ? M : 1;
  const long long s = blockIdx.x / A.qtiles;               /* the batch's sample: chain g, row r0 + r */
  const int q0 = (int)(blockIdx.x - s * A.qtiles) * SRX_QT;
  const int g = (int)(s / A.nr), r = (int)(s - (long long)g * A.nr);
  const int p = blockIdx.y * blockDim.x + threadIdx.x;
  const bool fl = A.flip && A.flip[A.k0 + g];
  const int16_t *row = A.rec + A.chain_off[A.k0 + g] + (long long)(A.r0 + r) * A.row_stride;
  const double *tr = A.tab + (size_t)s * 4 * Mt;
  double acc[SRX_QT];
#pragma unroll
  for (int j = 0; j < SRX_QT; ++j) acc[j] = 0.0;
  for (int m0 = 0; m0 < M; m0 += SRX_MC) {
    const int nm = min(SRX_MC, M - m0);
    for (int i = threadIdx.x; i < nm; i += blockDim.x) {
      const int a = row[m0 + i], b = row[M + m0 + i];
      sa[i] = fl ? N - b : a;
      sb[i] = fl ? N - a : b;
    }
    for (int i = threadIdx.x; i < nm * SRX_QT; i += blockDim.x) {
      const int j = i / nm, mm = i - j * nm, m = m0 + mm, q = q0 + j;
      const int y = q < Q ? A.Y[(size_t)q * M + m] : 2;
      const int mt = MANY ? m : 0;
      double2 t = make_double2(0.0, 0.0);
      if (y == 0) t = make_double2(tr[(size_t)Mt + mt], tr[mt]);
      else if (y == 1) t = make_double2(tr[(size_t)2 * Mt + mt], tr[(size_t)3 * Mt + mt]);
      st[mm][j] = t;
    }
    __syncthreads();
    for (int mm = 0; mm < nm; ++mm) {
      const bool alive = sa[mm] <= p && p < sb[mm];
#pragma unroll
      for (int j = 0; j < SRX_QT; ++j) {
        const double2 t = st[mm][j];
        acc[j] += alive ? t.x : t.y;
      }
    }
    __syncthreads();
  }
  if (p < N) {
#pragma unroll
    for (int j = 0; j < SRX_QT; ++j)
      if (q0 + j < Q) A.slab[((size_t)s * Q + (q0 + j)) * N + p] = acc[j];
  }
}

/* one wave per (sample, query): L -> w in place, lse */
__global__ __launch_bounds__(64 * SRX_NWAVES) void sr_place_norm_kernel(PlaceArgs A, long long pairs)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * SRX_NWAVES + wave;   /* sample * Q + query */
  if (i >= pairs) return;                                          /* the whole wave: no barrier below */
  const int N = A.N;
  double *L = A.slab + (size_t)i * N;
  sr_mtab tb;
  tb.exp_tab = x_exp_tab; tb.log_tab = x_log_tab;
  double mx = L[0];
  for (int p = lane; p < N; p += 64) mx = fmax(mx, L[p]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  double z = 0.0;
  for (int p = lane; p < N; p += 64) {
    const double e = sr_exp_m(L[p] - mx, &tb);
    L[p] = e;
    z += e;
  }
  double Z = 0.0;
#pragma unroll
  for (int j = 0; j < 64; ++j) Z += __shfl(z, j, 64);
  if (lane == 0) A.lse[i] = mx + sr_log_m(Z, &tb);
  for (int p = lane; p < N; p += 64) L[p] = L[p] / Z;
}

/* part[g][q][x] += w over the batch's rows in order; x a position, or a site read at its own position */
__global__ __launch_bounds__(SRX_ACC_THREADS) void sr_place_acc_kernel(PlaceArgs A)
{
  const int N = A.N, Q = A.Q, g = blockIdx.y;
  const size_t qn = (size_t)Q * N;
  const size_t i = (size_t)blockIdx.x * SRX_ACC_THREADS + threadIdx.x;   /* q * N + x */
  if (i >= qn) return;
  const int x = (int)(i % (size_t)N);
  const double *w = A.slab + (size_t)g * A.nr * qn + (i - x);            /* row r's [q][.] at w + r * qn */
  double *dst = A.part + (size_t)g * qn + i;
  double acc = *dst;
  if (!A.site) {
    for (int r = 0; r < A.nr; ++r) acc += w[(size_t)r * qn + x];
  } else {
    const bool fl = A.flip && A.flip[A.k0 + g];
    const int16_t *pi = A.rec + A.chain_off[A.k0 + g] + (long long)A.r0 * A.row_stride + 2 * (long long)A.M + x;
    for (int r = 0; r < A.nr; ++r) {
      const int v = pi[(long long)r * A.row_stride], pp = fl ? N - 1 - v : v;
      acc += (pp >= 0 && pp < N) ? w[(size_t)r * qn + pp] : 0.0;
    }
  }
  *dst = acc;
}

/* tot += part[0] + ... in chain order, one add after the other */
__global__ void sr_place_combine_kernel(double *tot, const double *part, int G, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double t = tot[i];
  for (int g = 0; g < G; ++g) t += part[(size_t)g * n + i];
  tot[i] = t;
}

__global__ void sr_place_finish_kernel(double *tot, double T, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tot[i] = tot[i] / T;
}

static long long srx_scratch(void)
{
  const char *e = getenv("SR_PLACE_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? v : SRX_SCRATCH_DEFAULT;
}

/* The placement of the Q rows of Y under the n_sel chains of a record view.  cd [n_sel] (each chain's [count][cdw]
   rows: c at [m], d at [Mt + m], Mt = M when manycd, else 1), Y [Q][M] and flip [n_sel] (or NULL) are host inputs,
   already checked; pos, site [Q][N] and lse [n_sel][count][Q] are host buffers, each optional. */
extern "C" int srx_place(const sr_recview *v, int N, int M, const double *const *cd, int cdw, int manycd,
                         const uint8_t *Y, int Q, const uint8_t *flip, double *pos, double *site, double *lse,
                         float *ms)
{
  int rc = 0;
  uint8_t *d_Y = nullptr, *d_flip = nullptr;
  double *d_cd = nullptr, *d_tab = nullptr, *d_slab = nullptr, *d_lse = nullptr, *d_part = nullptr, *d_tot = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!v) return -1;
  const int n_sel = v->n_sel, count = v->count;
  hipStream_t st = (hipStream_t)v->stream;
  if (!v->rec || !v->chain_off || !cd || !Y || Q < 1 || n_sel <= 0 || count < 1 || N < 1 || N > 32767 || M < 1 ||
      (long long)n_sel * count >= (1LL << 31) || (long long)Q * N > (1LL << 27))
    return -1;
  if (ms) *ms = 0.0f;
  const size_t qn = (size_t)Q * N;
  const int Mt = manycd ? M : 1;
  const double T = (double)((long long)n_sel * count);
  const long long scratch = srx_scratch();
  const int nrole = (pos ? 1 : 0) + (site ? 1 : 0);
  const int qtiles = (Q + SRX_QT - 1) / SRX_QT;
  /* chains per group: the partial planes; rows per batch: the slab, and a grid that stays within bounds */
  long long G = scratch / (long long)(qn * (nrole ? nrole : 1) * sizeof(double));
  if (G > n_sel) G = n_sel;
  if (G > SR_GRID_CAP) G = SR_GRID_CAP;
  if (G > SRX_GRID_X_MAX / Q) G = SRX_GRID_X_MAX / Q;
  if (G < 1) G = 1;
  long long RB = scratch / (G * (long long)(qn * sizeof(double)));
  if (RB > scratch / (G * (long long)Mt * 4 * (long long)sizeof(double)))
    RB = scratch / (G * (long long)Mt * 4 * (long long)sizeof(double));
  if (RB > SRX_GRID_X_MAX / (G * (long long)Q)) RB = SRX_GRID_X_MAX / (G * (long long)Q);
  if (RB > count) RB = count;
  if (RB < 1) RB = 1;
  const int pthreads = N >= SRX_PT ? SRX_PT : 64 * ((N + 63) / 64);
  const unsigned ptiles = (unsigned)((N + pthreads - 1) / pthreads);
  const unsigned qnb = (unsigned)((qn + 255) / 256);
  float total_ms = 0.0f;
  {
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMalloc(&d_Y, (size_t)Q * M));
    HIPCHK(hipMemcpy(d_Y, Y, (size_t)Q * M, hipMemcpyHostToDevice));
    if (flip) {
      HIPCHK(hipMalloc(&d_flip, (size_t)n_sel));
      HIPCHK(hipMemcpy(d_flip, flip, (size_t)n_sel, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&d_cd, sizeof(double) * G * RB * cdw));
    HIPCHK(hipMalloc(&d_tab, sizeof(double) * G * RB * 4 * Mt));
    HIPCHK(hipMalloc(&d_slab, sizeof(double) * G * RB * qn));
    HIPCHK(hipMalloc(&d_lse, sizeof(double) * G * RB * Q));
    if (nrole) {
      HIPCHK(hipMalloc(&d_part, sizeof(double) * G * nrole * qn));
      HIPCHK(hipMalloc(&d_tot, sizeof(double) * nrole * qn));
      HIPCHK(hipMemsetAsync(d_tot, 0, sizeof(double) * nrole * qn, st));
    }
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    PlaceArgs A;
    A.rec = v->rec; A.chain_off = v->chain_off; A.row_stride = v->row_stride; A.Y = d_Y; A.flip = d_flip;
    A.tab = d_tab; A.slab = d_slab; A.lse = d_lse; A.part = nullptr; A.N = N; A.M = M; A.Q = Q; A.qtiles = qtiles;
    A.site = 0;
    for (int k0 = 0; k0 < n_sel; k0 += (int)G) {
      const int ng = (int)(G < n_sel - k0 ? G : n_sel - k0);
      if (nrole) HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * G * nrole * qn, st));
      for (int r0 = 0; r0 < count; r0 += (int)RB) {
        const int nr = (int)(RB < count - r0 ? RB : count - r0);
        for (int g = 0; g < ng; ++g)
          HIPCHK(hipMemcpyAsync(d_cd + (size_t)g * nr * cdw, cd[k0 + g] + (size_t)r0 * cdw, sizeof(double) * nr * cdw,
                                hipMemcpyHostToDevice, st));
        const long long ns = (long long)ng * nr, pairs = ns * Q;
        A.k0 = k0; A.r0 = r0; A.nr = nr; A.ng = ng;
        HIPCHK(hipEventRecord(e0, st));
        hipLaunchKernelGGL(sr_place_table_kernel, dim3((unsigned)((ns * Mt + SRX_TAB_THREADS - 1) / SRX_TAB_THREADS)),
                           dim3(SRX_TAB_THREADS), 0, st, d_cd, cdw, Mt, ns, d_tab);
        HIPCHK(hipGetLastError());
        const dim3 pg((unsigned)(ns * qtiles), ptiles);
        if (manycd) hipLaunchKernelGGL(sr_place_profile_kernel<true>, pg, dim3(pthreads), 0, st, A);
        else hipLaunchKernelGGL(sr_place_profile_kernel<false>, pg, dim3(pthreads), 0, st, A);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sr_place_norm_kernel, dim3((unsigned)((pairs + SRX_NWAVES - 1) / SRX_NWAVES)),
                           dim3(64 * SRX_NWAVES), 0, st, A, pairs);
        HIPCHK(hipGetLastError());
        for (int role = 0, slot = 0; role < 2; ++role) {
          if (!(role ? site : pos)) continue;
          A.site = role;
          A.part = d_part + (size_t)slot * G * qn;
          hipLaunchKernelGGL(sr_place_acc_kernel, dim3(qnb, ng), dim3(SRX_ACC_THREADS), 0, st, A);
          HIPCHK(hipGetLastError());
          if (r0 + nr == count) {
            hipLaunchKernelGGL(sr_place_combine_kernel, dim3(qnb), dim3(256), 0, st, d_tot + (size_t)slot * qn,
                               A.part, ng, qn);
            HIPCHK(hipGetLastError());
            if (k0 + ng == n_sel) {
              hipLaunchKernelGGL(sr_place_finish_kernel, dim3(qnb), dim3(256), 0, st, d_tot + (size_t)slot * qn, T, qn);
              HIPCHK(hipGetLastError());
            }
          }
          ++slot;
        }
        HIPCHK(hipEventRecord(e1, st));
        if (lse)
          for (int g = 0; g < ng; ++g)
            HIPCHK(hipMemcpyAsync(lse + ((size_t)(k0 + g) * count + r0) * Q, d_lse + (size_t)g * nr * Q,
                                  sizeof(double) * nr * Q, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));   /* the next batch overwrites d_cd, d_tab, the slab and d_lse */
        float t = 0.0f;
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        total_ms += t;
      }
    }
    if (ms) *ms = total_ms;
    if (pos) HIPCHK(hipMemcpy(pos, d_tot, sizeof(double) * qn, hipMemcpyDeviceToHost));
    if (site) HIPCHK(hipMemcpy(site, d_tot + (pos ? qn : 0), sizeof(double) * qn, hipMemcpyDeviceToHost));
  }
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (d_Y) (void)hipFree(d_Y);
  if (d_flip) (void)hipFree(d_flip);
  if (d_cd) (void)hipFree(d_cd);
  if (d_tab) (void)hipFree(d_tab);
  if (d_slab) (void)hipFree(d_slab);
  if (d_lse) (void)hipFree(d_lse);
  if (d_part) (void)hipFree(d_part);
  if (d_tot) (void)hipFree(d_tot);
  return rc;
}
