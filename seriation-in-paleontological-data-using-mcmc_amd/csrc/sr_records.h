/*
 * sr_records.h -- the record view: how the analyses over saved records (posterior summaries, convergence
 * diagnostics, marginals, taxon-pair relations, WAIC, PSIS-LOO, chain agreement, the central state, posterior predictive checks,
 * cell occupancy, placement of query rows)
 * address the rows they read, and those
 * analyses' entry points.  Plain C.  Included by sr_host.c, sr_records.hip and the analysis .hip files only: the
 * sweep kernel's sources (sr_device.hip, sr_internal.h; the snapshot sr_spec.c compiles from) know nothing of it.
 */
#ifndef SR_RECORDS_H
#define SR_RECORDS_H
#include <stdint.h>
#include <stddef.h>

/* A selection of record rows resident on a GPU: n_sel chains' `count` rows of int16 entries [a (M) | b (M) | pi (N)].
   Row t of selected chain k starts at rec + chain_off[k] + t * row_stride; rec and chain_off are device pointers.
   Chains [c0, c0 + n) of a view are a view again, with no allocation: sr_recview_chains. */
typedef struct {
  int device;
  void *stream;                 /* hipStream_t the kernels are queued on (NULL: the default stream) */
  const int16_t *rec;
  const long long *chain_off;   /* [n_sel] element offsets; owned by the view */
  int n_sel, count;
  long long row_stride;
  int owns_rec;                 /* 1: rec was uploaded by sr_recview_host and is freed with the view */
} sr_recview;

#ifdef __cplusplus
extern "C" {
#endif

/* Every function below returns 0, -1 (invalid argument), -4 (out of host memory) or -5 (a HIP error, reported on
   stderr); a view that was not built holds nothing to release. */

/* records from host memory: ab_pi [n_sel][count][W] (selection order) uploaded to `device`, chain k at k * count * W;
   count == 0 is a view of no rows */
int sr_recview_host(sr_recview *v, int device, const int16_t *ab_pi, int n_sel, int count, long long W);
/* records already on `device` (a session's buffer): only the offsets off [n_sel] (host memory) are uploaded */
int sr_recview_device(sr_recview *v, int device, void *stream, const int16_t *d_rec, const long long *off, int n_sel,
                      int count, long long row_stride);
void sr_recview_release(sr_recview *v);

/* chains [c0, c0 + n) of v: borrows everything, is not released */
static inline sr_recview sr_recview_chains(const sr_recview *v, int c0, int n)
{
  sr_recview s = *v;
  s.chain_off += c0;
  s.n_sel = n;
  s.owns_rec = 0;
  return s;
}

/* The analyses: one entry point each, over a view.  Inputs other than the records and all outputs are host
   memory; ms (optional) receives the kernels' time.  sr_host.c refers to all of them, and to the view's functions,
   weakly: the host-only builds (device layer stubbed) have none and answer SR_EUNSUPPORTED. */

/* posterior summaries (sr_post.hip): one kind (an SR_POST_* bit position) per call, out_host [R][C] */
#define SRP_PAIR_ORDER 0
#define SRP_ALIVE 1
#define SRP_FALSE_ALIVE 2
#define SRP_FALSE_ONES 3
#define SRP_EXP_PI 4
#define SRP_EXP_A 5
int srp_posterior(const sr_recview *v, int kind, int N, int M, const uint8_t *X_host, int chains_selected,
                  double *out_host, float *ms);
/* convergence diagnostics (sr_diag.hip): the exact integer moments of the view's chains, two sequences of
   h = count / 2 rows per chain (rows [0, h) and [count - h, count)), lags 0..L (1 <= L < h): P, F, B
   [2 n_sel][L+1][W] and S1 [2 n_sel][W], W = 2M + N */
int srd_moments(const sr_recview *v, int W, int L, long long *P, long long *F, long long *B, long long *S1, float *ms);
/* posterior marginals (sr_marg.hip): the exact histograms of every record column (bins 0..N, a flagged chain's rows
   reflected) and what is read off them; flip [n_sel] (or NULL) and probs [Q] (Q <= 16) are inputs, hist [W][N+1],
   outside [W], pi_sum [n_sel][N], quant [Q][W], mode [W], mean [W] outputs, each optional */
int srm_marginals(const sr_recview *v, int N, int M, const uint8_t *flip, const double *probs, int Q, uint32_t *hist,
                  uint32_t *outside, long long *pi_sum, int32_t *quant, int32_t *mode, double *mean, float *ms);
/* taxon-pair relations, durations, richness (sr_rel.hip): exact counts, a flagged chain's limits reflected; flip
   [n_sel] (or NULL) is an input, pair[4] (orig_before, ext_before, precedes, overlap: [M][M] each), dur_hist
   [M][N+1], dur_outside [M], rich_hist [N][M+1] outputs, each optional */
int srr_relations(const sr_recview *v, int N, int M, const uint8_t *flip, uint32_t *const pair[4], uint32_t *dur_hist,
                  uint32_t *dur_outside, uint32_t *rich_hist, float *ms);
/* WAIC's pointwise terms (sr_waic.hip): lppd, ll_mean (optional), pwaic [N][M], summed in the order
   include/seriation.h fixes.  X [N][M] and cd [n_sel] are inputs: chain k's c, d rows [count][cdw], c of taxon m at
   [m], d at [Mt + m], Mt = M when manycd and 1 otherwise (cdw 3 takes the (c, d, loglik) rows as they are), every
   value already checked against the domain */
int srw_waic(const sr_recview *v, int N, int M, const uint8_t *X, const double *const *cd, int cdw, int manycd,
             double *lppd, double *ll_mean, double *pwaic, float *ms);
/* PSIS-LOO's pointwise terms (sr_loo.hip): lppd, elpd, pareto_k [N][M], as include/seriation.h defines them.  X, cd,
   cdw and manycd as srw_waic takes them; n the tail length of T = n_sel * count (at most 4096), G [m] and L [n] the
   host tables of the fit (not read when n < 5); ms3 [3] (optional) the kernels' time of the sum, the selection and
   the finish phase */
int srl_loo(const sr_recview *v, int N, int M, const uint8_t *X, const double *const *cd, int cdw, int manycd, int n,
            int m, const double *G, const double *L, double *lppd, double *elpd, double *pareto_k, float *ms3);
/* chain agreement (sr_agree.hip): pair_counts [n_sel][N][N], dist and dist_mirror [n_sel][n_sel] (only the pi part of
   a row is read), exact integers, each optional.  sra_distances_host is the reduction alone, from pair counts in
   host memory (any uint32 values): it reads no records and takes no view. */
int sra_agreement(const sr_recview *v, int N, int M, uint32_t *pair_counts, long long *dist, long long *dist_mirror,
                  float *ms);
int sra_distances_host(int device, int N, int n_sel, const uint32_t *pair_counts, long long *dist,
                       long long *dist_mirror, float *ms);

/* the central sampled state (sr_central.hip): flip [n_sel] (or NULL) is an input; order_loss, limit_loss
   [n_sel][count], pair_counts [N][N] (pooled, oriented), best [n_sel], state [2M+N] outputs, each optional; *chain and
   *row the central row's.  src_order_loss is the order loss alone against counts in host memory (against [N][N], any
   uint32 values). */
int src_central(const sr_recview *v, int N, int M, const uint8_t *flip, long long *order_loss, long long *limit_loss,
                uint32_t *pair_counts, int32_t *best, int32_t *state, int32_t *chain, int32_t *row, float *ms);
int src_order_loss(const sr_recview *v, int N, int M, const uint8_t *flip, const uint32_t *against,
                   long long *order_loss, float *ms);

/* posterior predictive checks (sr_ppc.hip): exact integers, defined in include/seriation.h.  X, cd, cdw and manycd
   as srw_waic takes them; reps in 1..64 and n_sel * count * reps < 2^31.  taxon_gt, taxon_eq, taxon_sum_obs,
   taxon_sum_rep [5][M], site_gt, site_eq, site_sum_rep [N], total_obs [n_sel][count][5], total_rep
   [n_sel][count][reps][5] are outputs, each optional; total_gt, total_eq [5] are always written */
int srq_ppc(const sr_recview *v, int N, int M, const uint8_t *X, const double *const *cd, int cdw, int manycd,
            uint64_t seed, int reps, uint32_t *taxon_gt, uint32_t *taxon_eq, long long *taxon_sum_obs,
            long long *taxon_sum_rep, uint32_t *site_gt, uint32_t *site_eq, long long *site_sum_rep,
            long long *total_obs, long long *total_rep, long long *total_gt, long long *total_eq, float *ms);

/* cell occupancy and the site and taxon error tallies (sr_occ.hip): exact counts, defined in include/seriation.h.
   X [N][M] is an input; alive [N][M], site[3] (the histograms of alive, f0, f1: [N][M+1] each) and taxon[3]
   ([M][N+1] each) are outputs, each optional (the two arrays of three pointers themselves are not) */
int sro_occupancy(const sr_recview *v, int N, int M, const uint8_t *X, uint32_t *alive, uint32_t *const site[3],
                  uint32_t *const taxon[3], float *ms);

/* placement of query rows (sr_place.hip): defined to the bit in include/seriation.h.  cd, cdw and manycd as srw_waic
   takes them; Y [Q][M] (0 absent, 1 present, 2 not assessed) and flip [n_sel] (or NULL) are inputs; pos, site [Q][N]
   and lse [n_sel][count][Q] outputs, each optional */
int srx_place(const sr_recview *v, int N, int M, const double *const *cd, int cdw, int manycd, const uint8_t *Y, int Q,
              const uint8_t *flip, double *pos, double *site, double *lse, float *ms);

#ifdef __cplusplus
}
#endif

#endif
