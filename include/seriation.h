/*
 * seriation.h -- C ABI of libseriation.so, the MI355X-native drop-in for the reference's
 * per-chain MCMC sweep (PrayagS/Seriation-in-Paleontological-Data-using-MCMC,
 * C_Implementation/mcmc.c).  Plain C types only; caller-owned buffers; every function
 * returns SR_OK (0) or a negative SR_E* code -- the library never calls exit().
 *
 * Reference interfaces replaced (file:line in the reference tree):
 *   sr_parse_dataset / sr_load_dataset   mcmc_readmodel            mcmc.c:339-437, mcmc.h:47
 *   sr_run_chains / sr_session_*         mcmc_init + mcmc_randomize + mcmc_sample loop
 *                                         mcmc.c:127-185, 214-258, 477-593, mcmc.h:48,51,55
 *   sr_chain_summary.exp_*               compute_exp_data / print_exp_data  mcmc.c:53-67
 *   sr_record / sink                     mcmc_save_chain           mcmc.c:69-92
 *   sr_run_to_dirs                       main()'s Chains/chain_XX/<name>.csv output  mcmc.c:148-197, 261-293
 *   sr_chain_summary.consistent          mcmc_consistent           mcmc.c:999-1094, 199-204
 *   sr_chain_spec.seed                   GSL_RNG_SEED via gsl_rng_env_setup  mcmc.c:591 / script.py:42
 * A chain's trajectory depends only on (dataset, seed): sharding chains over devices or
 * sessions never changes any chain's output.
 */
#ifndef SERIATION_H
#define SERIATION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SR_OK 0
#define SR_EINVAL (-1)         /* bad argument */
#define SR_EPARSE (-2)         /* "mcmc_readmodel: read error." (mcmc.c:349, 371) */
#define SR_EHEADER (-3)        /* "mcmc_readmodel: read error at header." (mcmc.c:355) */
#define SR_ENOMEM (-4)
#define SR_EDEVICE (-5)        /* HIP runtime error or no gfx950 device */
#define SR_EUNSUPPORTED (-6)   /* configuration outside the kernel's limits */
#define SR_EIO (-7)            /* cannot open/write an output file */
#define SR_EINCONSISTENT (-8)  /* mcmc_consistent failed after the run (mcmc.c:199-204) */

#define SR_MAXS 2000           /* mcmc.h:25 line limit of the reference parser */

typedef struct {
  int32_t N, M, nh;   /* sites, taxa, hard sites */
  uint8_t *X;         /* N*M, row-major (row = site), 0/1 */
  uint8_t *hard;      /* N, 1 if the row ended with '*' */
} sr_dataset;

/* maxs = SR_MAXS reproduces the reference's fgets(MAXS) semantics exactly (a longer line
 * is split and its tail read as the next row); maxs = 0 reads lines of any length. */
int sr_parse_dataset(const char *text, size_t len, int32_t maxs, sr_dataset *out);
int sr_load_dataset(const char *path, int32_t maxs, sr_dataset *out);
void sr_free_dataset(sr_dataset *ds);
/* Binary bit-packed form ("SRBX" header, N hard bytes, N rows of ceil(M/8) bytes; SURVEY §8f-4,
 * an extension: the reference reads text only).  sr_load_dataset also accepts it (by magic). */
int sr_save_dataset_bin(const sr_dataset *ds, const char *path);
int sr_load_dataset_bin(const char *path, sr_dataset *out);

typedef struct {
  int32_t chain_id;   /* names the output directory Chains/chain_NN */
  uint64_t seed;      /* GSL_RNG_SEED value (0 -> GSL default 4357) */
} sr_chain_spec;

typedef struct {
  int32_t burnin_calls;      /* tb: mcmc_sample calls before saving (mcmc.c:107, default 1000) */
  int32_t sample_calls;      /* ts: saved mcmc_sample calls (default 1000) */
  int32_t sweeps_per_call;   /* sweeps per mcmc_sample (mcmc.c:225, default 10) */
  int32_t manycd;            /* mcmc_readmodel's manycd (mcmc.h:40, mcmc.c:118): 0 = c, d shared by all taxa (the
                                reference CLI's default and script.py's); nonzero = per-taxon c[m], d[m] drawn one
                                after another each sweep (mcmc.c:777-786, 807-816) -- the exact (slower) kernel
                                paths, block_threads 0 or 1024 */
  int32_t device;            /* HIP device ordinal */
  int32_t block_threads;     /* threads per chain workgroup, 0 = auto */
  int32_t calls_per_launch;  /* mcmc_sample calls per kernel launch, 0 = auto */
  int32_t flags;             /* SR_F_* */
} sr_run_opts;
#define SR_F_NO_CHECK 1      /* skip the closing mcmc_consistent check */
#define SR_F_HBM_COLUMNS 2   /* force the HBM-column kernel variant (default: only when LDS is too small) */
#define SR_F_LDS_COLUMNS 4   /* force the LDS-column variant (SR_EUNSUPPORTED if it does not fit) */
#define SR_F_DEBUG_CHECK 8   /* the reference's MCMCDEBUG (mcmc.c:249-255): mcmc_consistent on every chain after
                                every mcmc_sample call (one call per launch); SR_EINCONSISTENT on the first failure */
#define SR_F_DEBUG_PRINT 16  /* with SR_F_DEBUG_CHECK: MCMCDEBUG's acceptance-rate line on stderr per chain and call */
#define SR_F_RNG_PHILOX 32   /* opt-in: the sampling phase draws every word from a counter-based Philox4x32-10 stream
                                keyed by the chain's seed instead of GSL's MT19937 (initialisation unchanged).  Not
                                the reference's stream: statistically equivalent, not bit-equal.  A checkpoint
                                keeps its stream kind; restoring it needs the same flag (else SR_EINVAL). */
#define SR_F_DIAG 64         /* the reference's stderr diagnostics during initialisation: "mcmc_initab: zero column
                                at %d, continuing." per all-zero column, from mcmc_readmodel's and mcmc_randomize's
                                mcmc_initab (mcmc.c:457); the drop-in CLI sets it */
#define SR_F_GENERIC_KERNEL 128  /* run the generic sweep kernel (shape from the launch arguments) instead of the
                                    default shape-specialised one (sr_session_specialized); SR_JIT=0 in the
                                    environment does the same.  Results are identical either way. */

typedef struct {
  int32_t chain_id;
  int32_t consistent;        /* 0 = mcmc_consistent passed (as the reference's exit 0) */
  double exp_loglik, exp_c, exp_d;   /* exactly print_exp_data's values (sums / 1000) */
} sr_chain_summary;

typedef struct {
  int32_t N, M;
  const int32_t *a, *b, *pi;  /* M, M, N: one mcmc_save_chain line */
  double c, d, loglik;        /* log P(false 1), log P(false 0) (manycd: taxon 0's), loglik */
  const double *cv, *dv;      /* manycd: every taxon's c[M], d[M]; NULL when all taxa share c, d */
} sr_record;

/* Called once per saved sample, per chain in sample order; return nonzero to abort. */
typedef int (*sr_sample_sink_fn)(void *ctx, int32_t chain_index, int32_t sample_index,
                                 const sr_record *rec);

void sr_default_opts(sr_run_opts *o);

/* gsl_rng_env_setup (mcmc_init, mcmc.c:591-592; GSL 2.6 rng/env.c) for callers that take the seed from the
 * environment as the reference CLI does: GSL_RNG_TYPE unset or "mt19937" -> SR_OK (verbose: the line
 * "GSL_RNG_TYPE=mt19937" when set), then GSL_RNG_SEED (strtoul base 0, unset -> 0 = GSL's default 4357;
 * verbose: "GSL_RNG_SEED=<value>") into *seed.  Another GSL generator -> SR_EUNSUPPORTED (the sampler
 * implements MT19937's stream only), a name GSL does not know -> SR_EINVAL (verbose: GSL's "not recognized"
 * message and list of generator types).  Every session / run entry point that samples MT19937's stream
 * applies the same GSL_RNG_TYPE check (silently) and refuses with the same codes, so no run samples MT19937
 * where the environment named another generator; SR_F_RNG_PHILOX sessions sample no GSL stream and ignore it.
 * Departure: for an unknown name GSL 2.6 prints the list, then its default error handler reports "unknown
 * generator" and aborts (SIGABRT); here the caller gets SR_EINVAL and the CLIs exit 1 (parity unpinned: no GSL
 * here to take the handler's exact line from). */
int sr_rng_env_setup(uint64_t *seed, int32_t verbose);

/* Run n_chains independent chains on one GPU (opts->device), burn-in then sampling;
 * per-sample records go to sink (may be NULL); out[n_chains] receives the summaries. */
int sr_run_chains(const sr_dataset *ds, const sr_chain_spec *specs, int32_t n_chains,
                  const sr_run_opts *opts, sr_sample_sink_fn sink, void *sink_ctx,
                  sr_chain_summary *out);

/* Same run, writing Chains/chain_NN/{chain_data,exp_data,taxa,sites,hard_sites}.csv
 * under chains_root byte-for-byte as the reference's main() does. */
int sr_run_to_dirs(const sr_dataset *ds, const sr_chain_spec *specs, int32_t n_chains,
                   const sr_run_opts *opts, const char *chains_root, sr_chain_summary *out);

/* Several GPUs from one call (the reference runs one process per chain, script.py:55-62):
 * chains sharded contiguously over n_devices shards, shard k on HIP device devices[k] (an ordinal may
 * repeat: those shards share the GPU), one host thread per shard.  Every output equals the
 * sr_run_chains / sr_run_to_dirs one; the sink is serialised and receives global chain indices
 * (samples in order per chain, chains of different shards interleaved).  opts->device is ignored. */
int sr_run_chains_multi(const sr_dataset *ds, const sr_chain_spec *specs, int32_t n_chains,
                        const sr_run_opts *opts, const int32_t *devices, int32_t n_devices,
                        sr_sample_sink_fn sink, void *sink_ctx, sr_chain_summary *out);
int sr_run_to_dirs_multi(const sr_dataset *ds, const sr_chain_spec *specs, int32_t n_chains,
                         const sr_run_opts *opts, const int32_t *devices, int32_t n_devices,
                         const char *chains_root, sr_chain_summary *out);

/* ---- sessions: chains resident in HBM on one GPU, asynchronous launches ---- */
typedef struct sr_session sr_session;
int sr_session_create(const sr_dataset *ds, const sr_chain_spec *specs, int32_t n_chains,
                      const sr_run_opts *opts, sr_session **out);
/* Launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int sr_session_set_stream(sr_session *s, void *hip_stream);
/* Enqueue `calls` mcmc_sample calls for every chain; save != 0 appends one record per call. */
int sr_session_run(sr_session *s, int32_t calls, int32_t save);
int sr_session_sync(sr_session *s);
int32_t sr_session_records(const sr_session *s);
int32_t sr_session_record_capacity(const sr_session *s);
/* ab_pi: [n_chains][count][2M+N] int16 (a, b, pi); cdl: [n_chains][count][3] (c, d, loglik);
   either may be NULL (not fetched) */
int sr_session_fetch_records(sr_session *s, int32_t first, int32_t count, int16_t *ab_pi, double *cdl);
int sr_session_reset_records(sr_session *s);
/* One chain's buffered records [first, first + count): ab_pi [count][2M+N] int16, cdl [count][3]
   (either may be NULL). */
int sr_session_fetch_chain_records(sr_session *s, int32_t chain, int32_t first, int32_t count, int16_t *ab_pi,
                                   double *cdl);
/* The same rows copied device to device into caller-owned memory on the session's GPU (dev_ab_pi [count][2M+N]
   int16, dev_cdl [count][3]; either may be NULL), queued on the session stream without waiting: the records
   never leave HBM (e.g. straight into the buffer of an RCCL all-gather on that stream). */
int sr_session_copy_chain_records(sr_session *s, int32_t chain, int32_t first, int32_t count, int16_t *dev_ab_pi,
                                  double *dev_cdl);
/* manycd sessions: the per-taxon c, d of buffered records [first, first + count): cdv [n_chains][count][2M]
   (c[M] then d[M], log values as mcmc_save_chain exponentiates them); SR_EINVAL for manycd = 0 sessions. */
int sr_session_fetch_cd_vectors(sr_session *s, int32_t first, int32_t count, double *cdv);
int32_t sr_session_manycd(const sr_session *s);
/* compute_exp_data / print_exp_data (mcmc.c:53-67) of every chain over its buffered records [first,
   first + count): out[c] = {chain_id, 0, sum(-loglik) / 1000, sum(e^c) / 1000, sum(e^d) / 1000}, sums in
   sample order, the reference's hard-coded divisor (exact means when count = 1000). */
int sr_session_summaries(sr_session *s, int32_t first, int32_t count, sr_chain_summary *out);
/* Current state of one chain (any pointer may be NULL); counts = t0,f0,t1,f1 (4*M). */
int sr_session_state(sr_session *s, int32_t chain, int32_t *a, int32_t *b, int32_t *pi,
                     double *c_d_loglik, int32_t *counts);
/* manycd sessions: one chain's current per-taxon c[M], d[M] (log values; either may be NULL); SR_EINVAL for
   manycd = 0 sessions (their c, d are sr_session_state's). */
int sr_session_state_cd(sr_session *s, int32_t chain, double *c, double *d);
/* Acceptance counters cc, cd, cab, cpi1, cpi20, cpi21, cpi3 (mcmc.c:220). */
int sr_session_accept_counts(sr_session *s, int32_t chain, int64_t *acc7);
/* How often the fast paths fell back to the reference's own computation (no counterpart in
   mcmc.c; every fallback is bit-exact): fb3 = {proposals decided by the exact sequential delta,
   Gibbs draws by the exact three-pass walk, c/d draws by the sequential GSL path}. */
int sr_session_fallback_counts(sr_session *s, int32_t chain, int64_t *fb3);
/* SR_F_DEBUG_CHECK: 1 if the chain failed mcmc_consistent after some mcmc_sample call of this
   session (the check of mcmc.c:254; sticky), 0 if not or without the flag. */
int sr_session_debug_flagged(const sr_session *s, int32_t chain);
/* Device time of the last sr_session_run (ms, HIP events on the session stream; syncs). */
double sr_session_last_kernel_ms(sr_session *s);
int32_t sr_session_block_threads(const sr_session *s);
/* Kernel variant the session runs: 0 = occurrence columns in LDS, one thread per taxon; 1 = columns
 * in HBM (chosen when the LDS layout exceeds 160 KB, e.g. 1024 sites x 2048 taxa); 2 is no longer
 * returned (it was the retired pair kernel, two lanes per taxon: slower than variant 0, DESIGN.md
 * "Retired experiments");
 * 3 = columns in HBM, split chains: two co-resident workgroups per chain, each owning half of the
 * taxa (1024 threads, 1025..2048 taxa, grid co-resident; SR_SPLIT=0 in the environment disables it). */
int32_t sr_session_variant(const sr_session *s);
/* 1 when the session's launches use the sweep kernel compiled for its exact shape (sites, taxa, hard
 * sites fixed at compile time) -- the default for sessions with occurrence columns in LDS (variant 0) --
 * 0 for the generic kernel (HBM columns, SR_F_GENERIC_KERNEL / SR_JIT=0, or the
 * specialised code object unavailable: one stderr line says why).  Results are identical either way. */
int32_t sr_session_specialized(const sr_session *s);
/* Prepare the shape-specialised kernel a session of this dataset and opts (block_threads, SR_F_*_COLUMNS,
 * SR_F_GENERIC_KERNEL) would run, without a GPU: compiled from the source snapshot the library was built
 * from (build/spec/) with hipcc into the cache ($SR_JIT_CACHE, else build/jit/ next to the library), so
 * that session creation finds it.  1 ready, 0 the session runs no specialised kernel, SR_EIO the code
 * object could not be produced (stderr says why), SR_EUNSUPPORTED / SR_EINVAL as sr_session_create.
 * (Session creation compiles a missing shape itself unless SR_JIT=cache: then only embedded or cached objects
 * are used and any other shape runs the generic kernel -- no compiler is spawned at run time.) */
int sr_specialize(const sr_dataset *ds, const sr_run_opts *opts);
/* Checkpoint / resume (the reference has none): the full chain state (columns, pi,
   limits, counts, c/d/loglik, MT19937 ring and cursor, acceptance counters) and the session's buffered
   records to a file; restoring it over the same dataset continues every chain exactly where it stopped,
   with the records in the new session's buffer (its capacity: the larger of opts->calls_per_launch and the
   record count), so summaries over a resumed sampling phase equal an uninterrupted run's.  Files without
   records (versions 3 / 4, before round 5) still restore, with an empty record buffer. */
int sr_session_checkpoint(sr_session *s, const char *path);
int sr_session_restore(const sr_dataset *ds, const char *path, const sr_run_opts *opts, sr_session **out);
void sr_session_destroy(sr_session *s);

/* ---- posterior summaries over saved samples, on the GPU ----
 * Replace the per-sample loops of the reference's analysis script (script.py):
 *   pair_order  [N][N]  compute_pair_order_matrix / generate_po_matrix   script.py:155-189
 *   alive       [N][M]  X_sum of plot_taxa_occurence_probability_matrix  script.py:306-333
 *   false_alive [N][M]  X_sum of plot_false_taxa_occurence_probability   script.py:350-377
 *   false_ones  [N][M]  X_sum of plot_false_ones_probability             script.py:392-417
 *   exp_pi      [N]     compute_exp_pi                                   script.py:230-251
 *   exp_a       [M]     compute_exp_a                                    script.py:254-275
 * bit for bit, quirks included (per-chain accumulators never reset, the fixed /1000, the
 * [site][taxon] loops comparing the site index with the limits); the argsort reorderings that
 * follow in the script are left to the caller.  NULL outputs are skipped; kernel_ms receives
 * the summed device time.  Samples are mcmc_save_chain rows (a, b, pi with pi[site] = position). */
typedef struct {
  double *pair_order, *alive, *false_alive, *false_ones, *exp_pi, *exp_a;
  double kernel_ms;
} sr_posterior_out;
/* ab_pi: [n_sel][count][2M+N] int16 host rows, chains in selection order; ds supplies N, M, X. */
int sr_posterior(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count,
                 int32_t chains_selected, int32_t device, sr_posterior_out *out);
/* The session's own records in HBM (no host round trip): chains[n_sel] are session chain
 * indices in selection order, samples [first, first + count) of its record buffer. */
int sr_session_posterior(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                         int32_t chains_selected, sr_posterior_out *out);

/* ---- convergence diagnostics over saved samples: split-R-hat and effective sample size ----
 * (an extension: the reference has none).  Quantity q runs over the W = 2M+N integer columns of a record row
 * (a | b | pi), then c, d, loglik (log scale as stored; manycd: taxon 0's): Q = W + 3.  Each of the n_sel chains'
 * `count` (>= 4) records gives two sequences of h = count / 2 rows, rows [0, h) and [count - h, count); S = 2 n_sel
 * sequences, chain 0's halves first.  Lags 0..L, L = max_lag (0 = h - 1; < 0 or >= h: SR_EINVAL).
 * The GPU computes the exact int64 moments of every integer column x_t of every sequence,
 *   P[s][k][j] = sum_{t <= h-1-k} x_t x_{t+k},  F[s][k][j] = sum_{t < k} x_t,  B[s][k][j] = sum_{t >= h-k} x_t,
 *   S1[s][j] = sum_t x_t;
 * the host forms G = h^2 P_k - h S1 (2 S1 - B_k - F_k) + (h - k) S1^2 exactly (128-bit), rounds it to f64 once,
 * gamma_k = G / h^3 (biased autocovariance), m = S1 / h, var = gamma_0 h / (h - 1); the scalar columns take the
 * same quantities from two sequential f64 passes.  Then, in f64 (sums over sequences in ascending order):
 * Wv = mean var, Bh = sum (m - mean m)^2 / (S - 1), vp = (h-1)/h Wv + Bh, rhat = sqrt(vp / Wv),
 * rho_k = 1 - (Wv - mean gamma_k) / vp, Geyer's initial monotone sequence over the pairs rho_2j + rho_2j+1
 * (cut_lag = 2j of the first negative pair, -1 if the lags ran out: ess is then an upper estimate),
 * tau = max(-1 + 2 sum, 1 / log10(S h)), ess = S h / tau: the split-R-hat / ESS of BDA3 and Vehtari et al. 2021
 * without rank normalisation.  A column that never moved (Wv = 0) has rhat = ess = NaN, cut_lag = -1. */
typedef struct {
  int32_t max_lag;                 /* in: 0 = h-1 */
  double *rhat, *ess;              /* [2M+N+3], NULL = skip */
  int32_t *cut_lag;                /* [2M+N+3], NULL = skip */
  int64_t *P, *F, *B, *S1;         /* optional raw moments: [S][L+1][W], [S][L+1][W], [S][L+1][W], [S][W]; NULL = skip */
  double kernel_ms;                /* out */
} sr_diag_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16, cdl [n_sel][count][3] (NULL: scalar entries NaN) */
int sr_diagnostics(const sr_dataset *ds, const int16_t *ab_pi, const double *cdl, int32_t n_sel, int32_t count,
                   int32_t device, sr_diag_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order) */
int sr_session_diagnostics(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                           sr_diag_out *out);
/* host only, no GPU: moments (+ optional scalar traces cdl [n_sel][count][3]) -> rhat / ess / cut_lag */
int sr_diag_reduce(int32_t W, int32_t n_sel, int32_t count, int32_t max_lag, const int64_t *P, const int64_t *F,
                   const int64_t *B, const int64_t *S1, const double *cdl, double *rhat, double *ess, int32_t *cut_lag);

/* ---- posterior marginals over saved samples: exact histograms, quantiles, modes, means ----
 * (an extension: the reference has none).  Records are rows [a (M) | b (M) | pi (N)] int16, W = 2M + N, with
 * pi[site] = position; chains in selection order, as for sr_posterior.  Every column has N + 1 bins for the values
 * 0..N (limits lie in [0, N]; positions in [0, N-1], so a pi column's bin N stays 0 for a sampler's records).
 * flip [n_sel] (NULL = none) reflects a flagged chain's rows before counting -- the likelihood is unchanged when the
 * order is reflected (position p -> N-1-p, alive interval [a, b) -> [N-b, N-a)), so chains of a dataset without hard
 * sites may settle in mirrored orders and must be oriented before they are pooled: the a column of taxon m takes
 * N - b_m, its b column N - a_m, a pi column N - 1 - pi.
 *   hist [W][N+1]     the number of the n_sel * count samples whose (possibly reflected) value is v
 *   outside [W]       values outside [0, N] after reflection (host records may hold any int16): counted here only
 *   pi_sum [n_sel][N] per-chain sum of the raw, unreflected pi column (the input of an orientation decision)
 * and per column j, with T_j the sum of hist[j] and C_j(v) its cumulative count, for each of n_probs <= 16
 * probabilities p in [0, 1]:
 *   quant [n_probs][W]  min{v : C_j(v) >= k}, k = clamp(ceil(p * (double)T_j), 1, T_j) (one f64 multiply, one ceil):
 *                       the k-th smallest in-range value, p = 0.5 the lower median
 *   mode [W]            the bin with the largest count, the lowest on ties
 *   mean [W]            (sum_v v hist[j][v]) / T_j: the numerator exact in int64, one f64 division
 * T_j = 0: quant = mode = -1, mean = NaN.  Integers, or one correctly rounded f64 operation on exact integers:
 * the result does not depend on the order of the sums.  Every output pointer is optional (NULL = skip).
 * SR_EINVAL: n_sel <= 0, count < 1, n_sel * count >= 2^31, n_probs outside [0, 16], a p outside [0, 1] or NaN,
 * N > 32767; the session form also for rows beyond the buffered records or a chain index out of range.  The
 * histograms are built on the GPU in column batches of at most 256 MB, so a call without hist works for any N. */
typedef struct {
  const uint8_t *flip;     /* in: [n_sel] or NULL */
  const double *probs;     /* in: [n_probs] */
  int32_t n_probs;
  uint32_t *hist;          /* out: [W][N+1], NULL = skip */
  uint32_t *outside;       /* out: [W] */
  int64_t *pi_sum;         /* out: [n_sel][N] */
  int32_t *quant, *mode;   /* out: [n_probs][W], [W] */
  double *mean;            /* out: [W] */
  double kernel_ms;        /* out */
} sr_marg_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M */
int sr_marginals(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count, int32_t device,
                 sr_marg_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order); the session's state
   and records are left untouched */
int sr_session_marginals(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                         sr_marg_out *out);

/* ---- taxon-pair relations, durations and the diversity curve over saved samples: exact counts ----
 * (an extension: the reference has none).  Joint functions of the limits, which no per-column output can give.
 * Records are rows [a (M) | b (M) | pi (N)] int16 as above; only the first 2M entries of a row are read; chains in
 * selection order.  flip [n_sel] (NULL = none) reflects a flagged chain's rows first, as in sr_marginals:
 * a'_m = N - b_m, b'_m = N - a_m.  All arithmetic is int32: any int16 input is legal and nothing wraps
 * (N - (-32768) is simply a large value).  T = n_sel * count samples; taxon m is alive at position p when
 * a_m <= p < b_m.
 * Pair matrices, each [M][M] uint32, entry [i][j] the number of the T samples with
 *   orig_before   a_i < a_j                          i originates strictly earlier
 *   ext_before    b_i < b_j                          i ends strictly earlier
 *   precedes      b_i <= a_j                         i is over before j begins; the diagonal counts empty intervals
 *   overlap       max(a_i, a_j) < min(b_i, b_j)      i and j share a position; symmetric; the diagonal counts
 *                                                    non-empty intervals
 * (pure comparisons: no value is "outside" for them).  Per taxon:
 *   dur_hist [M][N+1]   the samples with b_m - a_m = v, v in 0..N (unchanged by a reflection)
 *   dur_outside [M]     the samples whose difference lies outside [0, N]
 * Per position:
 *   rich_hist [N][M+1]  entry [p][r]: the samples in which exactly r taxa are alive at position p, p in 0..N-1;
 *                       defined for any input (limits beyond [0, N] simply clamp); every row sums to T
 * Every output pointer is optional (NULL = skip); a call only pays for what it asks.
 * SR_EINVAL: NULL ds, ab_pi or out, n_sel <= 0, count < 1, n_sel * count >= 2^31, N outside 1..32767, M < 1; the
 * session form also for rows beyond the buffered records or a chain index out of range.  SR_EUNSUPPORTED: a single
 * requested output larger than 1 GiB (a pair matrix with M > 16384, dur_hist with M (N+1) > 2^28, rich_hist with
 * N (M+1) > 2^28), or a library built without the device layer.  All reported before any device call. */
typedef struct {
  const uint8_t *flip;                                       /* in: [n_sel] or NULL */
  uint32_t *orig_before, *ext_before, *precedes, *overlap;   /* out: [M][M] each */
  uint32_t *dur_hist, *dur_outside;                          /* out: [M][N+1], [M] */
  uint32_t *rich_hist;                                       /* out: [N][M+1] */
  double kernel_ms;                                          /* out */
} sr_rel_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M */
int sr_relations(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count, int32_t device,
                 sr_rel_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order), on the session's
   stream; the session's state and records are left untouched */
int sr_session_relations(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                         sr_rel_out *out);

/* ---- WAIC and the pointwise model fit over saved samples: defined to the bit ----
 * (an extension: the reference's choose_chains compares mean -loglik, which cannot compare the shared-rates model
 * with the per-taxon one.)  Watanabe 2010; Vehtari, Gelman & Gabry 2017.  The likelihood factorises over the N M
 * cells of X (mcmc_logl, mcmc.c:625-648).  Records are rows [a (M) | b (M) | pi (N)] int16 as above, pi[site] =
 * position, chains in selection order; T = n_sel * count samples, sample (k, r) is row r of chain k.  The rates are
 * on the log scale as stored: manycd = 0: cd [n_sel][count][3], the (c, d, loglik) rows of
 * sr_session_fetch_records (loglik is not read); manycd != 0: cd [n_sel][count][2M], c[M] then d[M], as
 * sr_session_fetch_cd_vectors gives them.  No flip input: reflecting a chain (a' = N - b, b' = N - a,
 * pi' = N - 1 - pi) leaves every alive bit, and so every output, unchanged.
 * Term table, per sample (and per taxon when manycd): ec = exp(c), ed = exp(d) (this library's exp and log, bit
 * for bit the C library's), p = {1.0 - ec, ed, 1.0 - ed, ec}, l = {log(1.0 - ec), d, log(1.0 - ed), c}; the
 * indices: 0 true zero, 1 false zero, 2 true one, 3 false one.
 * Cell (n, m) in sample (k, r): alive = a_m <= pi_n < b_m, compared in int32 (any int16 is legal, nothing is
 * "outside"); with x = X[n][m] the index is 0 (x = 0, not alive), 1 (x = 0, alive), 2 (x = 1, alive), 3 (x = 1, not
 * alive).
 * Order of every sum over samples (part of the interface): within chain k sequentially over r ascending from +0.0,
 * then the chain sums sequentially over k ascending from +0.0; no fma, no floating-point atomics.
 * Pointwise, [N][M] f64: Sp the sum of the p terms, Sl of the l terms;
 *   lppd      log(Sp / (double)T)
 *   ll_mean   mu = Sl / (double)T
 *   pwaic     V / (double)(T - 1), V the sum, in the same order, of (l - mu) * (l - mu)
 * Reduction (plain C on the host; sr_waic_reduce runs it alone on given lppd, pwaic): e_i = lppd_i - pwaic_i;
 * lppd_sum, p_waic, elpd the sequential row-major sums (n major) of lppd_i, pwaic_i, e_i from +0.0;
 * waic = -2.0 * elpd; me = elpd / (double)(N M), Q the sequential sum of (e_i - me)^2,
 * se = sqrt((double)(N M) * (Q / (double)(N M - 1))) (NaN when N M = 1); site_elpd[n] the sequential sum of e over m
 * ascending, taxon_elpd[m] over n ascending; n_high the cells with pwaic_i > 0.4, the usual warning threshold.
 * Every output pointer is optional (NULL = skip); the scalars are always written.
 * SR_EINVAL: NULL ds, ab_pi, cd or out, n_sel <= 0, count < 1, T < 2, T >= 2^31, N outside 1..32767, M < 1, any c or
 * d that is read outside [-700, -2^-50] or NaN (inside, every term is finite and every p > 0); the session form also
 * for rows beyond the buffered records or a chain index out of range.  SR_EUNSUPPORTED: N M > 2^27, or a library
 * built without the device layer.  All reported before any kernel runs, the outputs untouched.  Device scratch is
 * bounded: chains and rows are taken in batches of at most SR_WAIC_SCRATCH bytes each (environment, default
 * 256 MiB) of per-chain partial sums and of table rows; the results do not depend on it. */
typedef struct {
  double *lppd, *ll_mean, *pwaic;        /* out: [N][M] each, NULL = skip */
  double *site_elpd, *taxon_elpd;        /* out: [N], [M], NULL = skip */
  double elpd, se, p_waic, lppd_sum, waic;
  int64_t n_high;
  double kernel_ms;
} sr_waic_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M and X */
int sr_waic(const sr_dataset *ds, const int16_t *ab_pi, const double *cd, int32_t manycd, int32_t n_sel,
            int32_t count, int32_t device, sr_waic_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order), on the session's
   stream; manycd is the session's; the session's state and records are left untouched */
int sr_session_waic(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                    sr_waic_out *out);
/* the reduction alone, on the host: scalars, site_elpd and taxon_elpd of out from lppd, pwaic [N][M] */
int sr_waic_reduce(int32_t N, int32_t M, const double *lppd, const double *pwaic, sr_waic_out *out);

/* ---- PSIS-LOO: leave-one-out cross-validation by Pareto-smoothed importance sampling, and the Pareto shape per
 * cell, over saved samples: defined to the bit ----
 * (an extension: the estimator Vehtari, Gelman & Gabry 2017 recommend over WAIC for the same quantity; the shape
 * estimate k says where it can be trusted.  For this model a cell with large k is an occurrence, or an absence,
 * whose likelihood is carried by a handful of samples: a presence far outside its taxon's range, or a gap inside
 * it.)  Inputs exactly as sr_waic: ds, ab_pi, cd, manycd, n_sel, count; T = n_sel * count, sample (k, r) and the cell
 * index 0..3 as there.  No flip input: a reflected chain changes no alive bit and no output.
 * Table, per sample (and per taxon when manycd), with this library's exp: p = {1.0 - ec, ed, 1.0 - ed, ec} as in
 * WAIC; r[j] = 1.0 / p[j], one IEEE division per table entry.
 * Per cell, sums over samples in WAIC's order (within chain k sequentially over r ascending from +0.0, then the
 * chain sums over k ascending from +0.0; no fma, no floating-point atomics): Sp the sum of p, Sr the sum of r;
 * lppd = log(Sp / (double)T), bit-equal to sr_waic's.
 * Tail length, in integers: n = min(T / 5, s), s the smallest integer with s * s >= 9 T (loo's min(0.2 T, 3 sqrt T)
 * with the rounding fixed).
 * Tail: y_1 <= ... <= y_n the n largest of the cell's T values r, as a sorted multiset; r_cut the (n+1)-th largest;
 * x_j = y_j - r_cut.  Nothing depends on which of several equal samples is taken.
 * Host tables, computed once per call with the C library's sqrt and log: m = 30 + isqrt(n);
 *   G_j = (1.0 - sqrt((double)m / ((double)j - 0.5))) / 3.0, j = 1..m;
 *   L_j = log(1.0 - ((double)j - 0.5) / (double)n), j = 1..n.
 * Fit (Zhang & Stephens 2009 as in loo 2.x gpdfit, log1p(-z) written log(1.0 - z)); every sum sequential ascending
 * from +0.0, every product rounded before it is added, nd = (double)n, exp and log this library's:
 *   xs = x_q, q = (n + 2) / 4 (integer division, 1-based);  theta_j = 1.0 / x_n + G_j / xs;
 *   k_j = (sum_i log(1.0 - theta_j * x_i)) / nd;  l_j = nd * ((log(-theta_j / k_j) - k_j) - 1.0);
 *   lmax = max_j l_j;  w_j = exp(l_j - lmax);  z = sum_j w_j;  th = sum_j theta_j * (w_j / z);
 *   k0 = (sum_i log(1.0 - th * x_i)) / nd;  sigma = -k0 / th;  k = (k0 * nd + 5.0) / (nd + 10.0) (the weakly
 *   informative prior of loo >= 2.0).
 * Unsmoothed cases: n < 5 (T < 25); !(xs > 0.0) (ties reaching the first quartile of the tail); any of l_j, th, k0,
 * sigma, k not finite.  Then pareto_k = +inf and elpd_loo = log((double)T / Sr), plain importance-sampling LOO.
 * Smoothed tail: s_j = r_cut + (sigma * (exp(-k * L_j) - 1.0)) / k, or r_cut - sigma * L_j if k == 0.0;
 *   wt_j = s_j if s_j < y_n, else y_n (loo's truncation at the largest raw ratio; it absorbs an overflowing exp);
 *   St = sum_j y_j, Sw = sum_j wt_j, Nn = sum_j wt_j / y_j, D = (Sr - St) + Sw;
 *   elpd_loo = log(((double)(T - n) + Nn) / D).
 * (A non-tail sample contributes weight r_t and weight x likelihood exactly 1: PSIS-LOO in the linear domain, with
 * no sort of the non-tail values.)
 * Pointwise, [N][M] f64, each optional: elpd_loo, pareto_k, lppd, p_loo_i = lppd_i - elpd_loo_i (formed on the host).
 * Reduction (plain C on the host; sr_loo_reduce runs it alone on given arrays): sr_waic_reduce's formulas with
 * e_i = elpd_loo_i: elpd, lppd_sum and p_loo the sequential row-major sums of e_i, lppd_i and lppd_i - e_i; se from me
 * and Q as there; looic = -2.0 * elpd; site_elpd [N], taxon_elpd [M]; n_k[4] the cells with k <= 0.5, 0.5 < k <= 0.7,
 * 0.7 < k <= 1, and k > 1 including +inf; tail_len = n (sr_loo and sr_session_loo only).
 * sr_loo_tail is the tail alone on the host, the source the device runs: y [n] ascending, r_cut, Sr -> *k, *elpd; it
 * sorts nothing.  sr_loo_tail_len(T) is n (0 for T outside 1..2^31-1).
 * SR_EINVAL as sr_waic, but the rate domain is [-600, -2^-50]: with it every r <= e^600 and every sum over T < 2^31
 * values is finite.  SR_EUNSUPPORTED: N M > 2^27; n > 4096 (T above about 1.86 M); a library built without the
 * device layer.  All reported before any kernel runs, the outputs untouched.  Device scratch is bounded by
 * SR_LOO_SCRATCH bytes (environment, default 256 MiB) each of per-chain partial sums, of table rows and of the cells'
 * n + 1 largest ratios (cells are taken in batches, each batch re-reads the rows); the results do not depend on it. */
typedef struct {
  double *elpd_loo, *pareto_k, *lppd, *p_loo_i;   /* out: [N][M] each, NULL = skip */
  double *site_elpd, *taxon_elpd;                 /* out: [N], [M], NULL = skip */
  double elpd, se, p_loo, lppd_sum, looic;
  int64_t n_k[4];
  int32_t tail_len;
  double kernel_ms;
  double phase_ms[3];                             /* kernel_ms by phase: the sums, the selection, the finish */
} sr_loo_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M and X */
int sr_loo(const sr_dataset *ds, const int16_t *ab_pi, const double *cd, int32_t manycd, int32_t n_sel, int32_t count,
           int32_t device, sr_loo_out *out);
/* the session's own records and rates in HBM, rows [first, first+count) of chains[] (selection order), on the
   session's stream; manycd is the session's; the session's state and records are left untouched */
int sr_session_loo(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                   sr_loo_out *out);
/* the reduction alone, on the host: scalars (not tail_len), n_k, site_elpd and taxon_elpd of out from [N][M] arrays */
int sr_loo_reduce(int32_t N, int32_t M, const double *lppd, const double *elpd_loo, const double *pareto_k,
                  sr_loo_out *out);
/* one cell's tail alone, on the host: SR_EINVAL for NULL k or elpd, T outside 1..2^31-1, n < 0, n >= T (n > 0), NULL y
   with n > 0; SR_EUNSUPPORTED for n > 4096 */
int sr_loo_tail(int64_t T, int32_t n, const double *y, double r_cut, double Sr, double *k, double *elpd);
int32_t sr_loo_tail_len(int64_t T);

/* ---- Posterior predictive checks over saved samples: exact integers, the replicates defined to the bit ----
 * (an extension: WAIC ranks the two rate models against each other; whether the preferred one is adequate -- one
 * false-zero rate for every taxon, no per-site sampling effort -- is a posterior predictive check on realised
 * discrepancies, Gelman, Meng & Stern 1996.)  For every saved sample and every replicate a 0/1 matrix is drawn from
 * the model at the sample's (pi, a, b, c, d); a discrepancy of the replicate is compared with the same discrepancy of
 * X under the same sample, and the comparisons are tallied.
 * Inputs: records are rows [a (M) | b (M) | pi (N)] int16 as above, pi[site] = position, chains in selection order;
 * sample (k, r), row r of chain k, has index t = k * count + r, T = n_sel * count.  The rates are exactly as sr_waic
 * takes them: manycd = 0: cd [n_sel][count][3], (c, d, loglik) rows, loglik not read; manycd != 0: cd
 * [n_sel][count][2M], c[M] then d[M].  seed is any uint64 (0 is a seed like any other); reps, 1..64, the number of
 * replicates per sample.  No flip input: reflecting a chain (a' = N - b, b' = N - a, pi' = N - 1 - pi) changes no
 * alive bit, no span and -- the counter holds the site, not the position -- no random word.
 * The replicate matrix: ec = exp(c), ed = exp(d) (this library's exp, bit for bit the C library's);
 *   thr_alive = (uint64)((1.0 - ed) * 4294967296.0), thr_dead = (uint64)(ec * 4294967296.0): both scalings are exact,
 *   both conversions truncate, the values reach 0 and 2^32, so they are compared in 64 bits;
 *   cell (n, m) is alive when a_m <= pi_n < b_m, compared in int32 (any int16 is legal);
 *   w = philox4x32_10(ctr = {n, m >> 2, t, rep}, key = {seed lo, seed hi ^ 0x50504331})[m & 3]: one call serves one
 *   site and four consecutive taxa; the key constant keeps these streams apart from a Philox-mode sampler's;
 *   x_rep = w < (alive ? thr_alive : thr_dead).
 * Discrepancies of a 0/1 matrix Y under sample t, int32, per taxon m, in this index order:
 *   0 ones   the sites with y = 1
 *   1 span   0 if ones = 0, else max pi_n - min pi_n + 1 over the sites with y = 1 (pi need not be a permutation)
 *   2 gaps   span - ones: the zeros between the first and the last occurrence
 *   3 f0     the sites alive with y = 0
 *   4 f1     the sites not alive with y = 1
 * per site n: rich, the sum of y[n][m] over m (for Y = X the row sum, the same under every sample); in total: each of
 * the five taxon statistics summed over m, int64.
 * Outputs, over the pairs = T * reps (sample, replicate) pairs; every pointer is optional (NULL = skip), the scalars
 * are always written:
 *   taxon_gt, taxon_eq [5][M] uint32        the pairs with rep > obs, with rep == obs
 *   taxon_sum_obs, taxon_sum_rep [5][M] int64  the sums over the same pairs (each sample's observed value counts
 *                                           reps times)
 *   site_gt, site_eq [N] uint32, site_sum_rep [N] int64   the same for rich
 *   total_obs [n_sel][count][5], total_rep [n_sel][count][reps][5] int64   the totals of every sample and replicate
 *   total_gt[5], total_eq[5]                the tallies of the totals; pairs; kernel_ms, the kernels' time
 * A posterior predictive p-value is (gt + 0.5 * eq) / pairs.
 * SR_EINVAL: NULL ds, ab_pi, cd or out, n_sel <= 0, count < 1, reps outside 1..64, T * reps >= 2^31, N outside
 * 1..32767, M < 1, any c or d that is read outside [-700, -2^-50] or NaN; the session form also for rows beyond the
 * buffered records or a chain index out of range.  SR_EUNSUPPORTED: N M > 2^27, or a library built without the device
 * layer.  All reported before any kernel runs, the outputs untouched.  Device scratch is bounded: the samples are
 * taken in batches of at most SR_PPC_SCRATCH bytes (environment, default 256 MiB) of row sums, totals and
 * thresholds; the results do not depend on it. */
typedef struct {
  uint32_t *taxon_gt, *taxon_eq;            /* out: [5][M], NULL = skip */
  int64_t *taxon_sum_obs, *taxon_sum_rep;   /* out: [5][M], NULL = skip */
  uint32_t *site_gt, *site_eq;              /* out: [N], NULL = skip */
  int64_t *site_sum_rep;                    /* out: [N], NULL = skip */
  int64_t *total_obs;                       /* out: [n_sel][count][5], NULL = skip */
  int64_t *total_rep;                       /* out: [n_sel][count][reps][5], NULL = skip */
  int64_t total_gt[5], total_eq[5];
  int64_t pairs;
  double kernel_ms;
} sr_ppc_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M and X */
int sr_ppc(const sr_dataset *ds, const int16_t *ab_pi, const double *cd, int32_t manycd, int32_t n_sel, int32_t count,
           uint64_t seed, int32_t reps, int32_t device, sr_ppc_out *out);
/* the session's own records and rates in HBM, rows [first, first+count) of chains[] (selection order), on the
   session's stream; manycd is the session's; the session's state and records are left untouched */
int sr_session_ppc(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count, uint64_t seed,
                   int32_t reps, sr_ppc_out *out);

/* ---- cell occupancy and the per-site, per-taxon error tallies over saved samples: exact counts ----
 * (an extension.  sr_posterior's alive, false_alive and false_ones reproduce the reference script's three occupancy
 * plots with their quirks -- the site's row index in place of its sampled position, a closed interval, an accumulator
 * that is never reset, a fixed divisor of 1000 -- so they are not the posterior probability that taxon m lived at
 * site n; these counts are.)  Joint functions of (pi, a, b) and X, which no per-column output can give.
 * Inputs: records are rows [a (M) | b (M) | pi (N)] int16 as above, pi[site] = position, chains in selection order;
 * T = n_sel * count samples; ds supplies N, M and X.  Cell (n, m) is alive in a sample when a_m <= pi_n < b_m,
 * compared in int32: any int16 value is legal, nothing wraps and nothing is "outside".  No rates and no flip input:
 * reflecting a chain (a' = N - b, b' = N - a, pi' = N - 1 - pi) changes no alive bit and therefore no output.
 * Per sample, with x = X[n][m] (non-zero counts as 1):
 *   for site n over the M taxa    alive_n  the taxa alive at the site
 *                                 f0_n     the taxa alive with x = 0 (false zeros, Lazarus gaps)
 *                                 f1_n     the taxa not alive with x = 1 (false ones)
 *   for taxon m over the N sites  alive_m, f0_m, f1_m likewise
 * Outputs, unsigned counts over the T samples; every pointer is optional (NULL = skip), a call only pays for what
 * it asks, and one that asks for nothing succeeds:
 *   alive [N][M]                                             the samples in which cell (n, m) is alive
 *   site_alive_hist, site_f0_hist, site_f1_hist [N][M+1]     entry [n][r]: the samples with alive_n (f0_n, f1_n) equal
 *                                                            to r; every row sums to T
 *   taxon_alive_hist, taxon_f0_hist, taxon_f1_hist [M][N+1]  the same per taxon; every row sums to T
 * (taxon_alive_hist is not sr_relations' dur_hist in general: it counts the sites inside the range, which equals
 * b - a when pi is a permutation of 0..N-1 and 0 <= a <= b <= N.)  kernel_ms, the kernels' time, is always written.
 * The results do not depend on the order of the adds.  No device scratch beyond the outputs and X is allocated.
 * SR_EINVAL: NULL ds, ab_pi or out, n_sel <= 0, count < 1, n_sel * count >= 2^31, N outside 1..32767, M < 1; the
 * session form also for rows beyond the buffered records or a chain index out of range.  SR_EUNSUPPORTED: N M > 2^27,
 * a requested histogram larger than 1 GiB (N (M+1) or M (N+1) > 2^28), or a library built without the device layer.
 * All reported before any device call, the outputs untouched. */
typedef struct {
  uint32_t *alive;                                             /* out: [N][M], NULL = skip */
  uint32_t *site_alive_hist, *site_f0_hist, *site_f1_hist;     /* out: [N][M+1] each, NULL = skip */
  uint32_t *taxon_alive_hist, *taxon_f0_hist, *taxon_f1_hist;  /* out: [M][N+1] each, NULL = skip */
  double kernel_ms;                                            /* out */
} sr_occ_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M and X */
int sr_occupancy(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count, int32_t device,
                 sr_occ_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order), on the session's
   stream; the session's state and records are left untouched */
int sr_session_occupancy(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                         sr_occ_out *out);

/* ---- Placement: where a row that was not in the run belongs in the seriation, every output defined to the bit ----
 * (an extension.)  A new or fragmentary locality comes as a faunal list; given a sample's ranges and rates its
 * likelihood at a position is a product over the taxa, and the posterior placement is the average over the samples
 * of that likelihood normalised over the positions.  Position p means "of the same age as whichever site sits at
 * position p" (co-location, not insertion between two sites); placing one of the run's own rows is in-sample.
 * Inputs: records, ds (N, M; X is not read), cd, manycd, n_sel, count exactly as sr_waic takes them: rows
 * [a (M) | b (M) | pi (N)] int16, chains in selection order, the rates on the log scale, every c and d that is read
 * in [-700, -2^-50]; T = n_sel * count samples (one is enough).  Y [Q][M] uint8: 0 absent, 1 present, 2 not assessed.
 * flip [n_sel] or NULL: a flagged chain's rows are reflected first, in int32, as sr_marginals reflects them:
 * a' = N - b, b' = N - a, pi' = N - 1 - pi; everything below is defined on the reflected rows.
 * Term table, per sample (and per taxon when manycd), WAIC's l[4] = {log(1.0 - exp(c)), d, log(1.0 - exp(d)), c}
 * with this library's exp and log (bit for bit the C library's).
 * Profile of sample (k, r), query q, candidate position p in 0..N-1: L[p] = the sequential sum from +0.0, over m
 * ascending, of l[idx] of taxon m, idx WAIC's index with alive = a_m <= p < b_m (compared in int32: any int16 is
 * legal) and y = Y[q][m]: 0 for (y = 0, not alive), 1 for (y = 0, alive), 2 for (y = 1, alive), 3 for (y = 1, not
 * alive).  A cell with y = 2 contributes +0.0, which equals skipping it (no partial sum is ever -0.0: each starts at
 * +0.0 and every term is <= +0.0).
 * Normalisation: mx = max_p L[p]; e[p] = exp(L[p] - mx) over the whole domain of exp (subnormal results and
 * underflow to 0.0 are legal and are the C library's); z_j, j in 0..63, the sequential sum from +0.0 of e[p] over
 * p = j, j + 64, j + 128, ... < N; Z the sequential sum from +0.0 of z_0 ... z_63, j ascending (Z >= 1 always);
 * w[p] = e[p] / Z; lse = mx + log(Z).
 * Accumulation, in WAIC's order: within chain k sequentially over r ascending from +0.0, then the chain sums
 * sequentially over k ascending from +0.0; no fma outside exp and log, no floating-point atomic:
 *   Spos[q][p] += w[p];   Ssite[q][n] += (0 <= pi'_n < N ? w[pi'_n] : +0.0).
 * Outputs; every array is optional (NULL = skip), and a call that asks for nothing succeeds:
 *   pos  [Q][N] = Spos / (double)T      the posterior probability that query q is of the age of position p
 *   site [Q][N] = Ssite / (double)T     ... of the age of site n; reflecting a chain moves each e to the mirrored
 *                                       position, so site depends on the flags only through the rounding of Z
 *   lse  [n_sel][count][Q]              each sample's log of the sum over positions of the query's likelihood
 *   lpd  [Q], in plain C on the host after the kernels: mxx the maximum of the query's lse, s the sequential sum
 *        from +0.0 over (k major, r) of exp(lse - mxx), lpd = mxx + log(s / (double)T) - log((double)N): the log
 *        predictive density of the query row under a uniform prior over the positions, comparable between queries
 *        with the same assessed taxa
 *   kernel_ms, the kernels' time, is always written.
 * Device scratch is bounded as WAIC's is: chains and rows are taken in batches of at most SR_PLACE_SCRATCH bytes
 * (read from the environment at each call, 256 MiB by default, one chain and one row at the least); the results do
 * not depend on it.
 * SR_EINVAL: NULL ds, ds->X, ab_pi, cd, Y or out, Q < 1, a Y value above 2, T < 1 or T >= 2^31, N outside 1..32767,
 * M < 1, a rate outside the domain or NaN; the session form also for rows beyond the buffered records or a chain
 * index out of range.  SR_EUNSUPPORTED: Q N > 2^27, or a library built without the device layer.  All reported
 * before the device is touched, the outputs untouched. */
typedef struct {
  const uint8_t *flip;   /* in: [n_sel], non-zero = reflect that chain's rows first; NULL = none */
  double *pos;           /* out: [Q][N], NULL = skip */
  double *site;          /* out: [Q][N], NULL = skip */
  double *lse;           /* out: [n_sel][count][Q], NULL = skip */
  double *lpd;           /* out: [Q], NULL = skip */
  double kernel_ms;      /* out */
} sr_place_out;

/* records and rates in host memory, as sr_waic takes them; Y [Q][M] */
int sr_placement(const sr_dataset *ds, const int16_t *ab_pi, const double *cd, int32_t manycd, int32_t n_sel,
                 int32_t count, const uint8_t *Y, int32_t Q, int32_t device, sr_place_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order), shared or per-taxon
   rates as the session samples them (fetched as sr_session_waic fetches them); the session's state and records are
   left untouched */
int sr_session_placement(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                         const uint8_t *Y, int32_t Q, sr_place_out *out);

/* ---- chain agreement: pairwise order distances between chains and mode clustering: exact integers ----
 * (an extension: the reference's choose_chains ranks chains by mean -loglik and never asks whether they sampled the
 * same order.)  Records are rows [a (M) | b (M) | pi (N)] int16 as above, pi[site] = position; only the pi part is
 * read.  Chains in selection order, chain k has `count` rows.  Any int16 value is legal: values are only compared,
 * so nothing wraps and nothing is "outside".
 *   pair_counts [n_sel][N][N] uint32   O_k[i][j]: the number of chain k's rows with pi_i < pi_j, all ordered i != j;
 *                                      the diagonal is 0; for permutation rows O_k[i][j] + O_k[j][i] = count
 *   dist [n_sel][n_sel] int64          dist[k][l] = sum over i < j of |O_k[i][j] - O_l[i][j]|
 *   dist_mirror [n_sel][n_sel] int64   dist_mirror[k][l] = sum over i < j of |O_k[i][j] - O_l[j][i]|: the distance
 *                                      from chain k to the reflection of chain l (pi' = N - 1 - pi); the diagonal is
 *                                      defined: how far a chain is from its own mirror image
 *   scale = count * N (N - 1) / 2      the largest possible value: dist / scale lies in [0, 1]
 * Exact integers: the result does not depend on the order of the adds.  count < 2^31 and fewer than 2^29 pairs, so
 * every sum is below 2^60.  N = 1 is valid: no pairs, every distance 0, scale 0.  Every output pointer is optional
 * (NULL = skip); scale and kernel_ms are always written.
 * sr_agreement_distances is the reduction alone, from pair counts in host memory (any uint32 values; e.g. matrices
 * gathered from several GPUs).
 * SR_EINVAL: NULL ds, ab_pi, out or pair_counts (the input of sr_agreement_distances), n_sel <= 0, count < 1,
 * n_sel * count >= 2^31, N outside 1..32767; the session form also for rows beyond the buffered records or a chain
 * index out of range.  SR_EUNSUPPORTED: n_sel > 4096, a requested pair_counts larger than 2^28 entries, or a library
 * built without the device layer.  All reported before any device call, the outputs untouched.  Device scratch is
 * bounded: the site pairs are taken in bands of at most SR_AGREE_SCRATCH bytes of per-chain counts (environment,
 * read at each call, default 256 MiB; one row of 64-site tiles at least); the results do not depend on it.
 *
 * Mode clustering (sr_agreement_modes: host only, plain C, no GPU) over n chains:
 *   1. for k < l, e = min(dist[k][l], dist_mirror[k][l]); only the upper triangle is read;
 *   2. k and l are linked iff (double)e <= threshold * (double)scale: one f64 multiply and one compare;
 *   3. modes are the connected components, numbered from 0 in ascending order of their smallest chain index;
 *   4. flips: the smallest chain of a component has flip 0; breadth-first from it (a first-in first-out queue, the
 *      neighbours of each entry tried in ascending chain index), a chain l first reached from k gets
 *      flip[l] = flip[k] ^ (dist_mirror[min(k,l)][max(k,l)] < dist[min(k,l)][max(k,l)]);
 *   5. medoid[g]: the member of mode g with the smallest sum of e to the other members, ties to the lowest index;
 *   6. size[g]: the number of members.
 * mode [n] is required; flip [n], medoid [n], size [n] (the first n_modes entries are written) and n_modes are
 * optional.  SR_EINVAL: threshold outside [0, 1] or NaN, scale < 0, n <= 0, NULL dist, dist_mirror or mode. */
typedef struct {
  uint32_t *pair_counts;          /* out: [n_sel][N][N], NULL = skip */
  int64_t *dist, *dist_mirror;    /* out: [n_sel][n_sel], NULL = skip */
  int64_t scale;                  /* out */
  double kernel_ms;               /* out */
} sr_agree_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M */
int sr_agreement(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count, int32_t device,
                 sr_agree_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order), on the session's
   stream; the session's state and records are left untouched */
int sr_session_agreement(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                         sr_agree_out *out);
/* the reduction alone, from pair counts in host memory (any uint32 values): e.g. matrices gathered from several GPUs */
int sr_agreement_distances(int32_t N, int32_t n_sel, const uint32_t *pair_counts, int32_t device, int64_t *dist,
                           int64_t *dist_mirror, double *kernel_ms);
/* host only */
int sr_agreement_modes(int32_t n, const int64_t *dist, const int64_t *dist_mirror, int64_t scale, double threshold,
                       int32_t *mode, uint8_t *flip, int32_t *medoid, int32_t *size, int32_t *n_modes);

/* ---- the central sampled state: the saved record with the smallest posterior expected loss: exact integers ----
 * (an extension: every other summary is marginal -- a vector of means is not a permutation and per-column medians
 * need not satisfy a <= b -- while the medoid of the draws is one coherent (pi, a, b) the sampler produced.)
 * Records are rows [a (M) | b (M) | pi (N)] int16 as above, pi[site] = position, n_sel chains (selection order) of
 * `count` rows, T = n_sel * count.  flip [n_sel] (NULL = none) reflects a flagged chain's rows first, exactly as
 * sr_marginals does: a' = N - b, b' = N - a, pi' = N - 1 - pi.  All arithmetic on record values is int32: any int16
 * input is legal and nothing wraps.
 *   pair_counts [N][N] uint32      C[i][j]: the number of the T rows with pi'(i) < pi'(j), pooled over the chains;
 *                                  the diagonal is 0; both orders are counted, not derived (host records may tie)
 *   order_loss [n_sel][count] int64  of row r: the sum over i < j of [pi'_r(i) < pi'_r(j)] C[j][i] +
 *                                  [pi'_r(i) > pi'_r(j)] C[i][j]: the (row, pair) combinations that strictly order a
 *                                  pair opposite to r; a tie in r adds 0; for permutation rows the sum of r's
 *                                  Kendall-tau distances to all T rows.  Fewer than 2^29 pairs and counts below 2^32:
 *                                  below 2^61
 *   limit_loss [n_sel][count] int64  of row r: the sum over taxa m and all T rows s of |A_r[m] - A_s[m]| +
 *                                  |B_r[m] - B_s[m]|, A = clamp(a', 0, N), B = clamp(b', 0, N): defined for any input
 *   best [n_sel] int32             per chain k the row t that minimises (order_loss, limit_loss, t) within the chain
 *   central_chain, central_row     the (k, t) that minimises (order_loss, limit_loss, k, t) lexicographically: k in
 *                                  selection order, t within the rows given
 *   state [2M+N] int32             the central row as [a | b | pi], reflected if its chain is flagged, not clamped
 *   scale = T N (N - 1) / 2        as sr_agree_out.scale with T rows: order_loss / scale is the expected normalised
 *                                  Kendall distance from the row to a posterior draw
 * Exact integers: the result does not depend on the order of the adds.  order_loss, limit_loss, pair_counts, best and
 * state are optional (NULL = skip); the scalars are always written.
 * sr_order_loss is the order loss alone, of the given rows against counts the caller holds (against [N][N], any
 * uint32 values, read as C above; e.g. the pooled counts of another mode, or sr_agreement's per-chain pair_counts
 * summed), as sr_agreement_distances is to sr_agreement.
 * SR_EINVAL: a NULL ds, ab_pi, out (sr_order_loss: against, order_loss), n_sel <= 0, count < 1, T >= 2^31, N outside
 * 1..32767, M < 1, 2 M N T >= 2^62 (the limit loss would not fit; not for sr_order_loss); the session form also for
 * rows beyond the buffered records or a chain index out of range.  SR_EUNSUPPORTED: a requested pair_counts larger
 * than 1 GiB (N > 16384), or a library built without the device layer.  All reported before any device call, the
 * outputs untouched.  Device scratch is bounded: the site pairs are taken in bands of at most SR_CENTRAL_SCRATCH
 * bytes of counts (environment, read at each call, default 256 MiB; one row of 64-site tiles at least) and the limit
 * columns in batches whose histogram and table stay within the same bound (one column at least); the results do not
 * depend on it. */
typedef struct {
  const uint8_t *flip;           /* in: [n_sel] or NULL */
  int64_t *order_loss;           /* out: [n_sel][count], NULL = skip */
  int64_t *limit_loss;           /* out: [n_sel][count] */
  uint32_t *pair_counts;         /* out: [N][N] pooled, oriented */
  int32_t *best;                 /* out: [n_sel] */
  int32_t *state;                /* out: [2M+N] */
  int32_t central_chain, central_row;   /* out: selection order, row within the view */
  int64_t scale;                 /* out */
  double kernel_ms;              /* out */
} sr_central_out;

/* records in host memory: ab_pi [n_sel][count][2M+N] int16; ds supplies N, M */
int sr_central(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count, int32_t device,
               sr_central_out *out);
/* the session's own records in HBM, rows [first, first+count) of chains[] (selection order), on the session's
   stream; the session's state and records are left untouched */
int sr_session_central(sr_session *s, const int32_t *chains, int32_t n_sel, int32_t first, int32_t count,
                       sr_central_out *out);
/* the order loss alone, against any counts: against [N][N] any uint32, order_loss [n_sel][count]; kernel_ms optional */
int sr_order_loss(const sr_dataset *ds, const int16_t *ab_pi, int32_t n_sel, int32_t count, const uint8_t *flip,
                  const uint32_t *against, int32_t device, int64_t *order_loss, double *kernel_ms);

const char *sr_strerror(int code);
int sr_device_count(void);
const char *sr_version(void);

#ifdef __cplusplus
}
#endif
#endif
