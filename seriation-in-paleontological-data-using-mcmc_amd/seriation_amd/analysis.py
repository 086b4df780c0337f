"""Posterior summaries over the selected chains (script.py:102-429).

Scalar statistics (E[c], E[d], CORRMN: per-chain sums of ~1000 values) are host Python, in
two forms with identical results:
  * file form -- reads Chains/chain_NN/chain_data.csv exactly as script.py does (token
    positions, the hard-coded /1000), for drop-in use after `run_all_chains`;
  * record form -- the same operation sequence on in-memory records (c, d in log scale as
    the sampler keeps them; pi as int arrays), as produced by `run_chains(keep_records=True)`
    or gathered across ranks (dist.gather_selected_records), without writing the files.

The per-sample matrix accumulations (pair-order matrix, taxon alive / false-alive /
false-ones probabilities, E[pi], E[a]) run on the GPU (csrc/sr_post.hip through
sr_posterior / sr_session_posterior), bit for bit as the script computes them; only the
final argsort reorderings are host numpy.  There is no CPU fallback for them.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib as L
from .core import _check


def _chain_lines(root, chain):
    with open(os.path.join(root, "Chains", "chain_%02d" % chain, "chain_data.csv")) as fh:
        return fh.readlines()


def compute_exp_cd(chains, chains_selected, root="."):
    """script.py:100-124: mean over chains of (sum over samples of the first c / d token)/1000,
    divided by chains_selected."""
    c_chain = d_chain = 0.0
    for chain in chains:
        c_sum = d_sum = 0.0
        for line in _chain_lines(root, chain):
            f = line.split(",")
            c_sum += float(f[3].split(" ")[0].strip())
            d_sum += float(f[4].split(" ")[0].strip())
        c_chain += c_sum / 1000
        d_chain += d_sum / 1000
    return c_chain / chains_selected, d_chain / chains_selected


def _pearson_identity(pi):
    """script.py:147: scipy.stats.pearsonr(pi_chain, np.arange(0, sites))[0] -- the reference's
    own call (scipy of this image; the reference pinned scipy 1.4.1, whose formula may differ
    from it in the last bits)."""
    from scipy.stats import pearsonr
    return float(pearsonr(pi, np.arange(0, len(pi)))[0])


def compute_exp_ages(chains, chains_selected, sites, root="."):
    """script.py:127-152 (CORRMN): mean over chains of (sum over samples of
    pearson(pi, 0..N-1))/1000, divided by chains_selected."""
    total = 0.0
    for chain in chains:
        s = 0.0
        for line in _chain_lines(root, chain):
            pi = [int(t.strip()) for t in line.split(",")[2].split(" ")[:sites]]
            s += _pearson_identity(pi)
        total += s / 1000
    return total / chains_selected


# ---------------------------------------------------------------- record forms
# The same operation sequences on in-memory records (c, d in log scale as the sampler keeps them;
# pi as int rows), as produced by run_chains(keep_records=True) or gathered across ranks
# (dist.gather_selected_records): each c / d is the value the file form reads back, i.e.
# mcmc_save_chain's "%.14f" of the C library's exp (mcmc.c:82-85), summed sequentially; so the
# record forms equal the file forms bit for bit (tests/test_analysis.py).
def _token(v):
    return float("%.14f" % math.exp(v))


def exp_cd_from_records(cdl_per_chain, chains_selected=None):
    """cdl_per_chain: iterable of [ts, 3] arrays (c, d, loglik) -> (E[c], E[d]) as
    compute_exp_cd; chains_selected defaults to the number of chains given."""
    cdl_per_chain = list(cdl_per_chain)
    c_chain = d_chain = 0.0
    for r in cdl_per_chain:
        c_sum = d_sum = 0.0
        for c, d, _ll in np.asarray(r, np.float64).tolist():
            c_sum += _token(c)
            d_sum += _token(d)
        c_chain += c_sum / 1000
        d_chain += d_sum / 1000
    n = len(cdl_per_chain) if chains_selected is None else chains_selected
    return c_chain / n, d_chain / n


def corr_mn_from_records(pi_per_chain, chains_selected=None):
    """pi_per_chain: iterable of [ts, N] int arrays -> CORRMN as compute_exp_ages."""
    pi_per_chain = list(pi_per_chain)
    tot = 0.0
    for P in pi_per_chain:
        s = 0.0
        for p in np.asarray(P).tolist():
            s += _pearson_identity(p)
        tot += s / 1000
    n = len(pi_per_chain) if chains_selected is None else chains_selected
    return tot / n


# ---------------------------------------------------------------- GPU posterior summaries
KINDS = ("pair_order", "alive", "false_alive", "false_ones", "exp_pi", "exp_a")


def _shape(kind, N, M):
    return {"pair_order": (N, N), "alive": (N, M), "false_alive": (N, M), "false_ones": (N, M),
            "exp_pi": (N,), "exp_a": (M,)}[kind]


def _outs(kinds, N, M):
    arrs = {k: np.zeros(_shape(k, N, M)) for k in kinds}
    out = L.sr_posterior_out()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return out, arrs


def posterior_from_records(dataset, ab_pi, chains_selected, kinds=KINDS, device=0):
    """sr_posterior: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order)
    -> {kind: array}; dataset supplies N, M and X (false_ones)."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    out, arrs = _outs(kinds, dataset.N, dataset.M)
    _check(L.lib().sr_posterior(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                rec.shape[0], rec.shape[1], int(chains_selected), device, ctypes.byref(out)),
           "sr_posterior")
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def posterior_from_session(session, chains, chains_selected, first=0, count=None, kinds=KINDS):
    """sr_session_posterior: the same summaries over a session's records still in HBM.
    chains: session chain indices in selection order."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs = _outs(kinds, session.ds.N, session.ds.M)
    _check(L.lib().sr_session_posterior(session.h, ch, len(chains), first, count, int(chains_selected),
                                        ctypes.byref(out)), "sr_session_posterior")
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def session_records(session):
    return L.lib().sr_session_records(session.h)


# ---------------------------------------------------------------- convergence diagnostics
# Split-R-hat and effective sample size per site position, taxon limit, c, d and loglik (definitions:
# include/seriation.h).  The lagged integer moments of the records come from the GPU (csrc/sr_diag.hip), exact in
# int64; the f64 tail is the library's host code.  There is no CPU fallback for the moments.
_I64P = ctypes.POINTER(ctypes.c_int64)
_DBLP = ctypes.POINTER(ctypes.c_double)


def _diag_lags(count, max_lag):
    h = count // 2
    return h, (h - 1 if max_lag == 0 else max_lag)


def _diag_views(flat, N, M):
    return {"a": flat[:M], "b": flat[M:2 * M], "pi": flat[2 * M:2 * M + N],
            "c": flat[2 * M + N], "d": flat[2 * M + N + 1], "loglik": flat[2 * M + N + 2]}


def _diag_outs(N, M, n_sel, count, max_lag, moments):
    Q = 2 * M + N + 3
    flat = {"rhat": np.zeros(Q), "ess": np.zeros(Q), "cut_lag": np.zeros(Q, np.int32)}
    out = L.sr_diag_out()
    out.max_lag = int(max_lag)
    out.rhat = flat["rhat"].ctypes.data_as(_DBLP)
    out.ess = flat["ess"].ctypes.data_as(_DBLP)
    out.cut_lag = flat["cut_lag"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    raw = {}
    # (invalid count / max_lag: no moment buffers; the library refuses the call with SR_EINVAL)
    if moments and count >= 4 and 0 <= max_lag < count // 2 and n_sel > 0:
        h, lags = _diag_lags(count, max_lag)
        W, S = 2 * M + N, 2 * n_sel
        raw = {"P": np.zeros((S, lags + 1, W), np.int64), "F": np.zeros((S, lags + 1, W), np.int64),
               "B": np.zeros((S, lags + 1, W), np.int64), "S1": np.zeros((S, W), np.int64)}
        for k, a in raw.items():
            setattr(out, k, a.ctypes.data_as(_I64P))
    return out, flat, raw


def _diag_result(out, flat, raw, N, M):
    res = {k: _diag_views(v, N, M) for k, v in flat.items()}
    res["kernel_ms"] = out.kernel_ms
    res.update(raw)
    return res


def diagnostics_from_records(dataset, ab_pi, cdl=None, max_lag=0, device=0, moments=False):
    """sr_diagnostics: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order), cdl
    [n_sel][count][3] (c, d, loglik; None: their entries are NaN) -> {"rhat", "ess", "cut_lag": {"a": [M], "b": [M],
    "pi": [N], "c", "d", "loglik"}, "kernel_ms"}; moments=True adds the raw int64 moments "P", "F", "B"
    [2 n_sel][L+1][2M+N] and "S1" [2 n_sel][2M+N]."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    cd = None
    if cdl is not None:
        cd = np.ascontiguousarray(cdl, dtype=np.float64)
        assert cd.shape == (n_sel, count, 3)
    out, flat, raw = _diag_outs(dataset.N, dataset.M, n_sel, count, max_lag, moments)
    _check(L.lib().sr_diagnostics(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                  cd.ctypes.data_as(_DBLP) if cd is not None else None, n_sel, count, device,
                                  ctypes.byref(out)), "sr_diagnostics")
    return _diag_result(out, flat, raw, dataset.N, dataset.M)


def diagnostics_from_session(session, chains, first=0, count=None, max_lag=0, moments=False):
    """sr_session_diagnostics: the same over a session's records still in HBM, rows [first, first + count) of
    chains (session chain indices in selection order)."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, flat, raw = _diag_outs(session.ds.N, session.ds.M, len(chains), count, max_lag, moments)
    _check(L.lib().sr_session_diagnostics(session.h, ch, len(chains), first, count, ctypes.byref(out)),
           "sr_session_diagnostics")
    return _diag_result(out, flat, raw, session.ds.N, session.ds.M)


def diag_reduce(P, F, B, S1, count, max_lag=0, cdl=None):
    """sr_diag_reduce (host only, no GPU): moments P, F, B [S][L+1][W], S1 [S][W] of S = 2 n_sel sequences of
    count // 2 rows (+ optional scalar traces cdl [n_sel][count][3]) -> (rhat, ess, cut_lag), each [W + 3]."""
    P, F, B, S1 = (np.ascontiguousarray(x, dtype=np.int64) for x in (P, F, B, S1))
    S, W = S1.shape
    h, lags = _diag_lags(count, max_lag)
    assert S % 2 == 0 and P.shape == F.shape == B.shape == (S, lags + 1, W)
    cd = None
    if cdl is not None:
        cd = np.ascontiguousarray(cdl, dtype=np.float64)
        assert cd.shape == (S // 2, count, 3)
    rhat, ess, cut = np.zeros(W + 3), np.zeros(W + 3), np.zeros(W + 3, np.int32)
    _check(L.lib().sr_diag_reduce(W, S // 2, count, int(max_lag), P.ctypes.data_as(_I64P), F.ctypes.data_as(_I64P),
                                  B.ctypes.data_as(_I64P), S1.ctypes.data_as(_I64P),
                                  cd.ctypes.data_as(_DBLP) if cd is not None else None, rhat.ctypes.data_as(_DBLP),
                                  ess.ctypes.data_as(_DBLP), cut.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
           "sr_diag_reduce")
    return rhat, ess, cut


# ---------------------------------------------------------------- posterior marginals
# Where each site and each taxon limit lies, and how sure: the exact histogram of every record column over the
# selected chains, and the quantiles, mode and mean read off it (definitions: include/seriation.h).  Histograms and
# summaries come from the GPU (csrc/sr_marg.hip); there is no CPU fallback.  Chains of a dataset without hard sites
# may settle in mirrored orders: orient them first (chain_orientation) or the pooled numbers mean nothing.
PROBS = (0.025, 0.5, 0.975)


def _marg_views(flat, N, M):
    """[..., 2M+N] -> views of the a, b and pi columns."""
    return {"a": flat[..., :M], "b": flat[..., M:2 * M], "pi": flat[..., 2 * M:2 * M + N]}


def _marg_outs(N, M, n_sel, probs, flips, hist):
    W = 2 * M + N
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    n_sel = max(int(n_sel), 0)
    flat = {"quant": np.zeros((len(p), W), np.int32), "mode": np.zeros(W, np.int32), "mean": np.zeros(W),
            "outside": np.zeros(W, np.uint32)}
    pi_sum = np.zeros((n_sel, N), np.int64)
    out = L.sr_marg_out()
    keep = [p, pi_sum]   # the buffers the struct points into
    if flips is not None:
        f = np.ascontiguousarray(np.asarray(flips) != 0, dtype=np.uint8)
        assert f.shape == (n_sel,)
        out.flip = f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        keep.append(f)
    out.probs = p.ctypes.data_as(_DBLP)
    out.n_probs = len(p)
    out.quant = flat["quant"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.mode = flat["mode"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.mean = flat["mean"].ctypes.data_as(_DBLP)
    out.outside = flat["outside"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    out.pi_sum = pi_sum.ctypes.data_as(_I64P)
    h = None
    if hist:
        h = np.zeros((W, N + 1), np.uint32)
        out.hist = h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    return out, flat, pi_sum, h, keep


def _marg_result(out, flat, pi_sum, h, N, M):
    res = {k: _marg_views(v, N, M) for k, v in flat.items()}
    res["pi_sum"] = pi_sum
    res["kernel_ms"] = out.kernel_ms
    if h is not None:
        res["hist"] = h
    return res


def marginals_from_records(dataset, ab_pi, probs=PROBS, flips=None, hist=False, device=0):
    """sr_marginals: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order) -> {"quant": {"a":
    [Q][M], "b": [Q][M], "pi": [Q][N]} (one row per probability), "mode", "mean", "outside": {"a": [M], "b": [M],
    "pi": [N]}, "pi_sum": [n_sel][N] (per-chain sums of the raw pi columns), "kernel_ms"}; hist=True adds "hist"
    [2M+N][N+1] uint32.  flips [n_sel]: chains whose rows are reflected before counting."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    out, flat, pi_sum, h, _keep = _marg_outs(dataset.N, dataset.M, n_sel, probs, flips, hist)
    _check(L.lib().sr_marginals(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel,
                                count, device, ctypes.byref(out)), "sr_marginals")
    return _marg_result(out, flat, pi_sum, h, dataset.N, dataset.M)


def marginals_from_session(session, chains, first=0, count=None, probs=PROBS, flips=None, hist=False):
    """sr_session_marginals: the same over a session's records still in HBM, rows [first, first + count) of
    chains (session chain indices in selection order)."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, flat, pi_sum, h, _keep = _marg_outs(session.ds.N, session.ds.M, len(chains), probs, flips, hist)
    _check(L.lib().sr_session_marginals(session.h, ch, len(chains), first, count, ctypes.byref(out)),
           "sr_session_marginals")
    return _marg_result(out, flat, pi_sum, h, session.ds.N, session.ds.M)


def chain_orientation(pi_sum):
    """pi_sum [n_sel][N] (marginals' per-chain sums of the pi columns) -> uint8 [n_sel]: 1 for a chain whose order
    runs against chain 0's, i.e. whose Pearson correlation with pi_sum[0] is negative (zero or undefined: 0).  The
    sign is that of n sum(xy) - sum(x) sum(y), taken in exact integers.  Intended use: one marginals call for
    pi_sum, then one with flips=chain_orientation(pi_sum)."""
    rows = [[int(v) for v in r] for r in np.asarray(pi_sum).tolist()]
    out = np.zeros(len(rows), np.uint8)
    if not rows:
        return out
    x, n = rows[0], len(rows[0])
    sx = sum(x)
    for k, y in enumerate(rows):
        cov = n * sum(a * b for a, b in zip(x, y)) - sx * sum(y)
        out[k] = 1 if cov < 0 else 0
    return out


# ---------------------------------------------------------------- taxon-pair relations and the diversity curve
# Which taxon came first, which pairs coexisted, how long each lasted and how many were alive at each position:
# joint functions of the limits, counted exactly over the selected chains' samples (definitions:
# include/seriation.h).  The counts come from the GPU (csrc/sr_rel.hip); there is no CPU fallback.  Orient mirrored
# chains first, as for the marginals.
REL_KINDS = ("orig_before", "ext_before", "precedes", "overlap", "dur_hist", "dur_outside", "rich_hist")


def _rel_outs(N, M, n_sel, flips, kinds):
    shapes = {"orig_before": (M, M), "ext_before": (M, M), "precedes": (M, M), "overlap": (M, M),
              "dur_hist": (M, N + 1), "dur_outside": (M,), "rich_hist": (N, M + 1)}
    arrs = {k: np.zeros(shapes[k], np.uint32) for k in kinds}
    out = L.sr_rel_out()
    keep = []   # the buffers the struct points into
    if flips is not None:
        f = np.ascontiguousarray(np.asarray(flips) != 0, dtype=np.uint8)
        assert f.shape == (max(int(n_sel), 0),)
        out.flip = f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        keep.append(f)
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return out, arrs, keep


def relations_from_records(dataset, ab_pi, flips=None, kinds=REL_KINDS, device=0):
    """sr_relations: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order) -> {kind: uint32 array}
    for the requested kinds ("orig_before", "ext_before", "precedes", "overlap": [M][M]; "dur_hist": [M][N+1];
    "dur_outside": [M]; "rich_hist": [N][M+1]) plus "total" (the number of samples) and "kernel_ms".  flips [n_sel]:
    chains whose limits are reflected before counting."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    out, arrs, _keep = _rel_outs(dataset.N, dataset.M, n_sel, flips, kinds)
    _check(L.lib().sr_relations(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel,
                                count, device, ctypes.byref(out)), "sr_relations")
    arrs["total"] = n_sel * count
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def relations_from_session(session, chains, first=0, count=None, flips=None, kinds=REL_KINDS):
    """sr_session_relations: the same over a session's records still in HBM, rows [first, first + count) of
    chains (session chain indices in selection order)."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs, _keep = _rel_outs(session.ds.N, session.ds.M, len(chains), flips, kinds)
    _check(L.lib().sr_session_relations(session.h, ch, len(chains), first, count, ctypes.byref(out)),
           "sr_session_relations")
    arrs["total"] = len(chains) * count
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def diversity_curve(rich_hist, probs=PROBS):
    """rich_hist [N][M+1] (relations' exact histogram of the number of taxa alive at each position) -> {"mean": [N]
    f64, "quant": [len(probs)][N] int32}, on the host, by the marginals' rules: the quantile of probability p is the
    richness at which the cumulative count first reaches the rank k = clamp(ceil(p * T), 1, T), T the position's
    total; the mean is an exact int64 numerator divided once in f64."""
    h = np.asarray(rich_hist).astype(np.int64)
    assert h.ndim == 2
    T = h.sum(axis=1)
    cum = np.cumsum(h, axis=1)
    quant = np.zeros((len(probs), h.shape[0]), np.int32)
    for q, p in enumerate(probs):
        k = np.clip(np.ceil(float(p) * T.astype(np.float64)).astype(np.int64), 1, T)
        quant[q] = np.argmax(cum >= k[:, None], axis=1)
    num = (h * np.arange(h.shape[1], dtype=np.int64)[None, :]).sum(axis=1)
    return {"mean": num.astype(np.float64) / T.astype(np.float64), "quant": quant}


# ---------------------------------------------------------------- WAIC and the pointwise model fit
# Does the model fit, and which of the two models -- error rates shared by all taxa, or per-taxon rates (manycd) --
# fits better: the widely applicable information criterion over the selected chains' samples, every output defined
# to the bit (definitions: include/seriation.h).  The N M T reduction runs on the GPU (csrc/sr_waic.hip); there is no
# CPU fallback.  No orientation is needed: a reflected chain gives the same alive bits.
_WAIC_SCALARS = ("elpd", "se", "p_waic", "lppd_sum", "waic")


def _waic_outs(N, M, pointwise):
    arrs = {"site_elpd": np.zeros(N), "taxon_elpd": np.zeros(M)}
    if pointwise:
        arrs.update({k: np.zeros((N, M)) for k in ("lppd", "ll_mean", "pwaic")})
    out = L.sr_waic_out()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(_DBLP))
    return out, arrs


def _waic_result(out, arrs, total, pointwise):
    res = {k: getattr(out, k) for k in _WAIC_SCALARS}
    res["elpd_waic"] = res.pop("elpd")   # "elpd" names the pointwise array below
    res["n_high"] = int(out.n_high)
    res["site_elpd"], res["taxon_elpd"] = arrs["site_elpd"], arrs["taxon_elpd"]
    res["total"] = total
    res["kernel_ms"] = out.kernel_ms
    if pointwise:
        for k in ("lppd", "ll_mean", "pwaic"):
            res[k] = arrs[k]
        res["elpd"] = arrs["lppd"] - arrs["pwaic"]
    return res


def waic_from_records(dataset, ab_pi, cd, manycd=False, pointwise=True, device=0):
    """sr_waic: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order) and the rates on the log
    scale, cd [n_sel][count][3] ((c, d, loglik) rows as Session.fetch_records gives them) or, manycd, [n_sel][count][2M]
    (c[M] then d[M], as Session.fetch_cd_vectors) -> {"elpd_waic", "se", "p_waic", "lppd_sum", "waic" (floats),
    "n_high", "site_elpd" [N], "taxon_elpd" [M], "total" (the number of samples), "kernel_ms"}; pointwise adds
    "lppd", "ll_mean", "pwaic" and "elpd" = lppd - pwaic, [N][M] each."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    r = np.ascontiguousarray(cd, dtype=np.float64)
    assert r.shape == (n_sel, count, 2 * dataset.M if manycd else 3)
    out, arrs = _waic_outs(dataset.N, dataset.M, pointwise)
    _check(L.lib().sr_waic(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                           r.ctypes.data_as(_DBLP), int(bool(manycd)), n_sel, count, device, ctypes.byref(out)),
           "sr_waic")
    return _waic_result(out, arrs, n_sel * count, pointwise)


def waic_from_session(session, chains, first=0, count=None, pointwise=True):
    """sr_session_waic: the same over a session's records still in HBM, rows [first, first + count) of chains
    (session chain indices in selection order); shared or per-taxon rates as the session samples them."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs = _waic_outs(session.ds.N, session.ds.M, pointwise)
    _check(L.lib().sr_session_waic(session.h, ch, len(chains), first, count, ctypes.byref(out)), "sr_session_waic")
    return _waic_result(out, arrs, len(chains) * count, pointwise)


def waic_compare(a, b):
    """Two WAIC results with pointwise arrays of equal shape (one dataset, e.g. shared rates against manycd) ->
    {"elpd_diff": the sequential row-major sum of a.elpd_i - b.elpd_i (positive: a fits better), "se_diff":
    sqrt(n * (Q / (n - 1))), Q the sequential sum of (diff_i - elpd_diff / n)^2, n the number of cells (NaN when
    n = 1)}: sr_waic_reduce's two-pass formula on the differences, host numpy.  Only the pointwise array "elpd" is
    read, and a PSIS-LOO result (loo_from_records, loo_from_session) carries its elpd_loo array under that name: two
    LOO results, or a LOO and a WAIC result, compare the same way."""
    ea, eb = np.asarray(a["elpd"], np.float64), np.asarray(b["elpd"], np.float64)
    assert ea.shape == eb.shape and ea.size >= 1
    d = (ea - eb).reshape(-1)
    n = float(d.size)
    tot = np.cumsum(d)[-1]
    dev = d - tot / n
    q = np.cumsum(dev * dev)[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.sqrt(np.float64(n) * (q / np.float64(n - 1.0)))
    return {"elpd_diff": float(tot), "se_diff": float(se)}


# ---------------------------------------------------------------- PSIS-LOO and the Pareto shape per cell
# The same question as WAIC by the estimator recommended over it: leave-one-out cross-validation by Pareto-smoothed
# importance sampling, every output defined to the bit (definitions: include/seriation.h).  pareto_k says where the
# estimate can be trusted; a cell above 0.7 is an occurrence, or an absence, whose likelihood is carried by a handful
# of samples -- the identifications to recheck first.  The sums, the per-cell selection of the largest ratios and the
# generalised-Pareto fit run on the GPU (csrc/sr_loo.hip); there is no CPU fallback.
_LOO_SCALARS = ("elpd", "se", "p_loo", "lppd_sum", "looic")
_LOO_ARRAYS = {"elpd": "elpd_loo", "pareto_k": "pareto_k", "lppd": "lppd", "p_loo_cell": "p_loo_i"}


def _loo_outs(N, M, pointwise):
    arrs = {"site_elpd": np.zeros(N), "taxon_elpd": np.zeros(M)}
    out = L.sr_loo_out()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(_DBLP))
    if pointwise:
        for k, field in _LOO_ARRAYS.items():
            arrs[k] = np.zeros((N, M))
            setattr(out, field, arrs[k].ctypes.data_as(_DBLP))
    return out, arrs


def _loo_result(out, arrs, total):
    res = {k: getattr(out, k) for k in _LOO_SCALARS}
    res["elpd_loo"] = res.pop("elpd")   # "elpd" names the pointwise array, as in a WAIC result
    res["n_k"] = [int(v) for v in out.n_k]
    res["tail_len"] = int(out.tail_len)
    res["total"] = total
    res["kernel_ms"] = out.kernel_ms
    res.update(arrs)
    return res


def loo_from_records(dataset, ab_pi, cd, manycd=False, pointwise=True, device=0):
    """sr_loo: ab_pi and cd as waic_from_records takes them (the rates in [-600, -2^-50]) -> {"elpd_loo", "se",
    "p_loo", "lppd_sum", "looic" (floats), "n_k" (the cells with pareto_k <= 0.5, <= 0.7, <= 1 and above), "tail_len",
    "site_elpd" [N], "taxon_elpd" [M], "total" (the number of samples), "kernel_ms"}; pointwise adds "elpd" (the
    elpd_loo array: waic_compare reads it), "pareto_k", "lppd" and "p_loo_cell" = lppd - elpd, [N][M] each."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    r = np.ascontiguousarray(cd, dtype=np.float64)
    assert r.shape == (n_sel, count, 2 * dataset.M if manycd else 3)
    out, arrs = _loo_outs(dataset.N, dataset.M, pointwise)
    _check(L.lib().sr_loo(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                          r.ctypes.data_as(_DBLP), int(bool(manycd)), n_sel, count, device, ctypes.byref(out)),
           "sr_loo")
    return _loo_result(out, arrs, n_sel * count)


def loo_from_session(session, chains, first=0, count=None, pointwise=True):
    """sr_session_loo: the same over a session's records and rates still in HBM, rows [first, first + count) of
    chains (session chain indices in selection order); shared or per-taxon rates as the session samples them."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs = _loo_outs(session.ds.N, session.ds.M, pointwise)
    _check(L.lib().sr_session_loo(session.h, ch, len(chains), first, count, ctypes.byref(out)), "sr_session_loo")
    return _loo_result(out, arrs, len(chains) * count)


# ---------------------------------------------------------------- posterior predictive checks
# Is the model adequate: for every saved sample, replicate matrices drawn from the model at that sample against X
# under the same sample, on five discrepancies per taxon (ones, span, gaps, false zeros, false ones), the row sums
# per site and the totals (definitions: include/seriation.h).  A p-value near 0 or 1 marks a taxon or site the model
# misfits; the false zeros' is a per-taxon test of the shared rate d.  The draws and the tallies run on the GPU
# (csrc/sr_ppc.hip); there is no CPU fallback.  Every count is an exact integer.
PPC_STATS = ("ones", "span", "gaps", "f0", "f1")


def ppc_pvalue(gt, eq, pairs):
    """(gt + 0.5 * eq) / pairs in float64"""
    return (np.asarray(gt, np.float64) + 0.5 * np.asarray(eq, np.float64)) / np.float64(pairs)


def _ppc_outs(N, M, n_sel, count, reps, totals):
    n, c, r = max(int(n_sel), 0), max(int(count), 0), max(int(reps), 0)
    arrs = {"taxon_gt": np.zeros((5, M), np.uint32), "taxon_eq": np.zeros((5, M), np.uint32),
            "taxon_sum_obs": np.zeros((5, M), np.int64), "taxon_sum_rep": np.zeros((5, M), np.int64),
            "site_gt": np.zeros(N, np.uint32), "site_eq": np.zeros(N, np.uint32), "site_sum_rep": np.zeros(N, np.int64)}
    if totals:
        arrs["total_obs"] = np.zeros((n, c, 5), np.int64)
        arrs["total_rep"] = np.zeros((n, c, r, 5), np.int64)
    out = L.sr_ppc_out()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(_U32P if a.dtype == np.uint32 else _I64P))
    return out, arrs


def _ppc_result(out, arrs):
    res = dict(arrs)
    res["total_gt"] = np.array(list(out.total_gt), np.int64)
    res["total_eq"] = np.array(list(out.total_eq), np.int64)
    res["pairs"] = int(out.pairs)
    res["kernel_ms"] = out.kernel_ms
    res["p_taxon"] = ppc_pvalue(res["taxon_gt"], res["taxon_eq"], res["pairs"])
    res["p_site"] = ppc_pvalue(res["site_gt"], res["site_eq"], res["pairs"])
    res["p_total"] = ppc_pvalue(res["total_gt"], res["total_eq"], res["pairs"])
    return res


def ppc_from_records(dataset, ab_pi, cd, manycd=False, seed=0, reps=1, totals=False, device=0):
    """sr_ppc: ab_pi [n_sel][count][2M+N] and the rates cd as waic_from_records takes them, seed any uint64, reps
    1..64 replicates per sample -> {"taxon_gt", "taxon_eq" [5][M] uint32, "taxon_sum_obs", "taxon_sum_rep" [5][M]
    int64 (rows in the order of PPC_STATS), "site_gt", "site_eq" [N], "site_sum_rep" [N], "total_gt", "total_eq"
    [5], "pairs" = n_sel * count * reps, "kernel_ms", and the p-values (gt + 0.5 eq) / pairs: "p_taxon" [5][M],
    "p_site" [N], "p_total" [5]}; totals adds "total_obs" [n_sel][count][5] and "total_rep" [n_sel][count][reps][5]."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    r = np.ascontiguousarray(cd, dtype=np.float64)
    assert r.shape == (n_sel, count, 2 * dataset.M if manycd else 3)
    out, arrs = _ppc_outs(dataset.N, dataset.M, n_sel, count, reps, totals)
    _check(L.lib().sr_ppc(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                          r.ctypes.data_as(_DBLP), int(bool(manycd)), n_sel, count, int(seed), int(reps), device,
                          ctypes.byref(out)), "sr_ppc")
    return _ppc_result(out, arrs)


def ppc_from_session(session, chains, first=0, count=None, seed=0, reps=1, totals=False):
    """sr_session_ppc: the same over a session's records and rates still in HBM, rows [first, first + count) of
    chains (session chain indices in selection order); shared or per-taxon rates as the session samples them."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs = _ppc_outs(session.ds.N, session.ds.M, len(chains), count, reps, totals)
    _check(L.lib().sr_session_ppc(session.h, ch, len(chains), first, count, int(seed), int(reps), ctypes.byref(out)),
           "sr_session_ppc")
    return _ppc_result(out, arrs)


# ---------------------------------------------------------------- cell occupancy and the error tallies
# Was taxon m alive at site n, which absences are Lazarus gaps and which occurrences lie outside the taxon's range,
# which sites and which taxa carry the errors: joint functions of (pi, a, b) and X, counted exactly over the selected
# chains' samples (definitions: include/seriation.h).  The counts come from the GPU (csrc/sr_occ.hip); there is no CPU
# fallback.  No orientation is needed: a reflected chain gives the same alive bits.  Means and quantile bands of the
# six histograms: diversity_curve.
OCC_KINDS = ("alive", "site_alive_hist", "site_f0_hist", "site_f1_hist", "taxon_alive_hist", "taxon_f0_hist",
             "taxon_f1_hist")


def _occ_outs(N, M, kinds):
    shapes = {k: ((N, M) if k == "alive" else (N, M + 1) if k.startswith("site_") else (M, N + 1)) for k in OCC_KINDS}
    arrs = {k: np.zeros(shapes[k], np.uint32) for k in kinds}
    out = L.sr_occ_out()
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return out, arrs


def occupancy_derived(alive, X, total):
    """alive [N][M] (exact counts over `total` samples) and X [N][M] -> the host-side f64 values, each one division of
    exact integers: "p_alive" = alive / T; "p_false_zero" = alive / T where x = 0, NaN elsewhere; "p_false_one" =
    (T - alive) / T where x = 1, NaN elsewhere; "site_completeness" [N] = sum_m x alive / sum_m alive, the expected
    share of the taxa alive at the site that were found there (NaN when the denominator is 0)."""
    a = np.asarray(alive).astype(np.int64)
    x = np.asarray(X) != 0
    T = np.float64(total)
    p = a.astype(np.float64) / T
    den = a.sum(axis=1)
    num = np.where(x, a, 0).sum(axis=1)
    comp = np.full(a.shape[0], np.nan)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=comp, where=den != 0)
    return {"p_alive": p, "p_false_zero": np.where(x, np.nan, p),
            "p_false_one": np.where(x, (np.int64(total) - a).astype(np.float64) / T, np.nan),
            "site_completeness": comp}


def _occ_result(out, arrs, X, total):
    res = dict(arrs)
    res["total"] = total
    res["kernel_ms"] = out.kernel_ms
    if "alive" in arrs:
        res.update(occupancy_derived(arrs["alive"], X, total))
    return res


def _dataset_x(ds):
    return np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M).copy()


def occupancy_from_records(dataset, ab_pi, kinds=OCC_KINDS, device=0):
    """sr_occupancy: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order) -> {kind: uint32 array}
    for the requested kinds ("alive": [N][M]; "site_alive_hist", "site_f0_hist", "site_f1_hist": [N][M+1];
    "taxon_alive_hist", "taxon_f0_hist", "taxon_f1_hist": [M][N+1]) plus "total" (the number of samples T) and
    "kernel_ms"; with "alive" also "p_alive", "p_false_zero", "p_false_one" [N][M] and "site_completeness" [N]
    (occupancy_derived)."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    out, arrs = _occ_outs(dataset.N, dataset.M, kinds)
    _check(L.lib().sr_occupancy(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel,
                                count, device, ctypes.byref(out)), "sr_occupancy")
    return _occ_result(out, arrs, _dataset_x(dataset), n_sel * count)


def occupancy_from_session(session, chains, first=0, count=None, kinds=OCC_KINDS):
    """sr_session_occupancy: the same over a session's records still in HBM, rows [first, first + count) of chains
    (session chain indices in selection order)."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs = _occ_outs(session.ds.N, session.ds.M, kinds)
    _check(L.lib().sr_session_occupancy(session.h, ch, len(chains), first, count, ctypes.byref(out)),
           "sr_session_occupancy")
    return _occ_result(out, arrs, _dataset_x(session.ds), len(chains) * count)


# ---------------------------------------------------------------- placement of query rows
# Where does a row that was not in the run belong: a new or fragmentary locality's faunal list (0 absent, 1 present,
# 2 not assessed) against the selected chains' samples.  Per sample the row's likelihood at every position, normalised
# over the positions; averaged over the samples, per position ("pos") and per site of the run ("site"), every output
# defined to the bit (definitions: include/seriation.h "Placement").  Position p means "of the same age as whichever
# site sits at position p", not an insertion between two sites; placing one of the run's own rows is in-sample.  The
# T Q N M part runs on the GPU (csrc/sr_place.hip); there is no CPU fallback.  Orient the chains first (flips):
# "pos" of mirrored chains averages a distribution with its mirror image.
def _place_outs(N, n_sel, count, Q, flips, lse):
    n, c, q = max(int(n_sel), 0), max(int(count), 0), max(int(Q), 0)
    arrs = {"pos": np.zeros((q, N)), "site": np.zeros((q, N)), "lpd": np.zeros(q)}
    if lse:
        arrs["lse"] = np.zeros((n, c, q))
    out = L.sr_place_out()
    f, fp = _flip_arg(flips, n_sel)
    if f is not None:
        out.flip = fp
    for k, a in arrs.items():
        setattr(out, k, a.ctypes.data_as(_DBLP))
    return out, arrs, [f]   # the last: the buffer the struct points into


def _place_result(out, arrs, total):
    arrs["total"] = total
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def _queries(queries, M):
    y = np.ascontiguousarray(queries, dtype=np.uint8)
    if y.ndim == 1:
        y = y.reshape(1, -1)
    assert y.ndim == 2 and y.shape[1] == M
    return y


def placement_from_records(dataset, ab_pi, cd, queries, manycd=False, flips=None, lse=False, device=0):
    """sr_placement: ab_pi [n_sel][count][2M+N] and cd as waic_from_records takes them, queries [Q][M] (0 absent,
    1 present, 2 not assessed; one row may come as [M]) -> {"pos": [Q][N], the posterior probability that the query is
    of the age of position p, "site": [Q][N], ... of the age of site n, "lpd": [Q], the log predictive density of the
    row under a uniform prior over the positions, "total" (the number of samples), "kernel_ms"}; lse=True adds "lse"
    [n_sel][count][Q], each sample's log of the summed likelihood.  flips [n_sel]: chains whose rows are reflected
    first."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    r = np.ascontiguousarray(cd, dtype=np.float64)
    assert r.shape == (n_sel, count, 2 * dataset.M if manycd else 3)
    y = _queries(queries, dataset.M)
    out, arrs, _keep = _place_outs(dataset.N, n_sel, count, y.shape[0], flips, lse)
    _check(L.lib().sr_placement(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                r.ctypes.data_as(_DBLP), int(bool(manycd)), n_sel, count,
                                y.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), y.shape[0], device,
                                ctypes.byref(out)), "sr_placement")
    return _place_result(out, arrs, n_sel * count)


def placement_from_session(session, chains, queries, first=0, count=None, flips=None, lse=False):
    """sr_session_placement: the same over a session's records still in HBM, rows [first, first + count) of chains
    (session chain indices in selection order); shared or per-taxon rates as the session samples them."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    y = _queries(queries, session.ds.M)
    out, arrs, _keep = _place_outs(session.ds.N, len(chains), count, y.shape[0], flips, lse)
    _check(L.lib().sr_session_placement(session.h, ch, len(chains), first, count,
                                        y.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), y.shape[0],
                                        ctypes.byref(out)), "sr_session_placement")
    return _place_result(out, arrs, len(chains) * count)


def placement_summary(pos, site, probs=PROBS):
    """pos, site [Q][N] (placement_from_records) -> per query {"mean": the mean position sum_p p pos[p], "mode": the
    first position of largest mass, "quant": int [len(probs)][Q], each the smallest p whose cumulative mass reaches
    the probability (N - 1 where rounding keeps the total below it), "best_site": the first site of largest mass,
    "p_best_site": its probability}.  Plain numpy, not defined to the bit."""
    pos, site = np.atleast_2d(np.asarray(pos, np.float64)), np.atleast_2d(np.asarray(site, np.float64))
    Q, N = pos.shape
    cum = np.cumsum(pos, axis=1)
    quant = np.zeros((len(probs), Q), np.int64)
    for i, pr in enumerate(probs):
        quant[i] = np.minimum((cum < pr).sum(axis=1), N - 1)
    best = site.argmax(axis=1)
    return {"mean": pos @ np.arange(N, dtype=np.float64), "mode": pos.argmax(axis=1), "quant": quant,
            "best_site": best, "p_best_site": site[np.arange(Q), best]}


def read_queries(path, M):
    """A query file in the dataset's format: a header line `Q M`, then Q lines of M tokens 0, 1 or ? (not assessed);
    a trailing * (the dataset's hard-site mark) is ignored -> uint8 [Q][M] with 2 for ?.  ValueError on anything
    else."""
    with open(path) as fh:
        lines = [ln for ln in fh.read().splitlines() if ln.strip()]
    head = lines[0].split() if lines else []
    if len(head) != 2 or not all(t.isdigit() for t in head):
        raise ValueError("%s: the first line must be `Q M`" % path)
    Q, m = int(head[0]), int(head[1])
    if m != M:
        raise ValueError("%s: %d taxa, the dataset has %d" % (path, m, M))
    if Q < 1 or len(lines) != 1 + Q:
        raise ValueError("%s: %d rows announced, %d found" % (path, Q, len(lines) - 1))
    code = {"0": 0, "1": 1, "?": 2}
    out = np.zeros((Q, M), np.uint8)
    for q, ln in enumerate(lines[1:]):
        toks = ln.rstrip().rstrip("*").split()
        if len(toks) != M:
            raise ValueError("%s: row %d holds %d tokens, not %d" % (path, q, len(toks), M))
        for j, t in enumerate(toks):
            if t not in code:
                raise ValueError("%s: row %d token %d is %r, not 0, 1 or ?" % (path, q, j, t))
            out[q, j] = code[t]
    return out


# ---------------------------------------------------------------- chain agreement and modes
# Which chains sampled the same order: per chain the exact counts of every site pair's order, the L1 distance between
# every two chains' counts, plain and against the mirror image, and the single-linkage modes read off them
# (definitions: include/seriation.h).  Counts and distances come from the GPU (csrc/sr_agree.hip); there is no CPU
# fallback.  The clustering is the library's host code.  Pool only the chains of one mode, with that mode's flips.
_U32P = ctypes.POINTER(ctypes.c_uint32)


def _agree_outs(N, n_sel, pair_counts):
    n = max(int(n_sel), 0)
    arrs = {"dist": np.zeros((n, n), np.int64), "dist_mirror": np.zeros((n, n), np.int64)}
    out = L.sr_agree_out()
    out.dist = arrs["dist"].ctypes.data_as(_I64P)
    out.dist_mirror = arrs["dist_mirror"].ctypes.data_as(_I64P)
    if pair_counts:
        arrs["pair_counts"] = np.zeros((n, N, N), np.uint32)
        out.pair_counts = arrs["pair_counts"].ctypes.data_as(_U32P)
    return out, arrs


def _agree_result(out, arrs):
    arrs["scale"] = int(out.scale)
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def agreement_from_records(dataset, ab_pi, pair_counts=False, device=0):
    """sr_agreement: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order; only pi is read) ->
    {"dist", "dist_mirror": int64 [n_sel][n_sel], "scale": count * N (N - 1) / 2, "kernel_ms"}; pair_counts=True adds
    "pair_counts" uint32 [n_sel][N][N] (entry [k][i][j]: chain k's rows with pi_i < pi_j)."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    out, arrs = _agree_outs(dataset.N, n_sel, pair_counts)
    _check(L.lib().sr_agreement(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel,
                                count, device, ctypes.byref(out)), "sr_agreement")
    return _agree_result(out, arrs)


def agreement_from_session(session, chains, first=0, count=None, pair_counts=False):
    """sr_session_agreement: the same over a session's records still in HBM, rows [first, first + count) of chains
    (session chain indices in selection order)."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs = _agree_outs(session.ds.N, len(chains), pair_counts)
    _check(L.lib().sr_session_agreement(session.h, ch, len(chains), first, count, ctypes.byref(out)),
           "sr_session_agreement")
    return _agree_result(out, arrs)


def agreement_distances(pair_counts, device=0):
    """sr_agreement_distances: the reduction alone.  pair_counts uint32 [n_sel][N][N] in host memory (any values; e.g.
    matrices gathered from several GPUs) -> {"dist", "dist_mirror": int64 [n_sel][n_sel], "kernel_ms"}."""
    pc = np.ascontiguousarray(pair_counts, dtype=np.uint32)
    assert pc.ndim == 3 and pc.shape[1] == pc.shape[2]
    n = pc.shape[0]
    arrs = {"dist": np.zeros((n, n), np.int64), "dist_mirror": np.zeros((n, n), np.int64)}
    ms = ctypes.c_double(0.0)
    _check(L.lib().sr_agreement_distances(pc.shape[1], n, pc.ctypes.data_as(_U32P), device,
                                          arrs["dist"].ctypes.data_as(_I64P), arrs["dist_mirror"].ctypes.data_as(_I64P),
                                          ctypes.byref(ms)), "sr_agreement_distances")
    arrs["kernel_ms"] = ms.value
    return arrs


def chain_modes(dist, dist_mirror, scale, threshold=0.1):
    """sr_agreement_modes (host only, no GPU): single-linkage modes of the chains.  Chains k < l are linked when
    min(dist[k][l], dist_mirror[k][l]) <= threshold * scale -> {"mode": int32 [n] (numbered by smallest member),
    "flip": uint8 [n], "medoid", "size": int32 [n_modes], "n_modes"}.  flip can be passed straight to the flips= of
    marginals_* / relations_* for the chains of one mode (flip[chains_of_that_mode]).
    The default threshold 0.1 is a default only: it rests on one measurement with the CPU oracle, one dataset
    (g10s10, seeds 1..8) and short runs (300 burn-in + 200 saved calls), where chains of one mode lay within
    0.035-0.066 of each other, the two halves of one chain 0.016-0.040 apart, and every other pair at 0.20-0.73.
    Look at dist / scale of your own run before trusting it."""
    d = np.ascontiguousarray(dist, dtype=np.int64)
    m = np.ascontiguousarray(dist_mirror, dtype=np.int64)
    assert d.ndim == 2 and d.shape[0] == d.shape[1] and m.shape == d.shape
    n = d.shape[0]
    mode, flip = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    medoid, size = np.zeros(n, np.int32), np.zeros(n, np.int32)
    n_modes = ctypes.c_int32(0)
    i32p = ctypes.POINTER(ctypes.c_int32)
    _check(L.lib().sr_agreement_modes(n, d.ctypes.data_as(_I64P), m.ctypes.data_as(_I64P), int(scale), float(threshold),
                                      mode.ctypes.data_as(i32p), flip.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                      medoid.ctypes.data_as(i32p), size.ctypes.data_as(i32p), ctypes.byref(n_modes)),
           "sr_agreement_modes")
    g = n_modes.value
    return {"mode": mode, "flip": flip, "medoid": medoid[:g].copy(), "size": size[:g].copy(), "n_modes": g}


# ---------------------------------------------------------------- the central sampled state
# One coherent answer: the saved record -- a real (pi, a, b) the sampler produced, a permutation that respects the hard
# sites -- with the smallest posterior expected loss, the medoid of the draws (definitions: include/seriation.h).  The
# order loss of a row is the sum of its Kendall distances to all the rows, ties broken by the L1 distance of the
# limits.  Counts and losses come from the GPU (csrc/sr_central.hip); there is no CPU fallback.  Pool only the chains
# of one mode, with that mode's flips.
def _flip_arg(flips, n_sel):
    if flips is None:
        return None, None
    f = np.ascontiguousarray(np.asarray(flips) != 0, dtype=np.uint8)
    assert f.shape == (max(int(n_sel), 0),)
    return f, f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _central_outs(N, M, n_sel, count, flips, pair_counts):
    n, c = max(int(n_sel), 0), max(int(count), 0)
    arrs = {"order_loss": np.zeros((n, c), np.int64), "limit_loss": np.zeros((n, c), np.int64),
            "best": np.zeros(n, np.int32)}
    state = np.zeros(2 * M + N, np.int32)
    out = L.sr_central_out()
    f, fp = _flip_arg(flips, n_sel)
    if f is not None:
        out.flip = fp
    out.order_loss = arrs["order_loss"].ctypes.data_as(_I64P)
    out.limit_loss = arrs["limit_loss"].ctypes.data_as(_I64P)
    out.best = arrs["best"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out.state = state.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    if pair_counts:
        arrs["pair_counts"] = np.zeros((N, N), np.uint32)
        out.pair_counts = arrs["pair_counts"].ctypes.data_as(_U32P)
    return out, arrs, state, [f]   # the last: the buffer the struct points into


def _central_result(out, arrs, state, N, M):
    arrs["central"] = (int(out.central_chain), int(out.central_row))
    arrs["state"] = {"a": state[:M], "b": state[M:2 * M], "pi": state[2 * M:]}
    arrs["scale"] = int(out.scale)
    arrs["kernel_ms"] = out.kernel_ms
    return arrs


def central_from_records(dataset, ab_pi, flips=None, pair_counts=False, device=0):
    """sr_central: ab_pi [n_sel][count][2M+N] (a | b | pi rows, chains in selection order) -> {"order_loss",
    "limit_loss": int64 [n_sel][count], "best": int32 [n_sel] (each chain's row of smallest loss), "central": (chain,
    row) of the smallest (order_loss, limit_loss, chain, row), "state": {"a": [M], "b": [M], "pi": [N]} int32 (that
    row, reflected if its chain is flagged), "scale": T N (N - 1) / 2 (order_loss / scale is the expected normalised
    Kendall distance to a draw), "kernel_ms"}; pair_counts=True adds "pair_counts" uint32 [N][N] (the pooled rows with
    pi_i < pi_j).  flips [n_sel]: chains whose rows are reflected first."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    out, arrs, state, _keep = _central_outs(dataset.N, dataset.M, n_sel, count, flips, pair_counts)
    _check(L.lib().sr_central(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel,
                              count, device, ctypes.byref(out)), "sr_central")
    return _central_result(out, arrs, state, dataset.N, dataset.M)


def central_from_session(session, chains, first=0, count=None, flips=None, pair_counts=False):
    """sr_session_central: the same over a session's records still in HBM, rows [first, first + count) of chains
    (session chain indices in selection order); "central" is (position in chains, row - first)."""
    count = session_records(session) - first if count is None else count
    ch = (ctypes.c_int32 * len(chains))(*[int(c) for c in chains])
    out, arrs, state, _keep = _central_outs(session.ds.N, session.ds.M, len(chains), count, flips, pair_counts)
    _check(L.lib().sr_session_central(session.h, ch, len(chains), first, count, ctypes.byref(out)),
           "sr_session_central")
    return _central_result(out, arrs, state, session.ds.N, session.ds.M)


def order_loss(dataset, ab_pi, against, flips=None, device=0):
    """sr_order_loss: the order loss alone, of the rows ab_pi [n_sel][count][2M+N] against counts the caller holds:
    against uint32 [N][N] (any values, read as central's pair_counts; e.g. another mode's pooled counts, or
    agreement's per-chain pair_counts summed) -> {"order_loss": int64 [n_sel][count], "kernel_ms"}."""
    rec = np.ascontiguousarray(ab_pi, dtype=np.int16)
    assert rec.ndim == 3 and rec.shape[2] == 2 * dataset.M + dataset.N
    n_sel, count = rec.shape[0], rec.shape[1]
    ag = np.ascontiguousarray(against, dtype=np.uint32)
    assert ag.shape == (dataset.N, dataset.N)
    loss = np.zeros((n_sel, count), np.int64)
    _f, fp = _flip_arg(flips, n_sel)
    ms = ctypes.c_double(0.0)
    _check(L.lib().sr_order_loss(ctypes.byref(dataset.c), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), n_sel,
                                 count, fp, ag.ctypes.data_as(_U32P), device, loss.ctypes.data_as(_I64P),
                                 ctypes.byref(ms)), "sr_order_loss")
    return {"order_loss": loss, "kernel_ms": ms.value}


def read_chain_cd(root, chains, taxa, manycd=False):
    """chain_data.csv of each chain -> the rates on the log scale, c = math.log(float(token)) of fields 3 and 4:
    float64 [n][lines][3] (the first c and d token and field 5, the line's loglik) or, manycd, [n][lines][2M] (all M
    c tokens, then all M d tokens).  All chains must hold the same number of lines."""
    out = []
    for chain in chains:
        rows = []
        for line in _chain_lines(root, chain):
            f = line.split(",")
            c, d = f[3].split()[:taxa], f[4].split()[:taxa]
            if manycd:
                rows.append([math.log(float(t)) for t in c] + [math.log(float(t)) for t in d])
            else:
                rows.append([math.log(float(c[0])), math.log(float(d[0])), float(f[5])])
        out.append(np.array(rows, np.float64).reshape(len(rows), 2 * taxa if manycd else 3))
    return np.stack(out)


def read_chain_rows(root, chains, sites, taxa):
    """chain_data.csv of each chain -> int16 [n][lines][2M+N] (fields 0, 1, 2 tokens as the script
    slices them).  All chains must hold the same number of lines."""
    out = []
    for chain in chains:
        rows = []
        for line in _chain_lines(root, chain):
            f = line.split(",", 3)
            rows.append(np.concatenate([np.array(f[0].split(), np.int64)[:taxa], np.array(f[1].split(), np.int64)[:taxa],
                                        np.array(f[2].split(), np.int64)[:sites]]))
        out.append(np.array(rows, np.int16).reshape(len(rows), 2 * taxa + sites))
    return np.stack(out)


def _file_posterior(chains, chains_selected, sites, taxa, kinds, root, X=None, device=0):
    from .core import Dataset
    rec = read_chain_rows(root, chains, sites, taxa)
    ds = Dataset(np.zeros((sites, taxa), np.uint8) if X is None else np.asarray(X, np.uint8)[:sites, :taxa],
                 np.zeros(sites, bool))
    return posterior_from_records(ds, rec, chains_selected, kinds, device)


def compute_pair_order_matrix(chains, chains_selected, sites, root=".", taxa=None, device=0):
    """script.py:155-189 on the GPU (quirk kept: the per-chain accumulator is never reset).
    taxa: M of the chain files (read from the first line when omitted)."""
    taxa = taxa or _taxa_of(root, chains[0])
    return _file_posterior(chains, chains_selected, sites, taxa, ("pair_order",), root, device=device)["pair_order"]


def compute_exp_pi(chains, sites, chains_selected, root=".", taxa=None, device=0):
    """script.py:230-251 on the GPU (quirk kept: the result is the last per-chain snapshot)."""
    taxa = taxa or _taxa_of(root, chains[0])
    return _file_posterior(chains, chains_selected, sites, taxa, ("exp_pi",), root, device=device)["exp_pi"]


def compute_exp_a(chains, chains_selected, taxa, root=".", sites=None, device=0):
    """script.py:254-275 on the GPU."""
    sites = sites or _sites_of(root, chains[0], taxa)
    return _file_posterior(chains, chains_selected, sites, taxa, ("exp_a",), root, device=device)["exp_a"]


def reorder(mat, exp_pi, exp_a):
    """Rows by the inverse permutation of argsort(exp_pi), columns in argsort(exp_a) order
    (script.py:288-301, 336-347)."""
    rpi = np.argsort(exp_pi)
    idx = np.empty_like(rpi)
    idx[rpi] = np.arange(len(rpi))
    return np.asarray(mat)[idx, :][:, np.argsort(exp_a)]


def taxa_occurence_probability_matrix(chains, chains_selected, sites, taxa, root=".", device=0):
    """plot_taxa_occurence_probability_matrix's return value (script.py:306-347)."""
    r = _file_posterior(chains, chains_selected, sites, taxa, ("alive", "exp_pi", "exp_a"), root, device=device)
    return reorder(r["alive"], r["exp_pi"], r["exp_a"])


def false_taxa_occurence_probability(chains, chains_selected, sites, taxa, root=".", device=0):
    """plot_false_taxa_occurence_probability's return value (script.py:350-389)."""
    r = _file_posterior(chains, chains_selected, sites, taxa, ("false_alive", "exp_pi", "exp_a"), root, device=device)
    return reorder(r["false_alive"], r["exp_pi"], r["exp_a"])


def false_ones_probability(chains, chains_selected, dataset, sites, taxa, root=".", device=0):
    """plot_false_ones_probability's return value (script.py:392-429), N x M (the script
    hard-codes the 124 x 139 shape of g10s10)."""
    from .core import Dataset
    ds = dataset if isinstance(dataset, Dataset) else Dataset.load(str(dataset), maxs=0)
    r = _file_posterior(chains, chains_selected, sites, taxa, ("false_ones", "exp_pi", "exp_a"), root, X=ds.X,
                        device=device)
    return reorder(r["false_ones"], r["exp_pi"], r["exp_a"])


def _taxa_of(root, chain):
    with open(os.path.join(root, "Chains", "chain_%02d" % chain, "chain_data.csv")) as fh:
        return len(fh.readline().split(",", 1)[0].split())


def _sites_of(root, chain, taxa):
    with open(os.path.join(root, "Chains", "chain_%02d" % chain, "chain_data.csv")) as fh:
        return len(fh.readline().split(",")[2].split())
