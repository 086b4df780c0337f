"""Hand-made columns for the Gibbs picks of the 9-word register walks -- TEST INFRASTRUCTURE.

draw_fast_s<9> (csrc/sr_device.hip) has no window: it sums every word of the walk from y = 1 at walk entry 0.  That
is sound because a walk of at most 288 entries cannot leave the f64 range upwards (every y < 2^667) and because
whatever a chain computes after sinking below 2^-1022 stays below 2^-355 of a total S >= 1.  The columns here drive
the chain to those ends: only zeros (the steepest rise), only ones (the chain reaches exactly 0), ones then zeros
(the chain sinks into the subnormals and rises again), zeros then ones; and walks that end on the boundaries of the
word, byte and table-trim cases of pass 1.  The case dicts have the keys of cert_cases.gibbs_cases, with u on and
around the reference's own CDF boundaries, and the oracle's expected picks.
"""
import functools

import numpy as np

import cert_cases
import oracle_ref

SINK = 110   # ones that take the chain below 2^-1022 at the steepest vB (9.64 bits per one: 106 are enough)


def corners():
    """The four corners of mcmc_samplebeta's bounds: the steepest and the flattest walks."""
    return [(c, d) for c in (cert_cases.MINC, cert_cases.MAXC) for d in (cert_cases.MIND, cert_cases.MAXD)]


def extreme_walks(N):
    """(name, walk-order bits x[0..L), limit o) with L = N: the longest walk of the shape."""
    L = N
    z, e = np.zeros(L, np.int32), np.ones(L, np.int32)
    out = [("zeros", z, L), ("ones", e, 0)]
    for k, os_ in ((SINK, (0, SINK, L)), (L // 2, (L // 2,))):
        oz = np.concatenate([e[:k], z[k:]])
        zo = np.concatenate([z[:k], e[k:]])
        for o in os_:
            out.append(("ones%d-zeros-o%d" % (k, o), oz, o))
            out.append(("zeros%d-ones-o%d" % (k, o), zo, o))
    return out


def end_walks(N, ends, seed):
    """Walks that end at L in `ends` (entries 0..L) over a sparse random column, from limits at both ends and
    in the middle."""
    rng = np.random.default_rng(seed)
    out = []
    for L in ends:
        if L > N:
            continue
        x = (rng.random(L) < 0.2).astype(np.int32)
        for o in sorted({0, L // 2, L}):
            out.append(("end%d-o%d" % (L, o), x, o))
    return out


def column(x, N, rev):
    """The position-ordered column whose walk (cert_cases.walk_bits) begins with x; zeros beyond the walk."""
    col = np.zeros(N, np.int32)
    if rev:
        col[N - len(x):] = x[::-1]
    else:
        col[:len(x)] = x
    return col


def ladder(x, o, c, d, N):
    """u values for one walk: 0, 0.5, the largest double below 1, and cert_cases.u_ladder around the reference's
    boundaries of the heaviest entries, the ends of the mass, the limit and both ends of the walk."""
    L = len(x)
    us = [0.0, 0.5, float(np.nextafter(1.0, 0.0))]
    for i in cert_cases._boundaries(x, o, c, d, (0, L - 1)):
        ub = oracle_ref.auxa_boundary(x, o, c, d, i)
        if 0.0 <= ub <= 1.0:
            us.extend(cert_cases.u_ladder(ub, N))
    return us


def build(N, walks, revs=(False,), grid=None):
    """Blocks of 64 cases sharing (c, d) and one column, as cert_cases.gibbs_cases lays them out; `walk` names the
    walk of each case."""
    grid = corners() if grid is None else grid
    cols, cidx, cds, oo, LL, rv, uu, exp, names = [], [], [], [], [], [], [], [], []
    for name, x, o in walks:
        L = len(x)
        for rev in revs:
            col = column(x, N, rev)
            assert np.array_equal(cert_cases.walk_bits(col, N, rev, L), x)
            cols.append(col)
            for c, d in grid:
                us = ladder(x, o, c, d, N)
                us += [0.5] * (-len(us) % 64)
                cds.extend([(c, d)] * (len(us) // 64))
                for u in us:
                    cidx.append(len(cols) - 1)
                    oo.append(o)
                    LL.append(L)
                    rv.append(1 if rev else 0)
                    uu.append(u)
                    exp.append(oracle_ref.auxa_pick(x, o, c, d, u))
                    names.append(name)
    n = len(uu)
    NW = (N + 31) // 32
    ncol = len(cols)
    bits = np.zeros((ncol, NW * 32), np.uint8)
    bits[:, :N] = np.array(cols, np.uint8)
    grp = bits.reshape(ncol, NW, 32)
    words = (grp.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    ones = np.concatenate([np.zeros((ncol, 1), np.int64), np.cumsum(grp.sum(-1), axis=1)], axis=1)
    ci = np.array(cidx)
    return dict(N=N, n=n, P=np.ascontiguousarray(words[ci].T), pre=np.ascontiguousarray(ones[ci].astype(np.uint16).T),
                cd=np.array(cds, np.float64), o=np.array(oo, np.int32), L=np.array(LL, np.int32),
                rev=np.array(rv, np.int32), u=np.array(uu, np.float64), expected=np.array(exp, np.int32), cols=cols,
                cidx=ci, walk=names)


@functools.lru_cache(maxsize=None)
def extreme_cases(N, both_directions=False):
    """The extreme walks of shape N at the four corners (computed once per process; do not modify)."""
    return build(N, extreme_walks(N), revs=(False, True) if both_directions else (False,))
