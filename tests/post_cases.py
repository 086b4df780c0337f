"""TEST INFRASTRUCTURE ONLY -- the edge matrix of the posterior kernel (csrc/sr_post.hip): shapes, sample streams
and record kinds, shared by the GPU comparison (tests/test_gpu_posterior_edges.py) and by the CPU tests that check
the reference at these edges (tests/test_posterior_oracle.py) and that the inputs can tell a subtly wrong kernel
from a right one (tests/test_posterior_edges_host.py).

The kernel tiles its output TR = 16 rows x TCOL = 64 columns, four rows per wave, and consumes the selected chains'
rows as one stream in LDS chunks of CS = 64 samples, two buffers.  The shapes cross each tile edge by one element
and hit it exactly; the streams do the same with the chunk edge, put chain ends inside a chunk, on its edge and
more than once per chunk, and include a view of no rows."""
import collections

import numpy as np

TR, TCOL, CS = 16, 64, 64   # sr_post.hip's tile and chunk

SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (64, 16), (65, 17), (129, 130)]
# (n_sel, count); every one of them at (17, 65) and at (65, 17)
STREAMS = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 128), (1, 129), (2, 32), (3, 64), (5, 13), (70, 1), (2, 0)]
# the other shapes: a chunk edge crossed with a chain end off it, and a stream that ends on it
OTHER_STREAMS = {(1, 1): [(2, 1), (3, 43)], (15, 63): [(2, 33)], (16, 64): [(3, 43), (1, 64)], (64, 16): [(2, 65)],
                 (129, 130): [(4, 40), (1, 65)]}
KINDS = ("random", "limits", "extreme")
XMODES = ("ones", "zeros", "half", "twos")

Case = collections.namedtuple("Case", "kind N M n_sel count cs xmode")


def case_id(c):
    return "%s-%dx%d-%dx%d-cs%d-%s" % c


def _cases():
    out = []
    for N, M in SHAPES:
        for n_sel, count in (STREAMS if (N, M) in ((17, 65), (65, 17)) else OTHER_STREAMS[(N, M)]):
            for kind in (KINDS if count else KINDS[:1]):   # no rows: nothing to fill
                i = len(out)
                # the script divides by its own argument, not by the number of chains it was given
                cs = (n_sel + 5, n_sel // 2 if n_sel > 1 else 3, 8, n_sel)[i % 4]
                out.append(Case(kind, N, M, n_sel, count, cs, XMODES[(i // 4 + i) % 4]))
    # chains_selected < 0: include/seriation.h sets no sign and the library refuses only 0
    out.append(Case("limits", 17, 65, 5, 13, -3, "half"))
    out.append(Case("random", 65, 17, 2, 0, -2, "ones"))
    return out


CASES = _cases()


def limit_plants(N):
    """(a, b) pairs that put, in every row tile of the kernel, each of j == a, j == b, j == a - 1 and j == b + 1
    on a row j of that tile: (r, r) and (r + 1, r - 1) for one row r per tile (b = -1 for r = 0)."""
    out = []
    for t in range((N + TR - 1) // TR):
        rows = min(TR, N - t * TR)
        r = t * TR + (5 * t + 3) % rows   # not always the same one of a wave's four rows
        out += [(r, r), (r + 1, r - 1)]
    return out


def limit_events(rec, N, M):
    """[tiles][4] bool: does j == a, j == b, j == a - 1, j == b + 1 occur for a row j of each row tile?"""
    a = rec[..., :M].astype(np.int64).reshape(-1)
    b = rec[..., M:2 * M].astype(np.int64).reshape(-1)
    out = []
    for t in range((N + TR - 1) // TR):
        lo, hi = t * TR, min(N, (t + 1) * TR) - 1
        out.append([bool(np.any((v >= lo) & (v <= hi))) for v in (a, b, a - 1, b + 1)])
    return np.array(out)


def records(kind, N, M, n_sel, count, rng):
    """[n_sel][count][2M+N] int16 rows a | b | pi.
    random: limits 0 <= a <= b <= N, pi a permutation (pi[site] = position).
    limits: a and b of every taxon and row drawn from {0, j-1, j, j+1, N-1, N} for a site index j of its own, both
            orders, limit_plants() planted; pi a permutation.
    extreme: any int16 in every column (pi is then no permutation: the script's arithmetic does not care), with
            -32768 and 32767 planted in an a, a b and a pi column."""
    T, W = n_sel * count, 2 * M + N
    if kind == "extreme":
        x = rng.integers(-32768, 32768, (T, W))
        if T:
            x[0, 0], x[0, M], x[0, 2 * M] = -32768, 32767, -32768
            x[T - 1, M - 1], x[T - 1, 2 * M - 1], x[T - 1, W - 1] = 32767, -32768, 32767
        return x.astype(np.int16).reshape(n_sel, count, W)
    pi = np.argsort(rng.random((T, N)), axis=1)
    if kind == "random":
        a = rng.integers(0, N + 1, (T, M))
        b = np.minimum(N, a + rng.integers(0, N // 2 + 1, (T, M)))
    else:
        assert kind == "limits"
        j = rng.integers(0, N, (T, M))
        opts = np.stack([np.zeros_like(j), j - 1, j, j + 1, np.full_like(j, N - 1), np.full_like(j, N)], axis=2)
        a = np.take_along_axis(opts, rng.integers(0, 6, (T, M, 1)), 2)[..., 0]
        b = np.take_along_axis(opts, rng.integers(0, 6, (T, M, 1)), 2)[..., 0]
        plants = limit_plants(N)
        if T:
            assert T * M >= len(plants), "stream too short for the planted limits"
            slots = rng.choice(T * M, len(plants), replace=False)
            a.reshape(-1)[slots] = [p[0] for p in plants]
            b.reshape(-1)[slots] = [p[1] for p in plants]
    return np.concatenate([a, b, pi], axis=1).astype(np.int16).reshape(n_sel, count, W)


def dataset_x(xmode, N, M, rng):
    """X for false_ones: all ones, all zeros, density 0.5, or thirds of 0 / 1 / 2 (the script counts X == 1 only;
    seriation_amd.Dataset takes any uint8 matrix)."""
    if xmode == "ones":
        return np.ones((N, M), np.uint8)
    if xmode == "zeros":
        return np.zeros((N, M), np.uint8)
    if xmode == "half":
        return (rng.random((N, M)) < 0.5).astype(np.uint8)
    assert xmode == "twos"
    x = rng.integers(0, 3, (N, M)).astype(np.uint8)
    x.reshape(-1)[0] = 2
    return x


_BUILT = {}


def build(case):
    """(records [n_sel][count][2M+N] int16, X [N][M] uint8) of a case; built once, never modified."""
    if case not in _BUILT:
        rng = np.random.default_rng([case.N, case.M, case.n_sel, case.count, KINDS.index(case.kind)])
        rec = records(case.kind, case.N, case.M, case.n_sel, case.count, rng)
        X = dataset_x(case.xmode, case.N, case.M, rng)
        rec.setflags(write=False)
        X.setflags(write=False)
        _BUILT[case] = (rec, X)
    return _BUILT[case]


def chain_rows(rec):
    """the records as om_script takes them: one int64 [count][2M+N] array per chain, in selection order"""
    return [rec[k].astype(np.int64) for k in range(rec.shape[0])]
