"""Do the inputs of the posterior edge matrix (tests/post_cases.py) discriminate?  CPU only.

The GPU test compares csrc/sr_post.hip with oracle/om_script.py on those cases; it is worth what the cases can
tell apart.  Here the definition is restated once more in numpy with a switch for each of seven mistakes a kernel
of that structure could make; for every mistake at least one case of the matrix must give bits that differ from
om_script's, and without a mistake the restatement must give om_script's bits.  The `limits` records must also
hold what they promise: in every row tile, a row equal to a limit and a row one off it, on both sides."""
import numpy as np
import pytest

import om_script
import post_cases

KINDS = ("pair_order", "alive", "false_alive", "false_ones", "exp_pi", "exp_a")

# mistake -> the kinds it can show in
VARIANTS = {
    "reset": KINDS,                                     # the accumulator reset at each chain end
    "gt_a": ("alive", "false_alive", "false_ones"),     # j > a in place of j >= a
    "lt_b": ("alive", "false_alive", "false_ones"),     # j < b in place of j <= b
    "drop63": KINDS,                                    # the last row of every 64-row chunk of the stream dropped
    "late_end": KINDS,                                  # the first row after a chain end counted into the previous chain
    "diag": ("pair_order",),                            # the diagonal of pair_order treated like any other element
    "x_ne0": ("false_ones",),                           # X != 0 in place of X == 1
}


def same(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def value(kind, row, N, M, X, variant):
    """what one sample adds to every element of one kind"""
    a, b, pi = row[:M][None, :], row[M:2 * M][None, :], row[2 * M:]
    if kind == "pair_order":
        v = (pi[:, None] < pi[None, :]).astype(np.float64)
        if variant != "diag":
            v[np.eye(N, dtype=bool)] = -1.0
        return v
    if kind == "exp_pi":
        return pi.astype(np.float64)
    if kind == "exp_a":
        return a[0].astype(np.float64)
    j = np.arange(N)[:, None]
    inside = ((j > a) if variant == "gt_a" else (j >= a)) & ((j < b) if variant == "lt_b" else (j <= b))
    if kind == "alive":
        return inside.astype(np.float64)
    if kind == "false_alive":
        return (~inside).astype(np.float64)
    return (((X != 0) if variant == "x_ne0" else (X == 1)) & ~inside).astype(np.float64)


def restated(kind, rec, cs, N, M, X, variant=None):
    """The definition (sr_post.hip's header comment) as one stream of samples: acc += v per sample; at each chain
    end acc /= 1000 and tot += acc (exp_pi: tot = 0 + acc); tot / chains_selected."""
    n_sel, count = rec.shape[:2]
    rows = rec.astype(np.int64)
    shape = {"pair_order": (N, N), "exp_pi": (N,), "exp_a": (M,)}.get(kind, (N, M))
    st = {"acc": np.zeros(shape), "tot": np.zeros(shape)}

    def end():
        st["acc"] = st["acc"] / 1000
        st["tot"] = (0 + st["acc"]) if kind == "exp_pi" else st["tot"] + st["acc"]

    g, pending = 0, False
    for ch in range(n_sel):
        if variant == "reset":
            st["acc"] = np.zeros(shape)
        for s in range(count):
            if not (variant == "drop63" and g % post_cases.CS == post_cases.CS - 1):
                st["acc"] = st["acc"] + value(kind, rows[ch, s], N, M, X, variant)
            if pending:
                end()
                pending = False
            g += 1
        if variant == "late_end" and count and ch < n_sel - 1:
            pending = True
        else:
            end()
    return st["tot"] / cs


def script(kind, rec, cs, N, M, X):
    rows = post_cases.chain_rows(rec)
    return {"pair_order": lambda: om_script.pair_order_matrix(rows, cs, N, M),
            "alive": lambda: om_script.alive_sum(rows, cs, N, M),
            "false_alive": lambda: om_script.false_alive_sum(rows, cs, N, M),
            "false_ones": lambda: om_script.false_ones_sum(rows, cs, X, N, M),
            "exp_pi": lambda: om_script.exp_pi(rows, N, cs, M),
            "exp_a": lambda: om_script.exp_a(rows, cs, M)}[kind]()


def cost(c):
    return c.n_sel * c.count * c.N * max(c.N, c.M)


BY_COST = sorted(post_cases.CASES, key=cost)


def test_matrix_is_the_issue_s():
    """every shape; every stream at (17, 65) and (65, 17); all three kinds wherever there are rows; all four X"""
    seen = {(c.N, c.M) for c in post_cases.CASES}
    assert seen == set(post_cases.SHAPES)
    for shape in ((17, 65), (65, 17)):
        for kind in post_cases.KINDS:
            got = {(c.n_sel, c.count) for c in post_cases.CASES if (c.N, c.M) == shape and c.kind == kind}
            assert got >= {st for st in post_cases.STREAMS if st[1]}, (shape, kind)
        assert any((c.N, c.M) == shape and c.count == 0 for c in post_cases.CASES)
    for shape in post_cases.SHAPES:
        assert {c.kind for c in post_cases.CASES if (c.N, c.M) == shape} == set(post_cases.KINDS)
    assert {c.xmode for c in post_cases.CASES} == set(post_cases.XMODES)
    cs = [(c.cs > c.n_sel) - (c.cs < c.n_sel) for c in post_cases.CASES]
    assert cs.count(0) * 2 < len(cs) and 1 in cs and -1 in cs and any(c.cs < 0 for c in post_cases.CASES)
    assert len(set(post_cases.CASES)) == len(post_cases.CASES)


@pytest.mark.parametrize("case", [c for c in post_cases.CASES if c.kind == "limits"], ids=post_cases.case_id)
def test_limits_records_hold_their_promise(case):
    rec, _ = post_cases.build(case)
    N, M = case.N, case.M
    a, b, pi = rec[..., :M].astype(int), rec[..., M:2 * M].astype(int), rec[..., 2 * M:]
    assert post_cases.limit_events(rec, N, M).all()
    assert (a <= b).any() and (a > b).any()
    assert a.min() >= -1 and a.max() <= N and b.min() >= -1 and b.max() <= N
    assert np.array_equal(np.sort(pi, axis=2), np.broadcast_to(np.arange(N), pi.shape))


@pytest.mark.parametrize("case", [c for c in post_cases.CASES if c.kind == "limits"], ids=post_cases.case_id)
def test_limits_catch_both_thresholds_in_every_row_tile(case):
    """so a wrong comparison in one wave's rows only, or in the last (partly filled) row tile only, shows"""
    rec, X = post_cases.build(case)
    want = script("alive", rec, case.cs, case.N, case.M, X)
    for variant in ("gt_a", "lt_b"):
        got = restated("alive", rec, case.cs, case.N, case.M, X, variant)
        diff = (got.view(np.uint64) != want.view(np.uint64)).any(axis=1)
        for t in range(0, case.N, post_cases.TR):
            assert diff[t:t + post_cases.TR].any(), (variant, t)


def test_extreme_records_hold_both_ends():
    for case in post_cases.CASES:
        if case.kind == "extreme":
            rec, _ = post_cases.build(case)
            for cols in (rec[..., :case.M], rec[..., case.M:2 * case.M], rec[..., 2 * case.M:]):
                assert cols.min() == -32768 or cols.max() == 32767
            assert rec.min() == -32768 and rec.max() == 32767


def test_restatement_is_the_script():
    """no mistake switched on: om_script's bits, on the cheaper half of the matrix (every stream, both signs of
    chains_selected) -- so a difference below is the mistake's"""
    for case in BY_COST[:len(BY_COST) // 2] + [c for c in post_cases.CASES if c.cs < 0]:
        rec, X = post_cases.build(case)
        for kind in KINDS:
            assert same(restated(kind, rec, case.cs, case.N, case.M, X),
                        script(kind, rec, case.cs, case.N, case.M, X)), (case, kind)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_some_case_catches(variant):
    caught = None
    for case in BY_COST:
        if variant in ("reset", "late_end") and (case.n_sel < 2 or case.count < 1):
            continue
        if variant == "drop63" and case.n_sel * case.count < post_cases.CS:
            continue
        if variant == "x_ne0" and case.xmode != "twos":
            continue
        rec, X = post_cases.build(case)
        for kind in VARIANTS[variant]:
            if not same(restated(kind, rec, case.cs, case.N, case.M, X, variant),
                        script(kind, rec, case.cs, case.N, case.M, X)):
                caught = (case, kind)
                break
        if caught:
            break
    assert caught, "no case of the matrix tells '%s' from the script" % variant
    print("%s: caught by %s (%s)" % (variant, post_cases.case_id(caught[0]), caught[1]))
