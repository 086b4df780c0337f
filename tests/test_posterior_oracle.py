"""The posterior-summary checker (oracle/om_script.py) against the reference script's scalar loops
transcribed literally (script.py:155-189, 230-275, 306-417), bit for bit, on small random samples and at the edges
the GPU matrix adds (tests/post_cases.py: chains of no rows and of one row, limits equal to the site index and one
off it, any int16, X entries of 2, chains_selected < 0).
CPU only: the GPU kernels are compared with om_script in tests/test_gpu_posterior.py and
tests/test_gpu_posterior_edges.py."""
import numpy as np
import pytest

import om_script


def random_rows(rng, nch, ns, N, M):
    out = []
    for _ in range(nch):
        rows = []
        for _ in range(ns):
            a = rng.integers(0, N + 1, M)
            b = np.minimum(N, a + rng.integers(0, N // 2 + 1, M))
            pi = rng.permutation(N)
            rows.append(np.concatenate([a, b, pi]))
        out.append(np.array(rows, np.int64))
    return out


def lit_po(chains_rows, cs, N, M):   # script.py:155-189
    po = np.zeros((N, N))
    poc = np.zeros((N, N))
    for rows in chains_rows:
        for r in rows:
            p = list(r[2 * M:])
            for i in range(N):
                for j in range(N):
                    if i == j:
                        poc[i][j] += -1
                    else:
                        poc[i][j] += int(p[i] < p[j])
        poc /= 1000
        po += poc
    po /= cs
    return po


def lit_site_taxon(chains_rows, cs, N, M, kind, X=None):   # script.py:315-333, 359-377, 401-417
    xs = np.zeros((N, M))
    xsc = np.zeros((N, M))
    for rows in chains_rows:
        for r in rows:
            a_chain = list(r[:M])
            b_chain = list(r[M:2 * M])
            for i, a in enumerate(a_chain):
                for j in range(N):
                    if kind == "alive":
                        xsc[j][i] += int(j >= a and j <= b_chain[i])
                    elif kind == "false_alive":
                        xsc[j][i] += int(j < a or j > b_chain[i])
                    elif X[j][i] == 1:
                        if j >= a and j <= b_chain[i]:
                            xsc[j][i] += 0
                        else:
                            xsc[j][i] += 1
        xsc /= 1000
        xs += xsc
    xs /= cs
    return xs


def lit_exp_pi(chains_rows, N, cs, M):   # script.py:230-251
    pi_sum = np.zeros(shape=(N,))
    pi_sum_chain = np.zeros(shape=(N,))
    for rows in chains_rows:
        pi_sum = 0
        for r in rows:
            pi_sum_chain += list(r[2 * M:])
        pi_sum_chain /= 1000
        pi_sum += pi_sum_chain
    return pi_sum / cs


def lit_exp_a(chains_rows, cs, M):   # script.py:254-275
    a_sum = np.zeros(shape=(M,))
    a_sum_chain = np.zeros(shape=(M,))
    for rows in chains_rows:
        for r in rows:
            a_sum_chain += list(r[:M])
        a_sum_chain /= 1000
        a_sum += a_sum_chain
    return a_sum / cs


def same(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("nch,ns,N,M,cs", [(1, 7, 5, 4, 1), (3, 40, 9, 6, 3), (4, 25, 12, 10, 8)])
def test_om_script_matches_literal_loops(nch, ns, N, M, cs):
    rng = np.random.default_rng(nch * 100 + ns)
    rows = random_rows(rng, nch, ns, N, M)
    X = (rng.random((N, M)) < 0.4).astype(np.uint8)
    assert same(om_script.pair_order_matrix(rows, cs, N, M), lit_po(rows, cs, N, M))
    assert same(om_script.alive_sum(rows, cs, N, M), lit_site_taxon(rows, cs, N, M, "alive"))
    assert same(om_script.false_alive_sum(rows, cs, N, M), lit_site_taxon(rows, cs, N, M, "false_alive"))
    assert same(om_script.false_ones_sum(rows, cs, X, N, M), lit_site_taxon(rows, cs, N, M, "false_ones", X))
    assert same(om_script.exp_pi(rows, N, cs, M), lit_exp_pi(rows, N, cs, M))
    assert same(om_script.exp_a(rows, cs, M), lit_exp_a(rows, cs, M))


# The edges the GPU matrix (tests/post_cases.py) adds: chains of no rows (0 / 1000 carried, then divided), chains
# of one row, limits equal to the site index and one off it (with b = -1 and a > b), chains_selected < 0.
EDGES = [("random", 2, 0, 5, 3, 8), ("random", 1, 0, 17, 17, 1), ("random", 2, 0, 4, 6, -2),
         ("random", 7, 1, 6, 5, 3), ("limits", 1, 1, 17, 17, 4), ("limits", 3, 1, 16, 2, 2),
         ("limits", 3, 12, 17, 16, 5), ("limits", 2, 18, 16, 17, 2), ("limits", 5, 5, 9, 7, -3),
         ("extreme", 2, 9, 7, 8, 3)]


@pytest.mark.parametrize("kind,nch,ns,N,M,cs", EDGES)
def test_om_script_matches_literal_loops_at_the_edges(kind, nch, ns, N, M, cs):
    import post_cases
    rng = np.random.default_rng([nch, ns, N, M])
    rec = post_cases.records(kind, N, M, nch, ns, rng)
    rows = post_cases.chain_rows(rec)
    assert len(rows) == nch and all(r.shape == (ns, 2 * M + N) for r in rows)
    if kind == "limits":
        assert post_cases.limit_events(rec, N, M).all()
    X = post_cases.dataset_x("twos", N, M, rng)
    assert same(om_script.pair_order_matrix(rows, cs, N, M), lit_po(rows, cs, N, M))
    assert same(om_script.alive_sum(rows, cs, N, M), lit_site_taxon(rows, cs, N, M, "alive"))
    assert same(om_script.false_alive_sum(rows, cs, N, M), lit_site_taxon(rows, cs, N, M, "false_alive"))
    assert same(om_script.false_ones_sum(rows, cs, X, N, M), lit_site_taxon(rows, cs, N, M, "false_ones", X))
    assert same(om_script.exp_pi(rows, N, cs, M), lit_exp_pi(rows, N, cs, M))
    assert same(om_script.exp_a(rows, cs, M), lit_exp_a(rows, cs, M))


def test_reorder_matches_script_loop():
    rng = np.random.default_rng(5)
    mat = rng.random((7, 5))
    e_pi, e_a = rng.random(7), rng.random(5)
    from seriation_amd import analysis
    assert same(analysis.reorder(mat, e_pi, e_a), om_script.reorder(mat, e_pi, e_a))
