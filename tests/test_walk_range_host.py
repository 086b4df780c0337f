"""The fixed scale of the 9-word Gibbs walks, modelled on the host (no GPU).

draw_fast_s<9> (csrc/sr_device.hip) sums every entry of the walk from y = 1 at walk entry 0, without a window.  The
model below is that chain entry by entry in numpy f64 -- y(w + 1) = y(w) r(bit w), S summed in order -- with the
certification of walk_pick_s (REL = (N + 33) 2^-50, ABS = (N + 1) 2^-39).  On the extreme columns of
tests/walk_range_cases.py, at the largest 9-word shape (N = 287) and at N = 256, at the four corners of the (c, d)
bounds:
  * no certified pick differs from the oracle's (oracle_auxa_pick);
  * at least 1/7 of the cases are certified (the share tests/test_gpu_cert.py asks of the device);
  * the two bounds the missing window rests on hold numerically: every y < 2^667, and every y computed after the
    chain sank below 2^-1022 is <= 2^-355.
"""
import numpy as np
import pytest

import cert_cases
import oracle_ref
import walk_range_cases as wr


def chain(x, c, d):
    """y[0..L] and its running sums P[0..L] for walk bits x: y[0] = 1, a zero multiplies by rA = e^(cc - d), a one
    by rB = e^(c - dd) (cc = log(1 - e^c), dd = log(1 - e^d), the device's K)."""
    e = oracle_ref.exp_log(np.array([c, d]))[0]
    cc, dd = (float(v) for v in oracle_ref.exp_log(1.0 - e)[1])
    rA, rB = (float(v) for v in oracle_ref.exp_log(np.array([cc - d, c - dd]))[0])
    y = np.ones(len(x) + 1)
    for w, bit in enumerate(x):
        y[w + 1] = y[w] * (rB if bit else rA)
    return y, np.cumsum(y), rA


def model_pick(P, N, u):
    """walk_pick_s on the entry sums P: the entry where u S falls, or -1 when it is not certified."""
    L = len(P) - 1
    S = P[L]
    inv = 1.0 / S
    REL = (N + 33) * 2.0 ** -50
    ABS = (N + 1) * 2.0 ** -39
    w = int(np.count_nonzero(P[:L] < u * S))
    Ph, Pp = P[w], (P[w - 1] if w else 0.0)
    t, tprev = u - Ph * inv, u - Pp * inv
    e = 2.0 * REL * min(Ph, S - Ph) * inv + ABS
    eprev = 2.0 * REL * min(Pp, S - Pp) * inv + ABS
    return w if (w == 0 or tprev > eprev) and (w == L or t < -e) else -1


@pytest.mark.parametrize("N", [287, 256])
def test_fixed_scale_chain_certifies_only_the_oracles_picks(N):
    cs = wr.extreme_cases(N)
    chains = {}
    certified = wrong = 0
    ymax, ydown, dips = 0.0, 0.0, 0
    for k in range(cs["n"]):
        c, d = (float(v) for v in cs["cd"][k // 64])
        key = (int(cs["cidx"][k]), c, d)
        if key not in chains:
            x = cert_cases.walk_bits(cs["cols"][key[0]], N, False, int(cs["L"][k]))
            y, P, rA = chain(x, c, d)
            assert np.log2(rA) <= 2.322   # d >= 0.2, c <= 0.1
            assert P[-1] >= 1.0
            chains[key] = P
            ymax = max(ymax, float(y.max()))
            low = np.nonzero(y < 2.0 ** -1022)[0]
            if len(low):
                dips += 1
                ydown = max(ydown, float(y[low[0]:].max()))
        got = model_pick(chains[key], N, float(cs["u"][k]))
        if got >= 0:
            certified += 1
            wrong += got != int(cs["expected"][k])
    print("N=%d cases=%d certified=%d wrong=%d log2(max y)=%.1f dipped chains=%d log2(max y after a dip)=%s"
          % (N, cs["n"], certified, wrong, np.log2(ymax), dips, np.log2(ydown) if ydown > 0 else "-inf"))
    assert wrong == 0
    assert certified >= cs["n"] // 7
    assert ymax < 2.0 ** 667
    assert dips > 0, "no column takes the chain below 2^-1022: the second bound is not exercised"
    assert ydown <= 2.0 ** -355
