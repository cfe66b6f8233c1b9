"""Per-state moments of the scores under the host simulator (ff_sr_state_moments / ff_sr_state_finish: csrc/ff_sr.h).
CPU only; the symbols are called through simlib.lib() with ctypes (tests/sr_beta_ref.py)."""
import hashlib

import numpy as np
import pytest

from tests import sr_beta_ref as RB
from tests import sr_ref as R
from tests.common import bits_equal
from tests.hostsim import simlib as S

# SHA-256 of the sums ff_sr_moments returns on sr_ref.moment_data(B, P), from the parent commit's sources under the simulator
PARENT_MOMENTS_SHA256 = {
    (1, 24): "492d9cc215fc52ec877a3e04e714d13a72ba1536ebd714b2af727a4454e336b8",
    (5, 36): "70bd9831f54c942c979c1a4446529ed1f0969ad3f6dc960ffc509f8740f5ce0d",
    (4099, 300): "0e389b9a82a4672c3ed50040146d3c6effa7215993820f158b0822756117052e",
    (0, 300): "df09228828575edcbc327fbe458de82880b8f21c38eebeb77382eaeac29a7ea1",
}


@pytest.mark.parametrize("name", RB.IDS)
def test_state_moments(name):
    """Raw sums against numpy.longdouble within the dot-product bounds, counts exact; the finished outputs within the bounds propagated
    from them; fisher exactly symmetric; obar_state of empty states zero; two calls bit-identical.  Case c: the batch split inside a
    state (walker 1000) and at a chunk boundary (2048), the halves' sums added and finished, within 2 x the bounds; the smallest
    eigenvalue of fisher >= -(largest entry of its bound) P."""
    B, P, counts = RB.CASES[name]
    ns = len(counts)
    O, e, ws, me = RB.state_data(name)
    _, sums = RB.sim_state_moments(S, O, e, ws, me)
    assert sums.shape == (RB.sums_len(P, ns),) and np.isfinite(sums).all()
    ref = RB.raw_ref(O, e, ws, me)
    RB.check_raw_sums(sums, ref)
    _, again = RB.sim_state_moments(S, O, e, ws, me)
    assert bits_equal(again, sums)
    f, ob, g = RB.sim_state_finish(S, sums, P, ns)
    if B == 0:
        assert (sums == 0.0).all()
        assert np.isnan(f).all() and np.isnan(g).all() and (ob == 0.0).all()      # a zero count: NaN, as ff_sr_finish gives
        return
    fr = RB.finished_ref(ref)
    RB.check_finished(f, ob, g, fr)
    f2, ob2, g2 = RB.sim_state_finish(S, sums, P, ns)
    assert bits_equal(f2, f) and bits_equal(ob2, ob) and bits_equal(g2, g)
    if name == "d":
        print(f"FIGURES d: max|fisher| {np.abs(f).max():.3e}, largest bound {float(fr['bF'].max()):.3e}")
    if name == "c":
        for cut in (1000, R.SR_CHUNK):
            _, lo = RB.sim_state_moments(S, O[:cut], e[:cut], ws[:cut], me)
            _, hi = RB.sim_state_moments(S, O[cut:], e[cut:], ws[cut:], me)
            both = lo + hi
            assert (RB.split_sums(both, P, ns)[3] == np.asarray(counts)).all()
            RB.check_finished(*RB.sim_state_finish(S, both, P, ns), fr, scale=2.0)
        lam = np.linalg.eigvalsh(f).min()
        bar = -float(fr["bF"].max()) * P
        print(f"FIGURES c: smallest eigenvalue {lam:.3e}, bar {bar:.3e}; fisher error / bound {float((np.abs(f - fr['F']) / fr['bF']).max()):.3f}")
        assert lam >= bar


def test_one_state_is_the_plain_moments():
    """nstates = 1: fisher and grad agree with ff_sr_finish on ff_sr_moments of the same data (e_mean = mean_e[0]) within the sum of
    both bounds.  The baseline is the sample mean, as ff_beta_finish's is: ff_sr_finish removes obar sum(e - E) / B, which then is
    rounding only (eps |E| |obar| / 2, an order below the bounds at these sizes); ff_sr_state_finish takes the baseline as given."""
    B, P = 37, 36
    O, e, _ = R.moment_data(B, P)
    em = float(e.mean())
    ws, me = np.zeros(B, dtype=np.int32), np.array([em])
    _, s1 = RB.sim_state_moments(S, O, e, ws, me)
    f1, ob1, g1 = RB.sim_state_finish(S, s1, P, 1)
    _, s0 = R.sim_moments(S, O, e, em)
    f0, ob0, g0 = R.sim_finish(S, s0, P)
    fr1 = RB.finished_ref(RB.raw_ref(O, e, ws, me))
    fr0 = R.finished_ref(R.moment_ref(O, e, em))
    assert bits_equal(RB.split_sums(s1, P, 1)[0], R.split_sums(s0, P)[0])      # S_raw: the same kernel body
    assert (np.abs(f1 - f0) <= fr1["bF"] + fr0["bF"]).all()
    assert (np.abs(g1 - g0) <= fr1["bG"] + fr0["bG"]).all()
    assert (np.abs(ob1[0] - ob0) <= fr1["bob"][0] + fr0["bob"]).all()


def test_nan_row_poisons_the_sums_it_enters():
    O, e, ws, me = RB.state_data("b")
    O = O.copy()
    O[5, 7] = np.nan      # a walker of state 2
    _, sums = RB.sim_state_moments(S, O, e, ws, me)
    Sr, o, g, c = RB.split_sums(sums, 36, 5)
    assert np.isnan(Sr[7]).all() and np.isnan(Sr[:, 7]).all() and np.isnan(o[2, 7]) and np.isnan(g[7])
    keep = np.ones((5, 36), dtype=bool); keep[2, 7] = False
    assert np.isfinite(o[keep]).all() and (c == RB.CASES["b"][2]).all()


def test_refusals():
    lib = S.lib()
    err = lambda: lib.ff_last_error().decode()
    for P, ns in ((0, 3), (1537, 3), (8, 0)):
        assert lib.ff_sr_state_moments_workspace_bytes(8, P, ns) == 0
        st, sums = RB.sim_state_moments(S, np.ones((8, P)), np.ones(8), np.zeros(8, dtype=np.int32), np.ones(max(ns, 1)), check=False, ns=ns)
        assert st == 2 and err().startswith("ff_sr:"), (P, ns, st, err())
        assert np.isnan(sums).all()      # nothing was launched
        f = np.full(4, 7.0)
        assert lib.ff_sr_state_finish(None, P, ns, S._p(f), S._p(f), S._p(f), S._p(f), S._p(f)) == 2 and err().startswith("ff_sr:")
        assert (f == 7.0).all()
    assert lib.ff_sr_state_moments_workspace_bytes(-1, 300, 3) == 0
    assert lib.ff_sr_state_moments_workspace_bytes(8, 1536, 4096) > 0
    f = np.zeros(8)
    assert lib.ff_sr_state_moments(None, 4, 2, 1, None, S._p(f), S._p(f), S._p(f), S._p(f), S._p(f)) == 1 and err().startswith("ff_sr:")


@pytest.mark.parametrize("B,P", R.MOMENT_CASES, ids=[f"B{B}_P{P}" for B, P in R.MOMENT_CASES])
def test_plain_moments_keep_the_parents_bits(B, P):
    Om, e, em = R.moment_data(B, P)
    _, sums = R.sim_moments(S, Om, e, em)
    assert hashlib.sha256(sums.tobytes()).hexdigest() == PARENT_MOMENTS_SHA256[(B, P)]
