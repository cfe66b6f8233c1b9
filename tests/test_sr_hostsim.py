"""Per-walker scores and their moments under the host simulator (ff_cnf_adjoint_scores: csrc/ff_cnf_adj.hip and
ff_adj_direct_body.inc with SCORES; ff_sr_moments / ff_sr_finish: csrc/ff_sr.h).  CPU only; the symbols are called
through simlib.lib() with ctypes (tests/sr_ref.py)."""

import numpy as np
import pytest

from oracle import oracle as O
from tests import sr_ref as R
from tests.common import bits_equal, net_arrays
from tests.hostsim import simlib as S

_CACHE = {}
shapes = pytest.mark.parametrize("n,d,B", R.SHAPES, ids=R.IDS)
with_mu = pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])


def _nets(golden, use_mu):
    """(simulator net without a radial table, oracle net) of the benchmark's weights (g3_backflow.npz, c1_)"""
    key = ("net", use_mu)
    if key not in _CACHE:
        eta, mu = net_arrays(golden["g3_backflow"], "c1_", use_mu)
        _CACHE[key] = (S.Net(eta, mu), O.Net(eta, mu))
    return _CACHE[key]


def _case(golden, n, d, B, use_mu, tol):
    """walkers, z(t0), Delta, glogp0 and the scores of a shape: computed once, shared, never written to"""
    key = ("case", n, d, B, use_mu, tol["rtol"])
    if key not in _CACHE:
        net, _ = _nets(golden, use_mu)
        z, dl, g0 = R.sim_flow_end(S, R.walkers(n, d, B), net, tol)
        _, sc, st = R.sim_scores(S, z, g0, net, tol)
        for a in (z, dl, g0, sc):
            a.setflags(write=False)
        _CACHE[key] = (z, dl, g0, sc, st)
    return _CACHE[key]


@with_mu
@shapes
def test_rows_are_the_one_walker_adjoints_bit_for_bit(golden, n, d, B, use_mu):
    """Row b of the scores is, bit for bit, grad_params of the existing ff_cnf_adjoint called on walker b alone (radial_table = NULL,
    seeds glogp0[b] and -1, the same ff_ode); stats[0] and stats[2] are the sums over those calls; a walker_order that reverses the
    walkers changes nothing."""
    net, _ = _nets(golden, use_mu)
    z, _, g0, sc, st = _case(golden, n, d, B, use_mu, R.LOOSE)
    assert st[3] == 0 and np.isfinite(sc).all()
    nev = nrej = 0
    for b in range(B):
        gp, s1 = R.sim_adjoint_one(S, z, g0, net, R.LOOSE, b)
        assert bits_equal(sc[b], gp), (b, np.abs(sc[b] - gp).max())
        nev += int(s1[0]); nrej += int(s1[2])
    assert (int(st[0]), int(st[2])) == (nev, nrej)
    order = np.arange(B - 1, -1, -1, dtype=np.int32)
    _, sc_r, st_r = R.sim_scores(S, z, g0, net, R.LOOSE, order=order)
    assert bits_equal(sc_r, sc)
    assert (st_r == st).all()


def test_wide_net_takes_one_launch_per_unit_chunk():
    """He = Hm = 100 at 6 coordinates: 66 hidden units per unit0 chunk, so that loop runs twice (each chunk in blocks of five units per lane) -- rows still bit for bit"""
    n, d, B = R.WIDE_NET_SHAPE
    eta, mu = R.wide_net_arrays()
    net = S.Net(eta, mu)
    z, _, g0 = R.sim_flow_end(S, R.walkers(n, d, B), net, R.LOOSE)
    _, sc, st = R.sim_scores(S, z, g0, net, R.LOOSE)
    assert sc.shape == (B, 600) and np.isfinite(sc).all() and (np.abs(sc).max(axis=0) > 0).all()
    nev = 0
    for b in range(B):
        gp, s1 = R.sim_adjoint_one(S, z, g0, net, R.LOOSE, b)
        assert bits_equal(sc[b], gp), b
        nev += int(s1[0])
    assert int(st[0]) == nev


@with_mu
@shapes
def test_scores_against_oracle(golden, n, d, B, use_mu):
    """At rtol 1e-10 / atol 1e-12 against oracle.cnf_adjoint walker by walker; the error of a row is relative to that row's largest
    |entry|.  Bar: 4 x the largest such error of the EXISTING direct ff_cnf_adjoint (B = 1 calls) against the same oracle calls on
    the same walkers, measured here first -- per shape, which asks no less than the largest over the shapes.  The largest figures
    as measured under the simulator are in tests/sr_ref.py (YARDSTICK_HOSTSIM, SCORES_HOSTSIM)."""
    net, onet = _nets(golden, use_mu)
    z, dl, g0, sc, _ = _case(golden, n, d, B, use_mu, R.TIGHT)
    yard = worst = 0.0
    for b in range(B):
        _, ref, _ = O.cnf_adjoint(z[b:b + 1], dl[b:b + 1], g0[b:b + 1], np.array([-1.0]), onet, t0=R.T0, t1=R.T1, **R.TIGHT)
        gp, _ = R.sim_adjoint_one(S, z, g0, net, R.TIGHT, b)
        yard = max(yard, R.row_rel_err(gp, ref))
        worst = max(worst, R.row_rel_err(sc[b], ref))
    print(f"FIGURES {n}x{d} mu={use_mu}: existing direct adjoint against the oracle {yard:.3e}; scores {worst:.3e}; bar {4 * yard:.3e}")
    assert yard > 0.0
    assert worst <= 4 * yard, (worst, yard)


@pytest.mark.parametrize("n,d,B", [(3, 2, 11), (3, 3, 8)], ids=["3x2_B11", "3x3_B8"])
def test_non_finite_walker_gives_a_nan_row_and_leaves_the_others(golden, n, d, B):
    net, _ = _nets(golden, True)
    z, _, g0, sc, _ = _case(golden, n, d, B, True, R.LOOSE)
    zb = z.copy()
    bad = 1      # (inside the first group, with neighbours on both sides)
    zb[bad, n - 1, 0] = np.inf
    _, sb, st = R.sim_scores(S, zb, g0, net, R.LOOSE)
    assert np.isnan(sb[bad]).all()
    keep = np.arange(B) != bad
    assert bits_equal(sb[keep], sc[keep])
    assert st[3] == 1


def test_refusals(golden):
    net, _ = _nets(golden, True)
    lib = S.lib()
    err = lambda: lib.ff_last_error().decode()
    for n, d in ((13, 2), (5, 3)):
        z = R.walkers(n, d, 2)
        st, sc, _ = R.sim_scores(S, z, z, net, R.LOOSE, check=False)
        assert st == 2 and err().startswith("ff_scores:"), (st, err())
        assert (sc == 7.0).all()      # nothing was launched
    z = R.walkers(3, 2, 2)
    prev = lib.ff_set_kernel_family(1)
    try:
        st, sc, _ = R.sim_scores(S, z, z, net, R.LOOSE, check=False)
    finally:
        lib.ff_set_kernel_family(prev)
    assert st == 2 and err().startswith("ff_scores:") and (sc == 7.0).all()
    st, _, _ = R.sim_scores(S, z, z, net, R.LOOSE, check=False, null_scores=True)
    assert st == 1 and err().startswith("ff_scores:")
    st, sc, _ = R.sim_scores(S, z[:0], z[:0], net, R.LOOSE)      # B = 0: a no-op
    assert st == 0
    for P in (0, 1537):
        assert lib.ff_sr_moments_workspace_bytes(8, P) == 0
        st, sums = R.sim_moments(S, np.ones((8, P)), np.ones(8), 0.0, check=False)
        assert st == 2 and err().startswith("ff_sr:"), (P, st, err())
        assert np.isnan(sums).all()
    assert lib.ff_sr_moments_workspace_bytes(-1, 300) == 0
    assert lib.ff_sr_moments_workspace_bytes(8, 1536) > 0
    f = np.zeros(4)
    assert lib.ff_sr_finish(None, 0, S._p(f), S._p(f), S._p(f), S._p(f)) == 2 and err().startswith("ff_sr:")
    assert lib.ff_sr_moments(None, 4, 2, None, S._p(f), S._p(f), S._p(f), S._p(f)) == 1 and err().startswith("ff_sr:")


@pytest.mark.parametrize("B,P", R.MOMENT_CASES, ids=[f"B{B}_P{P}" for B, P in R.MOMENT_CASES])
def test_moments(B, P):
    """Raw sums against numpy.longdouble within the dot-product bound; the finished outputs within the bounds propagated from it;
    fisher exactly symmetric; two calls bit-identical; the walkers split at a chunk boundary, the halves' sums added and finished:
    within 2 x the bound."""
    Om, e, em = R.moment_data(B, P)
    _, sums = R.sim_moments(S, Om, e, em)
    assert np.isfinite(sums).all()
    if B == 0:
        assert (sums == 0.0).all()
        return
    ref = R.moment_ref(Om, e, em)
    R.check_raw_sums(sums, ref, P)
    fr = R.finished_ref(ref)
    R.check_finished(*R.sim_finish(S, sums, P), fr)
    _, again = R.sim_moments(S, Om, e, em)
    assert bits_equal(again, sums)
    if B > R.SR_CHUNK:
        _, lo = R.sim_moments(S, Om[:R.SR_CHUNK], e[:R.SR_CHUNK], em)
        _, hi = R.sim_moments(S, Om[R.SR_CHUNK:], e[R.SR_CHUNK:], em)
        R.check_finished(*R.sim_finish(S, lo + hi, P), fr, scale=2.0)


def test_nan_row_is_not_masked():
    Om, e, em = R.moment_data(5, 36)
    Om[3, 7] = np.nan
    _, sums = R.sim_moments(S, Om, e, em)
    Sr, o, g, se, cnt = R.split_sums(sums, 36)
    assert np.isnan(Sr[7]).all() and np.isnan(Sr[:, 7]).all() and np.isnan(o[7]) and np.isnan(g[7])
    assert np.isfinite(o[np.arange(36) != 7]).all() and np.isfinite(se) and cnt == 5
