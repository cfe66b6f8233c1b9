"""ff_cnf_generate_frames (CNF.generate(z, nframes): csrc/ff_cnf_fwd.hip, csrc/ff_wide.hip) under the host
simulator: the frame-writing instantiations of the two flow kernels against the project's own ff_cnf_generate over (t0, t_k).
CPU only; the symbol is called through simlib.lib() with ctypes directly (tests/frames_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import frames_ref as F
from tests.common import bits_equal, net_arrays
from tests.hostsim import simlib as S

SHAPES = F.HOSTSIM_SHAPES
IDS = [f"{n}x{d}_B{B}" for n, d, B in SHAPES]
_CACHE = {}


def _net(golden, use_mu, table):
    """the benchmark's weights (tests/golden/g3_backflow.npz, c1_), with or without mu"""
    key = ("net", use_mu, table)
    if key not in _CACHE:
        eta, mu = net_arrays(golden["g3_backflow"], "c1_", use_mu)
        _CACHE[key] = S.Net(eta, mu, table=table)
    return _CACHE[key]


def _generate(golden, use_mu, table, n, d, B, t1, tol):
    """ff_cnf_generate over (t0, t1) on the walkers of a shape: computed once, shared, never written to"""
    key = ("gen", use_mu, table, n, d, B, t1, tol["rtol"])
    if key not in _CACHE:
        x, st = S.cnf_generate(F.walkers(n, d, B), _net(golden, use_mu, table), t0=F.T0, t1=t1, **tol)
        x.setflags(write=False)
        _CACHE[key] = (x, st)
    return _CACHE[key]


both = pytest.mark.parametrize("table", [True, False], ids=["table", "direct"])
with_mu = pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
shapes = pytest.mark.parametrize("n,d,B", SHAPES, ids=IDS)


@both
@with_mu
@shapes
def test_frame_zero_and_two_frames(golden, n, d, B, use_mu, table):
    """Cases 1 and 2: frames[0] is z bit for bit; with nframes = 2 the only frame time is the end of the interval, nothing is
    shortened, and frames[1] and the stats are those of ff_cnf_generate bit for bit -- the new instantiation is the old integration."""
    z = F.walkers(n, d, B)
    net = _net(golden, use_mu, table)
    x, st = _generate(golden, use_mu, table, n, d, B, F.T1, F.LOOSE)
    _, fr, stf = F.sim_frames(S, z, net, 2, **F.LOOSE)
    assert bits_equal(fr[0], z)
    assert bits_equal(fr[1], x)
    assert (stf == st).all(), (stf, st)
    _, fr5, _ = F.sim_frames(S, z, net, 5, **F.LOOSE)
    assert bits_equal(fr5[0], z)


def _frames_against_generate(golden, n, d, B, use_mu, table, nframes, tol):
    z = F.walkers(n, d, B)
    _, fr, st = F.sim_frames(S, z, _net(golden, use_mu, table), nframes, **tol)
    assert st[3] == 0 and np.isfinite(fr).all()
    worst = 0.0
    for k, tk in enumerate(F.frame_times(nframes)):
        if k == 0:
            continue
        xk, _ = _generate(golden, use_mu, table, n, d, B, tk, tol)
        worst = max(worst, float(np.abs(fr[k] - xk).max()))
    return worst


@both
@with_mu
@shapes
def test_each_frame_against_generate_tight(golden, n, d, B, use_mu, table):
    """Case 3: nframes = 5 at rtol = 1e-10, atol = 1e-12, every frames[k] against ff_cnf_generate over (t0, t_k) at the same
    tolerances.  Bar: 4 x the largest difference between one unchanged ff_cnf_generate over (t0, t1) and two chained ones over
    (t0, t1/2), (t1/2, t1) on these walkers -- measured 1.5348e-12 (3 particles in d = 3, B = 9, direct kernel, no mu): bar 6.139e-12.
    Measured for the frames: at most 1.22e-12 (3 x 2, B = 13, no mu)."""
    worst = _frames_against_generate(golden, n, d, B, use_mu, table, F.NF_TIGHT, F.TIGHT)
    print(f"frames vs generate, tight: {worst:.3e} (bar {F.BAR_TIGHT:.3e})")
    assert worst <= F.BAR_TIGHT, worst


@both
@with_mu
@shapes
def test_each_frame_against_generate_default_tolerances(golden, n, d, B, use_mu, table):
    """Case 4: nframes = 9 at the defaults 1e-6 / 1e-8.  Bar derived as in case 3: one solve against two chained ones differs by at
    most 7.8626e-08 (3 particles in d = 3, B = 9, direct kernel, with mu): bar 3.145e-07.  Measured for the frames: at most 2.17e-07 (6 x 2, B = 7, no mu)."""
    worst = _frames_against_generate(golden, n, d, B, use_mu, table, F.NF_LOOSE, F.LOOSE)
    print(f"frames vs generate, defaults: {worst:.3e} (bar {F.BAR_LOOSE:.3e})")
    assert worst <= F.BAR_LOOSE, worst


def test_bars_are_four_times_the_split_of_one_solve(golden):
    """The constants of tests/frames_ref.py, measured again from ff_cnf_generate alone: the largest difference between one solve
    and two chained ones over every shape, table and direct, with and without mu, is the recorded figure (to 2 %: the figure moves
    in its last digits with the host's libm), and the bars are exactly 4 x the recorded figures."""
    worst = {"tight": 0.0, "loose": 0.0}
    half = 0.5 * (F.T0 + F.T1)
    for n, d, B in SHAPES:
        for use_mu in (True, False):
            for table in (True, False):
                for name, tol in (("tight", F.TIGHT), ("loose", F.LOOSE)):
                    x1, _ = _generate(golden, use_mu, table, n, d, B, F.T1, tol)
                    xh, _ = _generate(golden, use_mu, table, n, d, B, half, tol)
                    xc, _ = S.cnf_generate(xh, _net(golden, use_mu, table), t0=half, t1=F.T1, **tol)
                    worst[name] = max(worst[name], float(np.abs(x1 - xc).max()))
    print(worst)
    assert abs(worst["tight"] / F.SPLIT_TIGHT - 1.0) < 0.02, worst
    assert abs(worst["loose"] / F.SPLIT_LOOSE - 1.0) < 0.02, worst
    assert F.BAR_TIGHT == 4 * F.SPLIT_TIGHT and F.BAR_LOOSE == 4 * F.SPLIT_LOOSE


@both
@shapes
def test_walker_order_does_not_change_a_bit(golden, n, d, B, table):
    """Case 5: with a walker_order permutation the frames are bit-identical to those without it."""
    z = F.walkers(n, d, B)
    net = _net(golden, True, table)
    _, fr, st = F.sim_frames(S, z, net, 4, **F.LOOSE)
    order = np.ascontiguousarray(np.random.default_rng(B).permutation(B), dtype=np.int32)
    _, fro, sto = F.sim_frames(S, z, net, 4, order=order, **F.LOOSE)
    assert bits_equal(fro, fr) and (sto == st).all()


@shapes
def test_off_table_walker_redoes_every_frame(golden, n, d, B):
    """Case 6: one walker with a particle at radius 40 (the table ends at 32).  The table kernel posts its launch id and the
    direct kernel behind it rewrites every frame of every walker: the result is the direct call's bit for bit."""
    z = F.walkers(n, d, B).copy()
    z[B // 2, 0] = 0.0
    z[B // 2, 0, 0] = 40.0
    _, ft, stt = F.sim_frames(S, z, _net(golden, True, True), 4, **F.LOOSE)
    _, fd, std = F.sim_frames(S, z, _net(golden, True, False), 4, **F.LOOSE)
    assert np.isfinite(fd).all() and std[3] == 0
    assert bits_equal(ft, fd)


@both
@shapes
def test_failed_walkers_have_a_nan_suffix(golden, n, d, B, table):
    """Case 7: max_steps = 3 at tolerances where every walker needs more steps than that.  Frame 0 is z, the last frame is NaN
    for every walker, the NaN frames of a walker form a suffix (whole frames: every coordinate), and stats[3] is set."""
    tol = dict(rtol=1e-12, atol=1e-14)
    z = F.walkers(n, d, B)
    net = _net(golden, True, table)
    _, need = S.cnf_generate(z, net, **tol)
    assert need[1] > 3 and need[3] == 0                  # (the walkers do need more steps, and get there with them)
    S.warm(max_steps=3)
    try:
        _, fr, st = F.sim_frames(S, z, net, 4, **tol)
    finally:
        S.warm()
    assert st[3] != 0
    assert bits_equal(fr[0], z)
    nan = np.isnan(fr).reshape(4, B, -1)
    assert (nan.all(2) == nan.any(2)).all()              # a frame of a walker is NaN as a whole or not at all
    nanf = nan.all(2)                                    # (frame, walker)
    assert nanf[3].all() and not nanf[0].any()
    assert (np.diff(nanf.astype(int), axis=0) >= 0).all()      # once NaN, NaN in every later frame
    # what a walker did reach before it ran out of steps is the unbounded call's frame
    _, full, _ = F.sim_frames(S, z, net, 4, **tol)
    ok = ~nan
    assert bits_equal(fr[ok.reshape(fr.shape)], full[ok.reshape(fr.shape)])


def test_refusals_and_the_single_frame(golden):
    """Case 8: status codes and message prefix of the refusals (all before any launch); nframes = 1 copies z and integrates nothing."""
    lib = S.lib()
    net = _net(golden, True, False)
    z = F.walkers(6, 2, 4)
    out = np.full((2, 4, 6, 2), 7.0)
    stats = np.zeros(4, dtype=np.int32)
    ode = S._ode(0.0, 1.0, 1e-6, 1e-8)

    def call(B, n, d, zp, nframes, fp, netc=net.c, odec=ode):
        return lib.ff_cnf_generate_frames(None, B, n, d, C.byref(netc), C.byref(odec), zp, nframes, fp, S._p(stats))

    def refused(st, code):
        assert st == code and lib.ff_last_error().decode().startswith("ff_cnf_generate_frames:"), (st, lib.ff_last_error())

    refused(call(4, 6, 2, S._p(z), 0, S._p(out)), 1)                 # FF_EINVAL: nframes < 1
    refused(call(4, 6, 2, S._p(z), -3, S._p(out)), 1)
    refused(call(4, 6, 2, S._p(z), 2, None), 1)                      # null frames
    refused(call(4, 6, 2, None, 2, S._p(out)), 1)                    # null z
    refused(call(-1, 6, 2, S._p(z), 2, S._p(out)), 1)                # B < 0
    refused(call(4, 25, 2, S._p(z), 2, S._p(out)), 2)                # FF_EUNSUPPORTED: what ff_cnf_generate refuses
    refused(call(4, 21, 3, S._p(z), 2, S._p(out)), 2)
    refused(call(4, 25, 2, S._p(z), 1, S._p(out)), 2)                # ... also where nothing would be integrated
    refused(call(4, 6, 2, S._p(z), 2, S._p(out), odec=S._ode(0.0, 1.0, 0.0, 1e-8)), 1)
    assert (out == 7.0).all() and not stats.any()                    # nothing was launched
    assert call(0, 6, 2, S._p(z), 2, S._p(out)) == 0                 # B = 0: a no-op
    assert (out == 7.0).all()
    for table in (False, True):
        st, fr, stats1 = F.sim_frames(S, z, _net(golden, True, table), 1)
        assert st == 0 and fr.shape[0] == 1 and bits_equal(fr[0], z) and stats1[0] == 0 and not stats1.any()


def test_empty_interval_repeats_the_state(golden):
    """t0 = t1: every frame time is t0 and every frame is z (torch.linspace(t0, t0, K))."""
    z = F.walkers(6, 2, 7)
    for table in (False, True):
        _, fr, st = F.sim_frames(S, z, _net(golden, True, table), 3, t0=0.3, t1=0.3)
        assert all(bits_equal(fr[k], z) for k in range(3)) and st[3] == 0
    z = F.walkers(13, 2, 3)
    _, fr, st = F.sim_frames(S, z, _net(golden, True, True), 3, t0=0.3, t1=0.3)
    assert all(bits_equal(fr[k], z) for k in range(3)) and st[3] == 0


def test_backward_interval_lands_on_descending_frame_times(golden):
    """t1 < t0 (the direction delta_logp integrates in): frames at t0 + k (t1 - t0) / (K - 1), the last one the plain call's."""
    z = F.walkers(3, 2, 13)
    net = _net(golden, True, True)
    _, fr, _ = F.sim_frames(S, z, net, 3, t0=1.0, t1=0.0, **F.TIGHT)
    xm, _ = S.cnf_generate(z, net, t0=1.0, t1=0.5, **F.TIGHT)
    xe, _ = S.cnf_generate(z, net, t0=1.0, t1=0.0, **F.TIGHT)
    assert np.abs(fr[1] - xm).max() <= F.BAR_TIGHT and np.abs(fr[2] - xe).max() <= F.BAR_TIGHT
