"""Cases of the tabulated flow kernel's walker-group head and tail (csrc/ff_cnf_fwd.hip, MODE 0 and its frames twin),
shared by tests/test_gpu_flow_waves.py and its host-simulator twin tests/test_flow_waves_hostsim.py.

What the register diet touched is lane bookkeeping: a lane's walker, its particle and coordinate, its addresses and its idle-row
value are derived afresh at the head and at the tail of a walker group, the group index is a scalar, and the opening scalars of an
integration (the warm-start step, h0 and d1 of the probe evaluations) sit in a lane-private LDS column.  A slip there shows as a walker
that depends on the slot or the batch it sits in, as a wrong first step, or as a neighbour disturbed by a failing walker.

Shapes: n = 1 .. 6 in two dimensions, 2 and 3 in three; with and without a one-body net; two weight scales -- the benchmark's (golden
g5) and the seeded stiff set at max|w1| = 25, the finest table (h = 1/512, tests/common.py stiff_net).  Batches of 1, G - 1, G, G + 1
and 2 G + 3 walkers (G walkers per wave; the last one leaves a wave a partly filled last group behind two full ones).  Walkers: ordinary
ones, a particle at the origin, two particles 1e-9 apart, a pair radius just below, at and just beyond the table's end (at and beyond:
the off-table event is raised and the direct kernel redoes the call), one non-finite coordinate.

A backend provides, on numpy arrays:
  group(n, d) -> walkers per wave of the tabulated flow kernel
  net(scale, use_mu, table) -> handle of weights(scale, use_mu) (radial table or direct evaluation)
  generate(handle, z, order=None, h_init=None, uniform=False, max_steps=0) -> x, walker_cost, walker_h_out, stats
  frames(handle, z, nframes, order=None) -> frames (nframes, B, n, d)
"""
import numpy as np

from oracle import oracle as O
from tests.common import bits_equal, net_arrays, stiff_net
from tests.flow_radius_cases import AT, BAR_FLOW, OAT, ORT, RT      # the solves and the bar of the existing flow tests, unchanged

SHAPES = [(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (2, 3), (3, 3)]
SCALES = ["bench", "stiff"]
NFRAMES = 3
TAB_RMAX = 32.0                   # csrc/ff_radial.h FF_TAB_RMAX: radii r >= 32 are off the table
STIFF_W = 25.0                    # max|w1| of the finest table, h = 1/512 (tests/common.py STIFF_REGIMES "w25")


def weights(golden, scale, use_mu):
    eta, mu = net_arrays(golden["g5_gsvmc"], "z2_nt_") if scale == "bench" else stiff_net(STIFF_W, seed=1)
    return eta, (mu if use_mu else None)


def batches(G):
    return sorted({B for B in (1, G - 1, G, G + 1, 2 * G + 3) if B >= 1})


def walkers(n, d, B):
    """Ordinary walkers with, where the batch has room, walker 1 holding two particles 1e-9 apart and walker 2 a particle at the
    origin (a one-body radius of exactly 0)."""
    z = np.random.default_rng(1000 * n + d).standard_normal((B, n, d)) * 1.2
    if B > 1 and n > 1:
        z[1, 1] = z[1, 0]
        z[1, 1, 0] += 1e-9
    if B > 2:
        z[2, n - 1] = 0.0
    return z


_REF = {}


def oracle_ref(golden, scale, n, d, use_mu, z):
    """cnf_generate of the oracle at t = 1/2 and 1, computed once per case and shared"""
    key = (scale, n, d, use_mu, z.tobytes())
    if key not in _REF:
        eta, mu = weights(golden, scale, use_mu)
        end, _ = O.cnf_generate(z, O.Net(eta, mu), rtol=ORT, atol=OAT)
        mid, _ = O.cnf_generate(z, O.Net(eta, mu), t0=0.0, t1=0.5, rtol=ORT, atol=OAT)
        _REF[key] = (mid, end)
    return _REF[key]


def slots_case(K, golden, scale, n, d, use_mu, which=None, oracle=True):
    """A walker's x, cost class, walker_h_out and frames do not depend on the batch, the slot or the order it is served in; the first
    G + 1 walkers against the oracle."""
    G = K.group(n, d)
    net = K.net(scale, use_mu, True)
    Bs = batches(G)
    big = Bs[-1]
    z = walkers(n, d, big)
    x, cost, hout, st = K.generate(net, z)
    fr = K.frames(net, z, NFRAMES)
    assert st[3] == 0 and np.isfinite(x).all() and np.isfinite(fr).all() and (cost >= 0).all() and (hout > 0).all()
    assert bits_equal(fr[0], z)
    xe = K.generate(K.net(scale, use_mu, False), z)[0]
    assert not bits_equal(x, xe) or n == 1 and not use_mu          # the table kernel did serve (one particle without a net does not move)
    # the walkers in reverse: every walker in another slot (and, but for the middle one, in another lane group)
    rev = np.ascontiguousarray(z[::-1])
    xr, cr, hr, _ = K.generate(net, rev)
    assert bits_equal(xr[::-1], x) and np.array_equal(cr[::-1], cost) and bits_equal(hr[::-1], hout), (n, d, use_mu, "reversed")
    assert bits_equal(K.frames(net, rev, NFRAMES)[:, ::-1], fr), (n, d, use_mu, "reversed frames")
    # an explicit order
    order = np.ascontiguousarray(np.random.default_rng(big).permutation(big), dtype=np.int32)
    xo, co, ho, _ = K.generate(net, z, order=order)
    assert bits_equal(x, xo) and np.array_equal(cost, co) and bits_equal(ho, hout)
    assert bits_equal(K.frames(net, z, NFRAMES, order=order), fr)
    # a batch and its sub-batches
    for B in (Bs[:-1] if which is None else [Bs[k] for k in which if Bs[k] != big]):
        xs, cs, hs, _ = K.generate(net, z[:B])
        assert bits_equal(xs, x[:B]) and np.array_equal(cs, cost[:B]) and bits_equal(hs, hout[:B]), (n, d, use_mu, B)
        assert bits_equal(K.frames(net, z[:B], NFRAMES), fr[:, :B]), (n, d, use_mu, B, "frames")
    if oracle:
        S = min(big, G + 1)
        mid, end = oracle_ref(golden, scale, n, d, use_mu, z[:S])
        err = float(np.abs(x[:S] - end).max())
        errf = max(float(np.abs(fr[1, :S] - mid).max()), float(np.abs(fr[2, :S] - end).max()))
        print(f"FLOWWAVES {scale} {n}x{d} mu={use_mu} G={G}: generate {err:.2e} frames {errf:.2e} (bar {BAR_FLOW:.0e})")
        assert err < BAR_FLOW and errf < BAR_FLOW, (err, errf)


def warm_case(K, golden, scale, n, d, use_mu):
    """walker_h_uniform and the per-walker warm start both open with the step they were given.  With max_steps = 1 a walker attempts
    one step and stops: 2^-20 (times a factor per walker) is far below what the tolerance asks for, so that step is accepted, and
    walker_h_out -- the largest accepted step -- is then the step given, bit for bit (t = 0, so t + h - t = h exactly).  Without the
    limit the per-walker steps follow the walker through reversal and sub-batches, a uniform step given per walker is the uniform
    call, and the warm-started solve is within the bar of the oracle."""
    G = K.group(n, d)
    if n == 1 and not use_mu:
        return                                                     # v = 0, no radius: nothing to open
    net = K.net(scale, use_mu, True)
    B = 2 * G + 3
    z = walkers(n, d, B)
    h0 = 2.0 ** -20
    hw = h0 * (1.0 + np.arange(B) / B)
    one_u = K.generate(net, z, h_init=np.array([h0]), uniform=True, max_steps=1)
    assert bits_equal(one_u[2], np.full(B, h0)), (n, d, use_mu, one_u[2])
    one_w = K.generate(net, z, h_init=hw, max_steps=1)
    assert bits_equal(one_w[2], hw), (n, d, use_mu, one_w[2], hw)
    assert one_u[3][3] == 1 and one_w[3][3] == 1                   # (the interval is not done after one step of 2^-20: reported as failed)
    xu, cu, hu, su = K.generate(net, z, h_init=np.array([h0]), uniform=True)
    assert su[3] == 0 and np.isfinite(xu).all() and (hu >= h0).all()
    xw, cw, hwo, sw = K.generate(net, z, h_init=hw)
    assert sw[3] == 0 and (hwo >= hw).all()
    xr, cr, hr, _ = K.generate(net, np.ascontiguousarray(z[::-1]), h_init=np.ascontiguousarray(hw[::-1]))
    assert bits_equal(xr[::-1], xw) and np.array_equal(cr[::-1], cw) and bits_equal(hr[::-1], hwo)
    for Bs in sorted({1, G, G + 1}):
        xs, cs, hs, _ = K.generate(net, z[:Bs], h_init=hw[:Bs])
        assert bits_equal(xs, xw[:Bs]) and np.array_equal(cs, cw[:Bs]) and bits_equal(hs, hwo[:Bs]), (n, d, use_mu, Bs)
    xq, cq, hq, _ = K.generate(net, z, h_init=np.full(B, h0))
    assert bits_equal(xq, xu) and np.array_equal(cq, cu) and bits_equal(hq, hu)
    S = min(B, G + 1)
    _, end = oracle_ref(golden, scale, n, d, use_mu, z[:S])
    err = max(float(np.abs(xu[:S] - end).max()), float(np.abs(xw[:S] - end).max()))
    print(f"FLOWWAVES warm {scale} {n}x{d} mu={use_mu}: {err:.2e} (bar {BAR_FLOW:.0e})")
    assert err < BAR_FLOW, err


def special_case(K, golden, scale, n, d, use_mu):
    """A pair (or one-body) radius just below the table's end is served and within the bar of the oracle; at the end and just beyond it
    the whole call is the direct kernel's, bit for bit.  A non-finite coordinate: that walker is NaN, every other walker of its wave
    is what it is without it."""
    G = K.group(n, d)
    B = 2 * G + 3
    z = walkers(n, d, B)
    net, exact = K.net(scale, use_mu, True), K.net(scale, use_mu, False)
    k = B // 2
    if n > 1 or use_mu:
        for r0, off in ((np.nextafter(TAB_RMAX, 0.0), False), (TAB_RMAX, True), (np.nextafter(TAB_RMAX, 64.0), True)):
            far = z.copy()
            far[k] = 0.0
            if n > 1:                                              # the pair (0, 1) at distance r0, both inside one-body radius 16
                far[k, 0, 0], far[k, 1, 0] = -0.5 * r0, 0.5 * r0
                far[k, 2:, d - 1] = 1.0 + np.arange(n - 2)
                assert far[k, 1, 0] - far[k, 0, 0] == r0
            else:
                far[k, 0, 0] = r0
            xt, ct, ht, stt = K.generate(net, far)
            xd, cd, hd, std = K.generate(exact, far)
            assert std[3] == 0 and np.isfinite(xd).all()
            if off:
                assert bits_equal(xt, xd) and np.array_equal(ct, cd) and bits_equal(ht, hd), (n, d, use_mu, r0)
                assert bits_equal(K.frames(net, far, NFRAMES), K.frames(exact, far, NFRAMES)), (n, d, use_mu, r0, "frames")
            else:                                                  # served by whichever kernel the flow's own motion leaves it to
                assert stt[3] == 0 and float(np.abs(xt - xd).max()) < BAR_FLOW, (n, d, use_mu, r0)
    x = K.generate(net, z)[0]
    fr = K.frames(net, z, NFRAMES)
    bad = z.copy()
    kb = min(B - 1, G // 2 + 1)
    bad[kb, 0, d - 1] = np.nan
    xn = K.generate(net, bad)[0]
    frn = K.frames(net, bad, NFRAMES)
    keep = np.arange(B) != kb
    assert bits_equal(xn[keep], x[keep]) and bits_equal(frn[:, keep], fr[:, keep]), (n, d, use_mu)
    assert not np.isfinite(xn[kb]).all() and not np.isfinite(frn[NFRAMES - 1, kb]).all()
    if n > 1 or use_mu:                                           # (one particle without a one-body net has no radius: v = 0, nothing fails)
        assert np.isnan(xn[kb]).all() and np.isnan(frn[NFRAMES - 1, kb]).all()
