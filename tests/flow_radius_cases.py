"""Cases of the tabulated flow kernel's radius and component phases (csrc/ff_cnf_fwd.hip, MODE 0 and its frames twin),
shared by tests/test_gpu_flow_radius.py and its host-simulator twin tests/test_flow_radius_hostsim.py.

What the instruction diet touched: the partner of a one-body radius and the head of a particle's term with itself are read from a
slot of +0.0 through a per-lane address, the table row is fetched without a branch (index clamped, `ok` a predicate) and the off-table
event is raised from that predicate.  The cases: one, several and the largest number of walkers per wave (n = 1 .. 6 in two dimensions,
2 and 4 in three: an empty second radius slot and a half-full one), with and without a one-body net, batches of 1, G - 1, G + 1 and
2 G + 3 walkers (G walkers per wave), an explicit walker order; ordinary walkers, two coincident particles (r = 0), a particle at the
origin, a radius beyond the table (the direct-evaluation kernel redoes the whole call), a NaN coordinate.

A backend provides, on numpy arrays:
  group(n, d) -> walkers per wave of the tabulated flow kernel
  net(use_mu, table) -> handle of the weights below (radial table or direct evaluation)
  generate(handle, z, order) -> x, walker_cost, walker_h_out, stats
  frames(handle, z, nframes, order) -> frames (nframes, B, n, d)
"""
import numpy as np

from oracle import oracle as O
from tests.common import bits_equal, net_arrays
from tests.test_gpu_geometry import AT, BAR_FLOW, OAT, ORT, RT      # the solves and the bar of test_flow_at_looping_batch_vs_oracle

SHAPES = [(1, 2), (2, 2), (3, 2), (5, 2), (6, 2), (2, 3), (4, 3)]
NFRAMES = 3


def weights(golden, use_mu):
    eta, mu = net_arrays(golden["g5_gsvmc"], "z2_nt_")
    return eta, (mu if use_mu else None)


def batches(G):
    return sorted({B for B in (1, G - 1, G + 1, 2 * G + 3) if B >= 1})


def walkers(n, d, B):
    """Ordinary walkers with, where the batch has room, walker 1 holding two coincident particles (r = 0) and walker 2 a particle
    at the origin (a one-body radius of 0)."""
    z = np.random.default_rng(100 * n + d).standard_normal((B, n, d)) * 1.2
    if B > 1 and n > 1:
        z[1, 1] = z[1, 0]
    if B > 2:
        z[2, n - 1] = 0.0
    return z


def flow_case(K, golden, n, d, use_mu, which=None, oracle=True):
    G = K.group(n, d)
    net = K.net(use_mu, True)
    Bs = batches(G)
    big = Bs[-1]
    z = walkers(n, d, big)
    x, cost, hout, st = K.generate(net, z, None)
    fr = K.frames(net, z, NFRAMES, None)
    assert st[3] == 0 and np.isfinite(x).all() and np.isfinite(fr).all() and (cost >= 0).all() and (hout > 0).all()
    assert bits_equal(fr[0], z)
    # the direct-evaluation kernel differs in the last bits: the table kernel did serve
    xe = K.generate(K.net(use_mu, False), z, None)[0]
    assert not bits_equal(x, xe) or n == 1 and not use_mu          # (one particle without a one-body net does not move)
    # an explicit order: not a bit
    order = np.ascontiguousarray(np.random.default_rng(big).permutation(big), dtype=np.int32)
    xo, co, ho, _ = K.generate(net, z, order)
    assert bits_equal(x, xo) and np.array_equal(cost, co) and bits_equal(ho, hout)
    assert bits_equal(K.frames(net, z, NFRAMES, order), fr)
    # a batch and its sub-batches
    for B in (Bs[:-1] if which is None else [Bs[k] for k in which]):
        xs, cs, hs, _ = K.generate(net, z[:B], None)
        assert bits_equal(xs, x[:B]) and np.array_equal(cs, cost[:B]) and bits_equal(hs, hout[:B]), (n, d, use_mu, B)
        assert bits_equal(K.frames(net, z[:B], NFRAMES, None), fr[:, :B]), (n, d, use_mu, B, "frames")
    if oracle:
        S = min(big, G + 1)
        eta, mu = weights(golden, use_mu)
        ref, _ = O.cnf_generate(z[:S], O.Net(eta, mu), rtol=ORT, atol=OAT)
        err = float(np.abs(x[:S] - ref).max())
        mid, _ = O.cnf_generate(z[:S], O.Net(eta, mu), t0=0.0, t1=0.5, rtol=ORT, atol=OAT)
        errf = max(float(np.abs(fr[1, :S] - mid).max()), float(np.abs(fr[2, :S] - ref).max()))
        print(f"FLOWRAD {n}x{d} mu={use_mu} G={G}: generate {err:.2e} frames {errf:.2e} (bar {BAR_FLOW:.0e})")
        assert err < BAR_FLOW and errf < BAR_FLOW, (err, errf)


def special_case(K, golden, n, d, use_mu):
    """A radius beyond the table: the whole call is the direct-evaluation kernel's, bit for bit.  A NaN coordinate: that walker is NaN,
    every other walker of its wave is what it is without it."""
    G = K.group(n, d)
    B = 2 * G + 3
    z = walkers(n, d, B)
    net, exact = K.net(use_mu, True), K.net(use_mu, False)
    far = z.copy()
    far[B // 2, 0] = 0.0
    far[B // 2, 0, 0] = 40.0                                  # a one-body radius of 40, pair distances beyond 32 where there are pairs
    if n > 1 or use_mu:
        xt, ct, ht, stt = K.generate(net, far, None)
        xd, cd, hd, std = K.generate(exact, far, None)
        assert std[3] == 0 and np.isfinite(xd).all()
        assert bits_equal(xt, xd) and np.array_equal(ct, cd) and bits_equal(ht, hd)
        assert bits_equal(K.frames(net, far, NFRAMES, None), K.frames(exact, far, NFRAMES, None))
    x = K.generate(net, z, None)[0]
    fr = K.frames(net, z, NFRAMES, None)
    bad = z.copy()
    k = min(B - 1, G // 2 + 1)
    bad[k, 0, d - 1] = np.nan
    xn = K.generate(net, bad, None)[0]
    frn = K.frames(net, bad, NFRAMES, None)
    keep = np.arange(B) != k
    assert bits_equal(xn[keep], x[keep]) and bits_equal(frn[:, keep], fr[:, keep])
    if n > 1 or use_mu:                                       # (one particle without a one-body net has no radius: v = 0, nothing fails)
        assert np.isnan(xn[k]).all() and np.isnan(frn[NFRAMES - 1, k]).all()
