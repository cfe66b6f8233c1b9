"""TEST-ONLY: the cases of tests/test_robust_hostsim.py and tests/test_gpu_robust.py, stated once over a backend K that takes and returns
numpy arrays (the host simulator through ctypes, or the device through fermiflow_amd.native), so that the references and expectations a
GPU run is judged by have been run on a CPU first.  Every check prints its largest error as a fraction of its derived bound
(tests/robust_ref.py) before it asserts.

Backend:  robust(e, logp | None, k, shift) -> stat (10 doubles; [9] not yet written);
apply(e, logp, stat, n_global, finish, z=None, g=None) -> (u, sum_out (1,), stat, z, g)   (z, g: (B, n, d) copies, rows overwritten)."""
import math

import numpy as np

from tests import robust_ref as R
from tests.common import bits_equal


def _report(what, **fracs):
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()) + "  (fraction of the derived bound)")
    for k, v in fracs.items():
        assert v <= 1.0, (what, k, v)


def _frac(got, want, scale, tol):
    """R.frac, with an infinite reference value (a sum of squares beyond the double range) asked for exactly"""
    if math.isinf(want):
        return 0.0 if got == want else math.inf
    return R.frac(got, want, tol * scale + R.UNDERFLOW)


def check(K, e, logp, k, shift, what, n_global=None):
    """robust + apply on one batch against the definitions; returns (stat after the apply, u)"""
    e, logp = np.asarray(e, dtype=np.float64), np.asarray(logp, dtype=np.float64)
    N = len(e) if n_global is None else n_global
    stat = K.robust(e, logp, k, shift)
    want, scale = R.statistics(e, logp, k, shift)
    nv = int(want[R.NV])
    assert stat[R.NV] == nv, (what, stat[R.NV], nv)
    if nv == 0:
        assert np.isnan(stat[[R.MED, R.WIDTH, R.LO, R.HI, R.E, R.ESS, R.EC]]).all() and stat[R.NC] == 0, (what, stat)
        u, s, stat2, _, _ = K.apply(e, logp, stat, N, 1)
        assert bits_equal(u, np.zeros(len(e))) and s[0] == 0.0 and np.isnan(stat2[R.VALUE]), (what, u, s, stat2)
        print(f"{what}: no valid walker, every weight is +0.0")
        return stat2, u
    assert bits_equal(stat[R.MED], want[R.MED]), (what, stat[R.MED], want[R.MED])
    fr = {name: _frac(stat[i], want[i], scale[i], R.FIN_TOL) for name, i in (("a", R.WIDTH), ("lo", R.LO), ("hi", R.HI), ("E", R.E), ("E_ss", R.ESS))}
    assert stat[R.ESS] >= 0.0
    # downstream of the window: from the RETURNED lo, hi (and, for u and the value, the returned Ec)
    c, nc, ec, ec_scale = R.clipped(e, logp, stat[R.LO], stat[R.HI], stat[R.MED])
    assert stat[R.NC] == nc, (what, stat[R.NC], nc)
    fr["Ec"] = _frac(stat[R.EC], ec, ec_scale, R.FIN_TOL)
    u, s, stat2, _, _ = K.apply(e, logp, stat, N, 1)
    assert bits_equal(stat2[:R.VALUE], stat[:R.VALUE])
    uw, ub, sw, smag = R.weights(e, logp, c, stat[R.EC], N)
    ok = R.valid(e, logp)
    assert bits_equal(u[~ok], np.zeros(int((~ok).sum()))), what          # exactly +0.0 for an invalid walker
    fr["u"] = R.frac(u, uw, ub)
    fr["sum"] = R.frac(s[0], sw, R.SUM_TOL * smag)
    fr["value"] = R.frac(stat2[R.VALUE], sw / nv, R.FIN_TOL * smag / nv)
    u0, s0, stat0, _, _ = K.apply(e, logp, stat, N, 0)                   # finish = 0: the same sum, stat[9] left alone
    assert bits_equal(u0, u) and bits_equal(s0, s) and bits_equal(stat0, stat), what
    _report(f"{what} (n_v {nv}, n_c {nc})", **fr)
    return stat2, u


SHIFTS = (0.0, 29.5, float("nan"))


def sizes(K, B):
    """a heavy-tailed batch, clean and with invalid walkers of every kind, at three shifts"""
    e, lp = R.energies(B)
    for shift in SHIFTS:
        check(K, e, lp, 5.0, shift, f"clean B={B} shift={shift}")
    es, ls = R.spoil(e, lp, every=3 if B <= 3 else 7)
    for shift in SHIFTS[:2]:
        check(K, es, ls, 5.0, shift, f"spoiled B={B} shift={shift}")


def all_equal(K, B, value=20.1):
    e, lp = np.full(B, value), R.energies(B)[1]
    for shift in (0.0, value):
        stat, u = check(K, e, lp, 5.0, shift, f"all equal B={B} shift={shift}")
        assert stat[R.WIDTH] == 0.0 and stat[R.ESS] == 0.0 and stat[R.NC] == 0 and stat[R.LO] == stat[R.HI] == value
        assert bits_equal(u, np.zeros(B)) and stat[R.VALUE] == 0.0


def heavy_ties(K, B):
    e, lp = R.ties(B)
    stat, _ = check(K, e, lp, 2.0, 29.5, f"ties B={B}")
    assert stat[R.MED] == 29.75


def last_digit(K, B):
    e, lp = R.last_bit(B)
    check(K, e, lp, 3.0, 0.0, f"last bit B={B}")
    for sub in (np.array([0.0, -0.0]), np.array([-0.0, 0.0, -0.0]), np.array([5e-324, -5e-324, 0.0, -0.0])):
        stat, _ = check(K, sub, np.ones(len(sub)), 3.0, 0.0, f"zeros and subnormals {sub.tolist()}")
        assert bits_equal(stat[R.MED], R.lower_median(sub))


def finite_outliers(K, B):
    e, lp = R.outliers(B)
    stat, u = check(K, e, lp, 5.0, 29.5, f"outliers B={B}")
    assert np.isfinite(stat[[R.WIDTH, R.LO, R.HI, R.E, R.EC]]).all() and np.isfinite(u).all() and stat[R.NV] == B
    assert stat[R.WIDTH] > 1e295      # they are valid: they widen the window


def every_walker_invalid(K, B):
    e, lp = R.energies(B)
    e[::2] = np.nan
    lp[1::2] = -np.inf
    check(K, e, lp, 5.0, 29.5, f"all invalid B={B}")
    check(K, np.full(B, np.inf), lp, 5.0, 29.5, f"all infinite B={B}")


def clip_widths(K, B):
    """k small enough to clip about a third of the batch; k = 1e6 clips nobody"""
    e, lp = R.energies(B)
    ok = R.valid(e, lp)
    m = R.lower_median(e[ok])
    dev = np.abs(e[ok] - m)
    k = float(np.quantile(dev, 2.0 / 3.0) / dev.mean())
    stat, _ = check(K, e, lp, k, 29.5, f"a third clipped B={B} k={k:.4f}")
    assert abs(stat[R.NC] - B / 3) <= max(2, 0.02 * B), stat[R.NC]
    stat, _ = check(K, e, lp, 1e6, 29.5, f"nobody clipped B={B}")
    assert stat[R.NC] == 0


def padding(K, B):
    """NaN padding behind the batch (what a padded all-gather appends) changes nothing, bit for bit -- also where it opens another
    segment; padding in the middle moves walkers to other places in the summation trees: the integers and the median are the same, the
    sums stay inside their bounds (check)."""
    e, lp = R.spoil(*R.energies(B))
    em = np.where(np.isfinite(lp), e, np.nan)             # as a rank marks its invalid walkers before the gather
    plain = K.robust(em, None, 5.0, 29.5)
    assert bits_equal(plain[:R.VALUE], K.robust(e, lp, 5.0, 29.5)[:R.VALUE])
    for pad in (1, 7, 1100):
        padded = K.robust(np.concatenate([em, np.full(pad, np.nan)]), None, 5.0, 29.5)
        assert bits_equal(padded[:R.VALUE], plain[:R.VALUE]), (B, pad, padded, plain)
    cut = B // 3
    mid = np.concatenate([em[:cut], np.full(5, np.nan), em[cut:]])
    stat, _ = check(K, mid, np.zeros(len(mid)), 5.0, 29.5, f"padding in the middle B={B}")
    assert stat[R.NV] == plain[R.NV] and stat[R.NC] == plain[R.NC] and bits_equal(stat[R.MED], plain[R.MED])


def rows(K, B, n, d):
    """apply on walkers with rows: invalid rows hold the documented configuration and zeros, valid rows are untouched bit for bit"""
    e, lp = R.spoil(*R.energies(B), every=5)
    rng = np.random.default_rng([17, B, n, d])
    z, g = rng.normal(size=(B, n, d)), rng.normal(size=(B, n, d))
    ok = R.valid(e, lp)
    assert (~ok).any() and ok.any()
    z[~ok] = np.nan
    g[~ok] = np.inf
    stat = K.robust(e, lp, 5.0, 29.5)
    u, s, stat2, z2, g2 = K.apply(e, lp, stat, B, 1, z=z, g=g)
    u1, s1, stat1, _, _ = K.apply(e, lp, stat, B, 1)
    assert bits_equal(u, u1) and bits_equal(s, s1) and bits_equal(stat2, stat1)
    assert bits_equal(z2[ok], z[ok]) and bits_equal(g2[ok], g[ok])
    safe = R.safe_rows(n, d)
    assert bits_equal(z2[~ok], np.broadcast_to(safe, (int((~ok).sum()), n, d))) and bits_equal(g2[~ok], np.zeros((int((~ok).sum()), n, d)))
    # pairwise distinct particles, none at the origin
    dist = np.linalg.norm(safe[:, None] - safe[None], axis=-1) + np.eye(n)
    assert dist.min() > 0 and np.linalg.norm(safe, axis=-1).min() > 0
