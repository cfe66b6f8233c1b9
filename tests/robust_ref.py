"""TEST-ONLY: a plain restatement of the robust estimator's definitions (include/fermiflow_robust.h; kernels: csrc/ff_robust.h) in numpy,
math.fsum and long double -- from the definitions, never from the kernels' identities (no radix passes, no moments about a shift) --,
the inputs of its tests and the bounds they use.  The product package never imports this.

Bounds (those of tests/estimator_ref.py): integers and the median are exact (the median by bit pattern); a SUM within SUM_TOL x the sum
of |terms|; a FINISH value within FIN_TOL x the sum of the |terms| of its formula:
    a = sum |e - m| / n_v                 scale a
    lo, hi = m -+ k a                     scale |m| + k a
    E = c0 + sum (e - c0) / n_v           scale |c0| + sum |e - c0| / n_v            (c0: the finite shift)
    E_ss = sum (e - c0)^2 - n_v (E - c0)^2    scale the sum of the two terms
    Ec = m + sum (c - m) / n_v            scale |m| + sum |c - m| / n_v
    value = sum l (c - Ec) / n_v          scale sum |l (c - Ec)| / n_v
lo and hi are checked against their definitions; what follows from them (c, n_c, Ec) is checked against a reference that takes the
RETURNED lo and hi, so that a walker within an ulp of the window cannot flip a count; u and the value likewise take the returned Ec
(whose own error its own check bounds): u_b = (c_b - Ec) (N / n_v) is then one subtraction, one division and one multiplication,
1.5 eps of |c_b - Ec| N / n_v, accepted within 4 eps (|c_b| + |Ec|) N / n_v."""
import math

import numpy as np

from tests.estimator_ref import EPS, FIN_TOL, LD, SUM_TOL, finite_shift, frac  # noqa: F401 (re-exported for the cases)

NSTAT = 10
NV, MED, WIDTH, LO, HI, E, ESS, EC, NC, VALUE = range(NSTAT)
SAFE_STEP = 0.25      # FF_ROBUST_SAFE_STEP
# Relative bounds say nothing where a result is subnormal: a rounding there loses up to half the smallest subnormal whatever the value.
# The finish formulas above put at most four roundings on a value, the reference's own conversion to double one more: 8 x 2^-1074
# is added to their bounds (it decides only for batches made of subnormals and zeros).
UNDERFLOW = 8 * 5e-324


def valid(e, logp=None):
    e = np.asarray(e, dtype=np.float64)
    ok = np.isfinite(e)
    return ok if logp is None else ok & np.isfinite(np.asarray(logp, dtype=np.float64))


def keys(e):
    """the order-preserving map of the fp64 bit pattern to uint64: all bits of a negative number flipped, the sign bit of the others set"""
    u = np.ascontiguousarray(e, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def lower_median(ev):
    """the element of 0-based rank (n - 1) // 2 in the order of keys(); NaN for an empty array"""
    if len(ev) == 0:
        return float("nan")
    return float(ev[np.argsort(keys(ev), kind="stable")[(len(ev) - 1) // 2]])


def _f64(x):
    with np.errstate(over="ignore"):
        return float(np.float64(x))


def statistics(e, logp, k, shift):
    """(want, scale): entries NV .. ESS of stat from the definitions in long double, and the scale of each (None: exact)"""
    e = np.asarray(e, dtype=np.float64)
    ok = valid(e, logp)
    ev = e[ok].astype(LD)
    nv = int(ok.sum())
    want, scale = [float("nan")] * NSTAT, [None] * NSTAT
    want[NV] = float(nv)
    if nv == 0:
        return want, scale
    m = lower_median(e[ok])
    c0 = LD(finite_shift(shift))
    a = np.abs(ev - LD(m)).sum() / nv
    mean = ev.sum() / nv
    want[MED], want[WIDTH], want[LO], want[HI] = m, _f64(a), _f64(LD(m) - LD(k) * a), _f64(LD(m) + LD(k) * a)
    want[E], want[ESS] = _f64(mean), _f64(((ev - mean) ** 2).sum())
    scale[WIDTH] = _f64(a)
    scale[LO] = scale[HI] = _f64(abs(LD(m)) + LD(k) * a)
    scale[E] = _f64(abs(c0) + np.abs(ev - c0).sum() / nv)
    scale[ESS] = _f64(((ev - c0) ** 2).sum() + nv * (mean - c0) ** 2)
    return want, scale


def clipped(e, logp, lo, hi, m):
    """(c (float64; NaN where invalid), n_c, Ec, scale of Ec) for the given window"""
    e = np.asarray(e, dtype=np.float64)
    ok = valid(e, logp)
    c = np.full(e.shape, np.nan)
    c[ok] = np.minimum(np.maximum(e[ok], lo), hi)
    nv = int(ok.sum())
    if nv == 0:
        return c, 0, float("nan"), None
    cl = c[ok].astype(LD)
    return c, int((c[ok] != e[ok]).sum()), _f64(cl.sum() / nv), _f64(abs(LD(m)) + np.abs(cl - LD(m)).sum() / nv)


def weights(e, logp, c, ec, n_global):
    """(u, bound of u, sum l (c - Ec), sum of |terms|) for the given clipped energies and clipped mean"""
    ok = valid(e, logp)
    nv = int(ok.sum())
    u, bound = np.zeros(len(c)), np.zeros(len(c))
    if nv == 0:
        return u, bound, 0.0, 0.0
    ratio = LD(n_global) / nv
    u[ok] = ((c[ok].astype(LD) - LD(ec)) * ratio).astype(np.float64)
    bound[ok] = (4 * EPS * (np.abs(c[ok]).astype(LD) + abs(LD(ec))) * ratio).astype(np.float64)
    terms = (np.asarray(logp, dtype=np.float64)[ok].astype(LD) * (c[ok].astype(LD) - LD(ec))).astype(np.float64)
    return u, bound, math.fsum(terms), math.fsum(np.abs(terms))


def safe_rows(n, d):
    """the configuration ff_energy_robust_apply writes over the z row of an invalid walker: particle i at (0.25 (i + 1), 0 [, 0])"""
    z = np.zeros((n, d))
    z[:, 0] = SAFE_STEP * (np.arange(n) + 1)
    return z


# ----------------------------------------------------------------------------------------------------------------- inputs
def energies(B, seed=0):
    """e = 30 + 7 N(0, 1) with a heavy tail (one walker in 16 times 1 + 9 U^4), logp = -20 + 3 N(0, 1)"""
    rng = np.random.default_rng([11, seed, B])
    e = 30.0 + 7.0 * rng.normal(size=B)
    tail = rng.random(B) < 1.0 / 16.0
    e[tail] *= 1.0 + 9.0 * rng.random(int(tail.sum())) ** 4
    return e, -20.0 + 3.0 * rng.normal(size=B)


def spoil(e, logp, seed=0, every=7):
    """copies with NaN of both signs and +-inf in e, and non-finite l beside a finite e, at about one walker in `every`"""
    e, logp = np.array(e, dtype=np.float64), np.array(logp, dtype=np.float64)
    rng = np.random.default_rng([12, seed, len(e)])
    bad = np.flatnonzero(rng.random(len(e)) < 1.0 / every)
    neg_nan = np.array([0xfff8000000000001], dtype=np.uint64).view(np.float64)[0]
    for i, b in enumerate(bad):
        kind = i % 6
        if kind < 4:
            e[b] = (np.nan, neg_nan, np.inf, -np.inf)[kind]
        else:
            logp[b] = (np.nan, -np.inf)[kind - 4]
    return e, logp


def ties(B, seed=0):
    """most of the batch ON the median value, the rest spread about it"""
    rng = np.random.default_rng([13, seed, B])
    e = np.full(B, 29.75)
    far = rng.random(B) < 0.3
    e[far] += rng.normal(size=int(far.sum()))
    return e, -20.0 + 3.0 * rng.normal(size=B)


def last_bit(B, seed=0):
    """mixed signs, -0.0 and +0.0, subnormals, and neighbours in the last mantissa bit of one value: the last radix digit decides"""
    rng = np.random.default_rng([14, seed, B])
    base = np.array([1.5], dtype=np.float64).view(np.uint64)[0]
    near = (base + rng.integers(0, 8, size=B).astype(np.uint64)).view(np.float64)
    e = np.where(rng.random(B) < 0.5, near, rng.normal(size=B))
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1.5, 1.5])
    idx = rng.permutation(B)[:min(B, 3 * len(special))]
    e[idx] = np.resize(special, len(idx))
    return e, rng.normal(size=B)


def outliers(B, seed=0):
    """three finite outliers of +-1e300 in an ordinary batch"""
    e, logp = energies(B, seed)
    idx = np.random.default_rng([15, seed, B]).permutation(B)[:3]
    e[idx] = np.resize([1e300, -1e300, 1e300], len(idx))
    return e, logp


def dyadic(B, seed=0):
    """e_b = 2.5 + k_b / 64 with integer k_b that add up to 0 (B even): every sum, mean and difference is exact"""
    k = np.random.default_rng([16, seed, B]).integers(-40, 41, size=B // 2)
    k = np.concatenate([k, -k])
    return 2.5 + k / 64.0
