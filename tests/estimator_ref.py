"""TEST-ONLY: plain references for the estimator and schedule kernels of csrc/ff_walkers.hip (ff_energy_estimate, ff_reduce_energy,
ff_energy_finish, ff_reduce_moments, ff_beta_state_partials, ff_beta_finish, ff_walker_order / _schedule, ff_scale_counts), the
inputs of their tests and the tolerances those tests use.  numpy and math.fsum only; the product package never imports this.

Tolerances (derived, not tuned):
  * a SUM of terms t_i is accepted within SUM_TOL * fsum(|t_i|), SUM_TOL = 128 eps.  The longest chain of roundings any of the kernels
    puts on one term is under 64 (per-thread serial part + tree + cross-workgroup join; the one-workgroup kernels reach 32 + 1 + 10 at
    65 536 walkers, which is why they are tested up to that size only), each of at most eps/2 of a partial sum that |t| bounds.
  * a FINISH value is accepted within FIN_TOL = 256 eps times the sum of the absolute values of the terms its formula adds and subtracts
    (the `scale` every finish reference returns beside its value): its inputs are sums that carry up to 64 roundings each, and the
    formula puts a handful on top.
  * integers, the order and the scale table's decisions are exact; hs and the table go by rtol 1e-15.
Sums are exact (math.fsum over terms formed in long double and rounded once); finish values are computed walker by walker in long double
from their definitions, never from the moment identities the kernels use."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
SUM_TOL = 128 * EPS
FIN_TOL = 256 * EPS
LD = np.longdouble
SS_K = 16              # FF_SS_K: slices per state of ff_beta_state_partials
BINS = 32              # FF_ORD_BINS
SEG, THREADS = 512, 256      # FF_ORD_SEG, FF_ORD_THREADS
RTOL_TABLE = 1e-15


def finite_shift(c):
    """ff_finite_shift: a non-finite shift counts as 0"""
    c = float(c)
    return c if math.isfinite(c) else 0.0


def frac(got, want, bound):
    """largest |got - want| / bound over the entries (0 / 0 = 0: where the bound is zero the value must be exact)"""
    got, want, bound = (np.atleast_1d(np.asarray(a, dtype=LD)) for a in (got, want, bound))
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(diff == 0, 0.0, diff / bound)
    f = np.where(np.isnan(f), np.inf, f)
    return float(f.max()) if f.size else 0.0


def _fsum(terms):
    """(exact sum, exact sum of absolute values) of long-double terms rounded once to double"""
    t = np.asarray(terms, dtype=LD).astype(np.float64).reshape(-1)
    return math.fsum(t), math.fsum(np.abs(t))


# ---------------------------------------------------------------------------------------------------------------- sums
def energy_sums(e, logp, shift):
    """ff_reduce_energy / ff_energy_estimate: [sum (e - c), sum (e - c)^2, sum logp, sum logp (e - c)] and the sums of |terms|"""
    c = LD(finite_shift(shift))
    v, lp = np.asarray(e, dtype=LD) - c, np.asarray(logp, dtype=LD)
    pairs = [_fsum(v), _fsum(v * v), _fsum(lp), _fsum(lp * v)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def moments(e, shift):
    """ff_reduce_moments: [sum (e - c), sum (e - c)^2] and the sums of |terms|"""
    v = np.asarray(e, dtype=LD) - LD(finite_shift(shift))
    pairs = [_fsum(v), _fsum(v * v)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def state_bounds(ws, ns):
    """[b0, b1) of every state in the sorted list"""
    ws = np.asarray(ws)
    return np.searchsorted(ws, np.arange(ns), "left"), np.searchsorted(ws, np.arange(1, ns + 1), "left")


def state_partials(e, logp, ws, ns):
    """ff_beta_state_partials: part[s][k] = (sum e, count, sum logp, sum logp e) over slice k of state s -- the kernel's slice bounds
    c0 = b0 + len k // 16, c1 = b0 + len (k + 1) // 16 -- and the sums of |terms|: two (ns, 16, 4) arrays"""
    e, logp = np.asarray(e, dtype=LD), np.asarray(logp, dtype=LD)
    b0, b1 = state_bounds(ws, ns)
    part, mag = np.zeros((ns, SS_K, 4)), np.zeros((ns, SS_K, 4))
    for s in range(ns):
        n = int(b1[s] - b0[s])
        for k in range(SS_K):
            c0, c1 = int(b0[s]) + n * k // SS_K, int(b0[s]) + n * (k + 1) // SS_K
            part[s, k, 1] = mag[s, k, 1] = c1 - c0
            if c1 > c0:
                ee, ll = e[c0:c1], logp[c0:c1]
                for col, t in ((0, ee), (2, ll), (3, ll * ee)):
                    part[s, k, col], mag[s, k, col] = _fsum(t)
    return part, mag


# ------------------------------------------------------------------------------------------------------- finish values
def energy_finish(e, logp, shift):
    """est3 = [E, sum (e - E)^2, mean(logp (e - E))] of ff_energy_finish walker by walker, and the scale of each entry for a kernel
    that works about the shift c: |c| + sum |e - c| / n;  sum (e - c)^2 + n (E - c)^2;  (sum |logp (e - c)| + |E - c| sum |logp|) / n"""
    e, lp, c = np.asarray(e, dtype=LD), np.asarray(logp, dtype=LD), LD(finite_shift(shift))
    n = LD(len(e))
    E = e.sum() / n
    est = [E, ((e - E) ** 2).sum(), (lp * (e - E)).sum() / n]
    scale = [abs(c) + np.abs(e - c).sum() / n, ((e - c) ** 2).sum() + n * (E - c) ** 2,
             (np.abs(lp * (e - c)).sum() + abs(E - c) * np.abs(lp).sum()) / n]
    return np.array(est, dtype=np.float64), np.array(scale, dtype=np.float64)


def log_softmax(logits):
    """(log_softmax(logits) in long double, the absolute-error scale of each entry: |logit| + |log Z| + 1 -- the subtraction's two
    operands, and 1 for the relative error of Z = sum exp inside the logarithm)"""
    lg = np.asarray(logits, dtype=LD)
    m = lg.max()
    lz = m + np.log(np.exp(lg - m).sum())
    return lg - lz, np.abs(lg) + abs(lz) + 1


def beta_finish(e, logp, ws, logits, beta, shift):
    """Everything ff_beta_finish returns, from the definitions (BetaVMC.forward; the formulas of
    tests/test_hostsim.py::test_finite_temperature_estimator_kernels) walker by walker in long double:
      est8 = [E, sum (e - E)^2, F, sum (f - F)^2, S, S_analytical, mean(log p(s_b) (f_b - F)), mean(logp_b (e_b - mean_e[s_b]))],
      f_b = e_b + log p(s_b) / beta;  gphi[s] = cF_s - p(s) sum cF, cF_s = sum_{b in s} (f_b - F) / n;  mean_e;  logp_all.
    Every value comes with its scale: the sum of |terms| of the kernel's formula, with a_s = the error scale of log p(s) (log_softmax)
    standing in for |log p(s)| so that the error of the logarithm itself is covered.  sum (f - F)^2 is formed about the shift c0 like
    sum (e - E)^2: scale sum (f - c0)^2 + n (F - c0)^2."""
    e, lp = np.asarray(e, dtype=LD), np.asarray(logp, dtype=LD)
    ws = np.asarray(ws, dtype=np.int64)
    ns, n, beta, c0 = len(logits), LD(len(e)), LD(beta), LD(finite_shift(shift))
    lsm, a = log_softmax(logits)
    f = e + lsm[ws] / beta
    E, F = e.sum() / n, f.sum() / n
    cnt = np.bincount(ws, minlength=ns).astype(LD)
    b0, b1 = state_bounds(ws, ns)
    se = np.array([e[i:j].sum() for i, j in zip(b0, b1)], dtype=LD)
    sae = np.array([np.abs(e[i:j]).sum() for i, j in zip(b0, b1)], dtype=LD)
    me = se / np.maximum(cnt, 1)
    cF = np.array([(f[i:j] - F).sum() for i, j in zip(b0, b1)], dtype=LD) / n
    p = np.exp(lsm)
    est = [E, ((e - E) ** 2).sum(), F, ((f - F) ** 2).sum(), -lsm[ws].sum() / n, -(lsm * p).sum(),
           (lsm[ws] * (f - F)).sum() / n, (lp * (e - me[ws])).sum() / n]
    g = (sae + cnt * (a / beta + abs(F))) / n
    scale = [abs(c0) + np.abs(e - c0).sum() / n, ((e - c0) ** 2).sum() + n * (E - c0) ** 2,
             (np.abs(e) + a[ws] / beta).sum() / n, ((f - c0) ** 2).sum() + n * (F - c0) ** 2,
             a[ws].sum() / n, (p * (1 + np.abs(lsm)) * a).sum(),
             (a[ws] * (np.abs(e) + a[ws] / beta + abs(F))).sum() / n, (np.abs(lp) * (np.abs(e) + np.abs(me[ws]))).sum() / n]
    d = lambda x: np.asarray(x, dtype=np.float64)
    return dict(est8=d(est), est8_scale=d(scale), gphi=d(cF - p * cF.sum()), gphi_scale=d(g + p * g.sum()),
                mean_e=d(me), mean_e_scale=d(sae / np.maximum(cnt, 1)), logp_all=d(lsm), logp_all_scale=d(a))


# -------------------------------------------------------------------------------------------------------- the schedule
def classes(cost):
    """the cost class: cost clamped to [0, 32) (both clamps of ff_ord_row)"""
    return np.clip(np.asarray(cost, dtype=np.int64), 0, BINS - 1)


def sched_key(cost, hval=None, tab=None, interval=0.0):
    """ff_sched_key: the class, raised by four for every planned equal step beyond two (plain double operations: exact)"""
    cc = classes(cost)
    if tab is None or hval is None or not interval > 0.0:
        return cc
    hval, f = np.asarray(hval, dtype=np.float64), np.asarray(tab, dtype=np.float64)[cc]
    f = np.where(f > 0.0, f, 0.6)
    hq = hval * f
    pos = hval > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(hq >= interval, 1.0, np.ceil(interval / np.where(pos, hq, 1.0) - 1e-9))
    k = np.minimum(k, 8).astype(np.int64)
    return np.where(pos, np.minimum(BINS - 1, cc + 4 * np.maximum(k - 2, 0)), cc)


def order(cost, hval=None, tab=None, interval=0.0):
    """The exact permutation of ff_order_place_kernel: by row (most expensive key first), then segment of 512, then thread k % 256,
    then k // 256 (k = the walker's index in its segment)."""
    row = BINS - 1 - sched_key(cost, hval, tab, interval)
    j = np.arange(len(row))
    k = j % SEG
    return np.lexsort((k // THREADS, k % THREADS, j // SEG, row)).astype(np.int32)


def opening_steps(cost, hval, tab, interval=0.0):
    """hs of ff_walker_schedule: hval x the (updated) factor of the class, rounded down to interval / k"""
    hq = np.asarray(hval, dtype=np.float64) * np.asarray(tab, dtype=np.float64)[classes(cost)]
    if interval > 0.0:
        m = (hq > 0.0) & (hq < interval)
        hq[m] = interval / np.ceil(interval / hq[m] - 1e-9)
    return hq


def shrink_at_used(shrink_at):
    """what ff_walker_schedule makes of the caller's threshold: 0 = 0.10, else within [0.02, 0.5]"""
    return min(0.5, max(0.02, shrink_at)) if shrink_at > 0.0 else 0.10


def rule(tab, cls, hs, he, interval, shrink_at=0.10):
    """The table update of ff_walker_schedule (ff_scale_update over the counts of the previous pass): classes of which more than
    shrink_at rejected their first step (he < hs) shrink by 0.93; classes with less than half of that grow by 1.02 if 70 % of their
    voters (without an interval: every walker; with one: those planned for k >= 3 equal steps) accepted a step of the plan one shorter
    (without an interval: 1.25 x the opening step); within [0.25, 1]; classes with fewer than 64 walkers, and walkers without a step,
    keep theirs."""
    want = tab.copy()
    ok = (he > 0) & (hs > 0)
    if interval > 0:
        k = np.rint(interval / np.where(hs > 0, hs, 1.0))
        vote = ok & (k >= 3)
        yes = vote & (he >= 0.999 * interval / np.maximum(k - 1, 1))
    else:
        vote, yes = ok, ok & (he >= 1.25 * hs)
    for c in range(32):
        m = cls == c
        n_c, r_c, v_c, y_c = int((m & ok).sum()), int((m & ok & (he < 0.999 * hs)).sum()), int((m & vote).sum()), int((m & yes).sum())
        if n_c >= 64:
            f = 0.93 if r_c / n_c > shrink_at else (1.02 if (r_c / n_c < 0.5 * shrink_at and v_c >= 16 and y_c >= 0.7 * v_c) else 1.0)
            want[c] = min(1.0, max(0.25, tab[c] * f))
    return want


def scale_counts(cost, hs, he, interval=0.0):
    """The 128 integers of ff_scale_counts: [walkers with a step, by class | of them, first step rejected | voters | yes-votes]"""
    cls, hs, he = classes(cost), np.asarray(hs, dtype=np.float64), np.asarray(he, dtype=np.float64)
    ok = (he > 0) & (hs > 0)
    if interval > 0:
        k = np.rint(interval / np.where(hs > 0, hs, 1.0))
        vote = ok & (k >= 3)
        yes = vote & (he >= 0.999 * interval / np.maximum(k - 1, 1))
    else:
        vote, yes = ok, ok & (he >= 1.25 * hs)
    return np.concatenate([np.bincount(cls[m], minlength=BINS) for m in (ok, ok & (he < 0.999 * hs), vote, yes)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- inputs
def energies(B, seed=0):
    """e = 30 + 7 N(0, 1), logp = -20 + 3 N(0, 1)"""
    rng = np.random.default_rng([1, seed, B])
    return 30.0 + 7.0 * rng.normal(size=B), -20.0 + 3.0 * rng.normal(size=B)


def mean_shift(e):
    return math.fsum(e) / len(e)


def costs(B, seed=0):
    """step counts in [-3, 40): both clamps of ff_ord_row are hit"""
    return np.random.default_rng([2, seed, B]).integers(-3, 40, size=B).astype(np.int32)


def hvals(B, seed=0):
    """accepted steps in (0, 1.5) with a few exact zeros (a failed or cold-started walker)"""
    rng = np.random.default_rng([3, seed, B])
    h = 1.5 * (1.0 - rng.random(B))
    h[rng.choice(B, size=min(5, B // 8), replace=False)] = 0.0
    return h


START_TABLE = np.where(np.arange(BINS) <= 6, 0.9, 0.6)


def rejecting_pass(cost, hs, seed=0):
    """he of a pass without an interval (the patterns of tests/test_hostsim.py): classes 3 and 31 reject, class 5 sits between the two
    thresholds, 0, 1 and 6 show room to grow, half of 9 does, class 7 reports no accepted step"""
    rng = np.random.default_rng([4, seed, len(hs)])
    cls, he, B = classes(cost), np.array(hs, dtype=np.float64), len(hs)
    he[(cls == 3) | ((cls == 5) & (rng.random(B) < 0.075)) | (cls == 31)] *= 0.5
    he[(cls <= 1) | (cls == 6)] *= 1.3
    he[(cls == 9) & (rng.random(B) < 0.5)] *= 1.3
    he[cls == 7] = 0.0
    return he


def interval_pass(cost, hs3, interval=1.0):
    """he of a pass planned in equal steps of `interval`: classes 12 and 20 accept the step of the plan one shorter, class 15 larger
    steps short of it"""
    cls, hs3 = classes(cost), np.asarray(hs3, dtype=np.float64)
    k3 = np.rint(interval / np.where(hs3 > 0, hs3, 1.0))
    he3 = hs3.copy()
    m = ((cls == 12) | (cls == 20)) & (hs3 > 0)
    he3[m] = (interval / np.maximum(k3 - 1, 1))[m]
    he3[cls == 15] *= 1.2
    he3[(cls == 15) & (k3 > 5)] = hs3[(cls == 15) & (k3 > 5)]
    return he3


def states(ns, B, seed=0):
    """Sorted state list; with ns >= 4 and B >= 64 it holds an empty state (0), a state of one walker (1) and one of five (ns // 2:
    fewer than 16, so that most of its 16 slices are empty), the rest drawn with uneven weights"""
    rng = np.random.default_rng([5, seed, ns, B])
    if ns < 4 or B < 64:
        return np.sort(rng.integers(0, ns, size=B)).astype(np.int32)
    special = {0, 1, ns // 2}
    rest = np.array([s for s in range(ns) if s not in special])
    w = rng.random(len(rest)) ** 3 + 1e-3
    ws = np.concatenate([rng.choice(rest, size=B - 6, p=w / w.sum()), [1], [ns // 2] * 5])
    return np.sort(ws).astype(np.int32)


def state_logits(ns, seed=0):
    """N(0, 1), one state at -40 (with ns >= 4 the five-walker state of states(): log p / beta reaches -90 there)"""
    lg = np.random.default_rng([6, seed, ns]).normal(size=ns)
    if ns > 1:
        lg[ns // 2] = -40.0
    return lg


# zero variance: (B, e, shift, logits) -- a constant local energy, walkers dealt evenly over three states, beta = 3.  With equal
# logits f is constant too and sum (f - F)^2 is exactly 0 (what a clamp alone also returns); with logits (0, -1, -2) and the shift at the
# mean it is 0.074 n while its bound is 256 eps 0.52 n = 1.9e-09 at 65 536 walkers -- three hundred times below the n E^2 eps that
# moments about zero lose, whichever sign that error takes
_EQUAL, _UNEQUAL = (0.0, 0.0, 0.0), (0.0, -1.0, -2.0)
ZERO_VARIANCE = [(1000, 20.1, 0.0, _EQUAL), (4097, 20.1, 0.0, _EQUAL), (65536, 20.1, 0.0, _EQUAL), (65536, 20.1, 20.1, _EQUAL),
                 (65536, 13.7, 0.0, _EQUAL), (65536, 1.0 / 3.0, 0.0, _EQUAL), (4097, 1.0 / 3.0, 1.0 / 3.0, _EQUAL),
                 (65536, 20.1, 20.1, _UNEQUAL), (65536, 13.7, 13.7, _UNEQUAL), (65536, 30.0, 30.0, _UNEQUAL)]
ZERO_VARIANCE_BETA = 3.0


def zero_variance(B, e, logits=_EQUAL):
    """(e, logp, sorted states, logits) of one zero-variance row"""
    _, logp = energies(B, seed=7)
    return np.full(B, e), logp, np.sort(np.arange(B) % 3).astype(np.int32), np.array(logits)
