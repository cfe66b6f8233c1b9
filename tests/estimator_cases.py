"""TEST-ONLY: the cases of tests/test_gpu_estimators.py and tests/test_estimators_hostsim.py, stated once over a backend K that takes
and returns numpy arrays (the device through fermiflow_amd.native, or the host simulator through ctypes) -- so that the references and
expectations a GPU run is judged by have been run on a CPU first.  Every check prints its largest error as a fraction of its derived
bound (tests/estimator_ref.py) before it asserts.

Backend:  energy_estimate(e, logp, shift, n_global) -> (sums4, est3 | None);  reduce_energy(e, logp, shift) -> sums4;
energy_finish(sums4, shift, n) -> est3;  reduce_moments(e, shift=0.0, shift_dev=None, scale=1.0) -> out2;
beta(e, logp, ws, logits, beta, shift) -> (part (ns, 16, 4), est8, gphi, mean_e, logp_all);
walker_order(cost, hval=None) -> order | (order, hmean);  walker_schedule(cost, hval, tab, prev=None, interval=0.0, counts=None,
shrink_at=0.0) -> (order, hmean, hs, tab_out);  scale_counts(cost, hs, he, interval=0.0, into=None) -> counts128."""
import math

import numpy as np

from tests import estimator_ref as R
from tests.common import bits_equal

SHIFTS = ("zero", "29.5", "mean", "nan", "inf")


def shift_value(name, e):
    return {"zero": 0.0, "29.5": 29.5, "mean": R.mean_shift(e), "nan": float("nan"), "inf": float("inf")}[name]


def _report(what, **fracs):
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()) + "  (fraction of the derived bound)")
    for k, v in fracs.items():
        assert v <= 1.0, (what, k, v)


def energy_estimate(K, B):
    """case 1: the four sums and est3 of ff_energy_estimate at five shifts, with and without est3"""
    e, lp = R.energies(B)
    fs = ff = 0.0
    for name in SHIFTS:
        shift = shift_value(name, e)
        want, mag = R.energy_sums(e, lp, shift)
        ewant, escale = R.energy_finish(e, lp, shift)
        sums, est = K.energy_estimate(e, lp, shift, B)
        sums0, est0 = K.energy_estimate(e, lp, shift, 0)
        assert est0 is None and bits_equal(sums0, sums), (B, name)
        assert est[1] >= 0.0
        fs, ff = max(fs, R.frac(sums, want, R.SUM_TOL * mag)), max(ff, R.frac(est, ewant, R.FIN_TOL * escale))
    _report(f"energy_estimate B={B}", sums4=fs, est3=ff)
    return e, lp


def reduce_energy(K, B):
    """case 2: the one-workgroup sums against the reference and the many-workgroup kernel; two ranks' sums added, then the finish"""
    e, lp = R.energies(B)
    shift = 29.5
    want, mag = R.energy_sums(e, lp, shift)
    ewant, escale = R.energy_finish(e, lp, shift)
    sums = K.reduce_energy(e, lp, shift)
    many, _ = K.energy_estimate(e, lp, shift, 0)
    cut = B // 3
    parts = [K.reduce_energy(e[a:b], lp[a:b], shift) for a, b in ((0, cut), (cut, B)) if b > a]
    both = np.sum(parts, axis=0)
    # (against_estimate: the two kernels are each within the bound of the exact sums, so of each other within twice that -- implied
    # by the two comparisons against the reference, printed for the record)
    _report(f"reduce_energy B={B}", sums4=R.frac(sums, want, R.SUM_TOL * mag), against_estimate=R.frac(sums, many, 2 * R.SUM_TOL * mag),
            two_ranks=R.frac(both, want, R.SUM_TOL * mag), finish=R.frac(K.energy_finish(sums, shift, B), ewant, R.FIN_TOL * escale),
            finish_two_ranks=R.frac(K.energy_finish(both, shift, B), ewant, R.FIN_TOL * escale))


def reduce_moments(K, B):
    """case 3: host shift, and shift_dev x shift_dev_scale (the sum of e and 1 / B: one product, the same in the reference)"""
    e, _ = R.energies(B)
    w1, m1 = R.moments(e, 29.5)
    total = math.fsum(e)
    w2, m2 = R.moments(e, total * (1.0 / B))
    w3, m3 = R.moments(e, float("nan"))
    _report(f"reduce_moments B={B}", host_shift=R.frac(K.reduce_moments(e, shift=29.5), w1, R.SUM_TOL * m1),
            device_shift=R.frac(K.reduce_moments(e, shift_dev=total, scale=1.0 / B), w2, R.SUM_TOL * m2),
            nan_shift=R.frac(K.reduce_moments(e, shift_dev=float("nan"), scale=1.0), w3, R.SUM_TOL * m3))


def beta_estimator(K, ns, B, beta, shift, one_state=False):
    """case 4: the per-state slices and every output of ff_beta_finish"""
    e, lp = R.energies(B, seed=ns)
    ws = np.zeros(B, dtype=np.int32) if one_state else R.states(ns, B)
    logits = R.state_logits(ns)
    pwant, pmag = R.state_partials(e, lp, ws, ns)
    want = R.beta_finish(e, lp, ws, logits, beta, shift)
    part, est, gphi, mean_e, lpa = K.beta(e, lp, ws, logits, beta, shift)
    np.testing.assert_array_equal(part[:, :, 1], pwant[:, :, 1])       # the slice lengths
    assert est[1] >= 0.0 and est[3] >= 0.0
    f8 = [R.frac(est[k], want["est8"][k], R.FIN_TOL * want["est8_scale"][k]) for k in range(8)]
    _report(f"beta ns={ns} B={B} beta={beta} shift={shift}" + (" one state" if one_state else ""),
            slices=R.frac(part, pwant, R.SUM_TOL * pmag), **dict(zip(("E", "E_ss", "F", "F_ss", "S", "S_an", "gphi_val", "gtheta_val"), f8)),
            gphi=R.frac(gphi, want["gphi"], R.FIN_TOL * want["gphi_scale"]), mean_e=R.frac(mean_e, want["mean_e"], R.FIN_TOL * want["mean_e_scale"]),
            logp_all=R.frac(lpa, want["logp_all"], R.FIN_TOL * want["logp_all_scale"]))


def schedule(K, B):
    """case 5: the exact order, mean(hval), hs, the table and the 128 counts"""
    cost, h, tab = R.costs(B), R.hvals(B), R.START_TABLE
    cls = R.classes(cost)
    want_order = R.order(cost)
    assert sorted(want_order.tolist()) == list(range(B))
    o0 = K.walker_order(cost)
    np.testing.assert_array_equal(o0, want_order)
    o1, hm = K.walker_order(cost, hval=h)
    np.testing.assert_array_equal(o1, want_order)
    hbound = R.SUM_TOL * math.fsum(np.abs(h)) / B
    fh = R.frac(hm, math.fsum(h) / B, hbound)
    # no previous pass: the table is copied, hs = hval x factor
    o2, hm2, hs, tab1 = K.walker_schedule(cost, h, tab)
    np.testing.assert_array_equal(o2, want_order)
    assert bits_equal(hm2, hm) and bits_equal(tab1, tab)
    hs_ref = R.opening_steps(cost, h, tab)
    np.testing.assert_allclose(hs, hs_ref, rtol=R.RTOL_TABLE)
    # a previous pass, by its arrays and by its counts; three thresholds
    he = R.rejecting_pass(cost, hs_ref)
    cref = R.scale_counts(cost, hs_ref, he)
    cnts = K.scale_counts(cost, hs_ref, he)
    np.testing.assert_array_equal(cnts, cref)
    np.testing.assert_array_equal(K.scale_counts(cost, hs_ref, he, into=cnts), 2 * cref)      # the kernel adds to what is there
    for shrink_at in (0.0, 0.25, 0.01):
        want_tab = R.rule(tab, cls, hs_ref, he, 0.0, R.shrink_at_used(shrink_at))
        o3, _, hs2, tab2 = K.walker_schedule(cost, h, tab, prev=(cost, hs_ref, he), shrink_at=shrink_at)
        np.testing.assert_array_equal(o3, want_order)
        np.testing.assert_allclose(tab2, want_tab, rtol=R.RTOL_TABLE)
        np.testing.assert_allclose(hs2, R.opening_steps(cost, h, want_tab), rtol=R.RTOL_TABLE)
        _, _, hs2c, tab2c = K.walker_schedule(cost, h, tab, counts=cref.astype(np.float64), shrink_at=shrink_at)
        assert bits_equal(tab2c, tab2) and bits_equal(hs2c, hs2)
        again = K.walker_schedule(cost, h, tab, prev=(cost, hs_ref, he), shrink_at=shrink_at)
        assert all(bits_equal(a, b) for a, b in zip(again[1:], (hm2, hs2, tab2))) and (again[0] == o3).all()
    # interval = 1: the order goes by class + 4 x (planned equal steps beyond two), hs is rounded down to 1 / k
    want_o4 = R.order(cost, h, tab, 1.0)
    o4, _, hs3, _ = K.walker_schedule(cost, h, tab, interval=1.0)
    np.testing.assert_array_equal(o4, want_o4)
    hs3_ref = R.opening_steps(cost, h, tab, 1.0)
    np.testing.assert_allclose(hs3, hs3_ref, rtol=R.RTOL_TABLE)
    he3 = R.interval_pass(cost, hs3_ref)
    want4 = R.rule(tab, cls, hs3_ref, he3, 1.0)
    o5, _, hs4, tab4 = K.walker_schedule(cost, h, tab, prev=(cost, hs3_ref, he3), interval=1.0)
    np.testing.assert_array_equal(o5, want_o4)              # the key goes by the table the call was given, hs by the updated one
    np.testing.assert_allclose(tab4, want4, rtol=R.RTOL_TABLE)
    np.testing.assert_allclose(hs4, R.opening_steps(cost, h, want4, 1.0), rtol=R.RTOL_TABLE)
    c3 = R.scale_counts(cost, hs3_ref, he3, 1.0)
    np.testing.assert_array_equal(K.scale_counts(cost, hs3_ref, he3, interval=1.0), c3)
    _, _, hs4c, tab4c = K.walker_schedule(cost, h, tab, counts=c3.astype(np.float64), interval=1.0)
    assert bits_equal(tab4c, tab4) and bits_equal(hs4c, hs4)
    if B >= 4100:      # (~100 walkers per class: the patterns decide)
        t2 = R.rule(tab, cls, hs_ref, he, 0.0)
        assert t2[3] == tab[3] * 0.93 and t2[0] == min(1.0, tab[0] * 1.02) and t2[7] == tab[7] and t2[9] == tab[9]
        assert want4[12] == tab[12] * 1.02 and want4[20] == tab[20] * 1.02 and want4[15] == tab[15]
    _report(f"schedule B={B}", hmean=fh)


def zero_variance(K, B, e0, shift, logits):
    """case 6: a constant local energy.  Both centred sums of squares are >= 0 and inside their bound around their exact value -- 0 for
    sum (e - E)^2, and for sum (f - F)^2 with equal logits; with unequal logits sum (f - F)^2 is positive, no clamp hides its error
    and the bound (shift at the mean) is far below n E^2 eps -- on the one-launch estimator, on sums + finish and on the
    finite-temperature estimator; the standard deviations VMC._std forms are finite."""
    e, lp, ws, logits = R.zero_variance(B, e0, logits)
    beta = R.ZERO_VARIANCE_BETA
    _, est = K.energy_estimate(e, lp, shift, B)
    est_f = K.energy_finish(K.reduce_energy(e, lp, shift), shift, B)
    _, est8, _, _, _ = K.beta(e, lp, ws, logits, beta, shift)
    want = R.beta_finish(e, lp, ws, logits, beta, shift)
    tag = f"zero variance B={B} e={e0!r} shift={shift!r} logits={tuple(float(v) for v in logits)}"
    print(f"{tag}: E_ss {est[1]!r} (sums + finish {est_f[1]!r}), beta E_ss {est8[1]!r} F_ss {est8[3]!r} "
          f"(exact {want['est8'][3]!r}, bound {R.FIN_TOL * want['est8_scale'][3]:.3e})")
    _, escale = R.energy_finish(e, lp, shift)
    for v in (est[1], est_f[1], est8[1], est8[3]):
        assert v >= 0.0, v
        assert math.isfinite(math.sqrt(v / (B - 1)))
    _report(tag, E_ss=R.frac(est[1], 0.0, R.FIN_TOL * escale[1]),
            E_ss_finish=R.frac(est_f[1], 0.0, R.FIN_TOL * escale[1]), beta_E_ss=R.frac(est8[1], 0.0, R.FIN_TOL * want["est8_scale"][1]),
            F_ss=R.frac(est8[3], want["est8"][3], R.FIN_TOL * want["est8_scale"][3]))
