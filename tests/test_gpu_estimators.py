"""The estimator and schedule kernels of csrc/ff_walkers.hip on the device, through fermiflow_amd.native, against the plain references
of tests/estimator_ref.py: ff_energy_estimate (many workgroups joined by the one that finishes last), ff_reduce_energy /
ff_energy_finish, ff_reduce_moments, ff_beta_state_partials / ff_beta_finish, ff_walker_order / ff_walker_schedule, ff_scale_counts.
No model is built and nothing is trained: every test is a handful of launches on seeded arrays.  Floating-point results are compared
within the derived bounds of the reference module (never bit for bit against host arithmetic: the device contracts to FMA); bit
equality is asserted between two device results and for integers.  The same cases run under the host simulator in
tests/test_estimators_hostsim.py."""
import numpy as np
import pytest
import torch

from tests import estimator_cases as cases
from tests import estimator_ref as R
from tests.common import N, T, bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


class _Dev:
    """the backend of tests/estimator_cases.py over fermiflow_amd.native"""

    def __init__(self, dev):
        self.dev = dev

    def _t(self, a, dtype=torch.float64):
        return None if a is None else T(np.atleast_1d(a), self.dev, dtype)

    def energy_estimate(self, e, logp, shift, n_global):
        from fermiflow_amd import native
        sums, est = native.energy_estimate(self._t(e), self._t(logp), self._t(shift), n_global)
        return N(sums), None if est is None else N(est)

    def reduce_energy(self, e, logp, shift):
        from fermiflow_amd import native
        return N(native.reduce_energy(self._t(e), self._t(logp), self._t(shift)))

    def energy_finish(self, sums4, shift, n):
        from fermiflow_amd import native
        return N(native.energy_finish(self._t(sums4), self._t(shift), n))

    def reduce_moments(self, e, shift=0.0, shift_dev=None, scale=1.0):
        from fermiflow_amd import native
        return N(native.reduce_moments(self._t(e), shift=shift, shift_dev=self._t(shift_dev), shift_dev_scale=scale))

    def beta(self, e, logp, ws, logits, beta, shift):
        """the three launches of BetaVMC's estimator, as VMC.py strings them together"""
        from fermiflow_amd import native
        ns = len(logits)
        et, sh = self._t(e), self._t(shift)
        buf = native.beta_buffer(ns, self.dev)
        native.reduce_moments(et, shift_dev=sh, out=buf[:2])
        native.beta_state_partials(et, self._t(logp), self._t(ws, torch.int32), ns, buf)
        est, gphi, mean_e, lpa = native.beta_finish(buf, sh, self._t(logits), beta, len(e))
        return N(buf[2:]).reshape(ns, R.SS_K, 4), N(est), N(gphi), N(mean_e), N(lpa)

    def walker_order(self, cost, hval=None):
        from fermiflow_amd import native
        if hval is None:
            return N(native.walker_order(self._t(cost, torch.int32)))
        order, hm = native.walker_order(self._t(cost, torch.int32), hval=self._t(hval))
        return N(order), N(hm)[0]

    def walker_schedule(self, cost, hval, tab, prev=None, interval=0.0, counts=None, shrink_at=0.0):
        from fermiflow_amd import native
        tab_out = torch.full((R.BINS,), float("nan"), dtype=torch.float64, device=self.dev)
        if prev is not None:
            prev = (self._t(prev[0], torch.int32), self._t(prev[1]), self._t(prev[2]))
        order, hm, hs = native.walker_schedule(self._t(cost, torch.int32), self._t(hval), self._t(tab), tab_out, prev=prev, interval=interval,
                                               counts=self._t(counts), shrink_at=shrink_at)
        return N(order), N(hm)[0], N(hs), N(tab_out)

    def scale_counts(self, cost, hs, he, interval=0.0, into=None):
        from fermiflow_amd import native, _lib as L
        ct, ht, et = self._t(cost, torch.int32), self._t(hs), self._t(he)
        if into is None:
            return N(native.scale_counts(ct, ht, et, interval))
        counts = self._t(into)      # the C entry point adds to what the buffer holds
        L.check(L.lib().ff_scale_counts(L.stream(), ct.numel(), L.ptr(ct), L.ptr(ht), L.ptr(et), interval, L.ptr(counts)),
                "ff_scale_counts")
        return N(counts)


@pytest.mark.parametrize("B", [1, 255, 1024, 1025, 65536, 262145, 300000])
def test_energy_estimate(dev, B):
    """262 145 walkers: 257 workgroups, the last one holding one walker; 300 000: 293 -- more than one per CU, on every XCD"""
    cases.energy_estimate(_Dev(dev), B)


def test_energy_estimate_back_to_back_on_one_workspace(dev):
    """200 calls at 300 000 walkers (293 workgroups over eight XCDs with an L2 each) on the cached workspace with no host sync in
    between: every result is bit-identical to the first (one summation order whichever workgroup finishes last; a partial read stale
    from another XCD's L2, or a counter not back at zero, breaks this), the first is inside the bound, the counter word reads 0.  Then a
    call on a second stream: its own workspace (a new key in native._EST_WS), the same bits, the first workspace untouched."""
    from fermiflow_amd import native
    B, shift = 300000, 29.5
    e, lp = R.energies(B)
    et, lt, sh = T(e, dev), T(lp, dev), T([shift], dev)
    main = torch.cuda.current_stream(dev)
    key = (str(et.device), int(main.cuda_stream), B)
    res = [native.energy_estimate(et, lt, sh, B) for _ in range(200)]
    ws = native._EST_WS[key]
    sums = torch.stack([r[0] for r in res]); est = torch.stack([r[1] for r in res])
    torch.cuda.synchronize(dev)
    sums, est = N(sums), N(est)
    want, mag = R.energy_sums(e, lp, shift)
    ewant, escale = R.energy_finish(e, lp, shift)
    fs, fe = R.frac(sums[0], want, R.SUM_TOL * mag), R.frac(est[0], ewant, R.FIN_TOL * escale)
    print(f"energy_estimate B={B}, 200 calls: sums4 {fs:.3f}, est3 {fe:.3f}  (fraction of the derived bound)")
    assert fs <= 1.0 and fe <= 1.0
    bad = [k for k in range(200) if not (bits_equal(sums[k], sums[0]) and bits_equal(est[k], est[0]))]
    assert not bad, bad
    assert int(ws[:1].view(torch.int32)[0].item()) == 0 and native._EST_WS[key] is ws
    side = torch.cuda.Stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        s2, e2 = native.energy_estimate(et, lt, sh, B)
    side.synchronize()
    key2 = (str(et.device), int(side.cuda_stream), B)
    assert key2 != key and key2 in native._EST_WS and native._EST_WS[key2] is not ws and native._EST_WS[key] is ws
    assert bits_equal(N(s2), sums[0]) and bits_equal(N(e2), est[0])
    s3, e3 = native.energy_estimate(et, lt, sh, B)
    torch.cuda.synchronize(dev)
    assert bits_equal(N(s3), sums[0]) and bits_equal(N(e3), est[0])
    assert int(ws[:1].view(torch.int32)[0].item()) == 0 and int(native._EST_WS[key2][:1].view(torch.int32)[0].item()) == 0


@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 2047, 2049, 65536])
def test_reduce_energy_and_finish(dev, B):
    """the edges of the two-stride loop of the 1024-thread workgroup"""
    cases.reduce_energy(_Dev(dev), B)


@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 2047, 2049, 65536])
def test_reduce_moments(dev, B):
    cases.reduce_moments(_Dev(dev), B)


@pytest.mark.parametrize("beta", [0.5, 3.0, 10.0])
@pytest.mark.parametrize("ns,B", [(1, 1), (1, 65536), (7, 403), (7, 65536), (300, 5000), (300, 65536)])
def test_beta_estimator(dev, ns, B, beta):
    """300 states loop the 256-thread state loops of ff_beta_finish_kernel; the state lists hold an empty state, a state of one walker
    and one of five (empty slices); one logit sits at -40"""
    for shift in (0.0, 29.5):
        cases.beta_estimator(_Dev(dev), ns, B, beta, shift)


def test_beta_estimator_every_walker_in_state_zero(dev):
    """production at beta = 10"""
    cases.beta_estimator(_Dev(dev), 7, 65536, 10.0, 29.5, one_state=True)


@pytest.mark.parametrize("B", [1, 511, 513, 4100, 65536, 200003])
def test_schedule(dev, B):
    """200 003 walkers: 391 segments -- ff_order_place_kernel walks them in strides of 8"""
    cases.schedule(_Dev(dev), B)


@pytest.mark.parametrize("B,e,shift,logits", R.ZERO_VARIANCE)
def test_zero_variance(dev, B, e, shift, logits):
    """A constant local energy: the centred sums of squares (differences of large numbers) are never negative, and sum (f - F)^2,
    formed about the shift like sum (e - E)^2, is inside 256 eps (sum (f - c0)^2 + n (F - c0)^2) -- formed from moments about zero it
    missed that bound by a factor of hundreds with the shift AT the mean (tests/test_estimators_hostsim.py::test_zero_variance has the
    figures).  sqrt(est / (n - 1)), what VMC._std reports, is finite."""
    cases.zero_variance(_Dev(dev), B, e, shift, logits)
