"""The estimator and schedule kernels of csrc/ff_walkers.hip under the host simulator, against tests/estimator_ref.py: the CPU twins of
tests/test_gpu_estimators.py (the same cases, tests/estimator_cases.py, at sizes the simulator runs in seconds), so that the references
and expectations are checked before a GPU sees them.  The simulator's reduction workgroups have 4 threads (hip_shim.h: FF_RBLOCK), so
its serial chains are longer than the device's; the bounds are the device's all the same."""

import numpy as np
import pytest

from tests import estimator_cases as cases
from tests import estimator_ref as R
from tests.hostsim import simlib as S


class _Sim:
    """the backend of tests/estimator_cases.py over the host-simulated library"""
    energy_finish = staticmethod(S.energy_finish)
    reduce_energy = staticmethod(S.reduce_energy)
    walker_schedule = staticmethod(S.walker_schedule)

    @staticmethod
    def energy_estimate(e, logp, shift, n_global):
        sums, est, ws = S.energy_estimate(e, logp, shift, n_global)
        assert ws.view(np.uint32)[0] == 0
        return sums, est

    @staticmethod
    def reduce_moments(e, shift=0.0, shift_dev=None, scale=1.0):
        e = S._d(e); out = np.empty(2)
        sd = None if shift_dev is None else np.array([shift_dev], dtype=np.float64)
        S._ck(S.lib().ff_reduce_moments(None, len(e), S._p(e), shift, S._p(sd), scale, S._p(out)))
        return out

    @staticmethod
    def beta(e, logp, ws, logits, beta, shift):
        e, logp, ws, logits = S._d(e), S._d(logp), S._i(ws), S._d(logits)
        ns = len(logits)
        buf = np.zeros(S.lib().ff_beta_buffer_doubles(ns))
        sh = np.array([shift], dtype=np.float64)
        buf[:2] = _Sim.reduce_moments(e, shift_dev=shift, scale=1.0)
        S._ck(S.lib().ff_beta_state_partials(None, len(e), ns, S._p(ws), S._p(e), S._p(logp), S._p(buf)))
        est, gphi, mean_e, lpa = np.empty(8), np.empty(ns), np.empty(ns), np.empty(ns)
        S._ck(S.lib().ff_beta_finish(None, S._p(buf), S._p(sh), S._p(logits), ns, beta, len(e), S._p(est), S._p(gphi), S._p(mean_e), S._p(lpa)))
        return buf[2:].reshape(ns, R.SS_K, 4).copy(), est, gphi, mean_e, lpa

    @staticmethod
    def walker_order(cost, hval=None):
        r = S.walker_order(cost, hval)
        return r if hval is None else (r[0], np.float64(r[1]))

    @staticmethod
    def scale_counts(cost, hs, he, interval=0.0, into=None):
        if into is None:
            return S.scale_counts(cost, hs, he, interval)
        cost, into = S._i(cost), np.array(into, dtype=np.float64)
        S._ck(S.lib().ff_scale_counts(None, len(cost), S._p(cost), S._p(S._d(hs)), S._p(S._d(he)), interval, S._p(into)))
        return into


@pytest.mark.parametrize("B", [1, 255, 1024, 1025, 5000])
def test_energy_estimate(B):
    cases.energy_estimate(_Sim, B)


def test_energy_estimate_workspace_serves_call_after_call():
    """the counter is left at zero: one workspace, twenty calls, one result"""
    e, lp = R.energies(5000)
    first, est, ws = S.energy_estimate(e, lp, 29.5, 5000)
    for _ in range(20):
        sums, est2, ws = S.energy_estimate(e, lp, 29.5, 5000, ws=ws)
        assert cases.bits_equal(sums, first) and cases.bits_equal(est2, est) and ws.view(np.uint32)[0] == 0


@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 2047, 2049, 5000])
def test_reduce_energy_and_finish(B):
    cases.reduce_energy(_Sim, B)


@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 2047, 2049, 5000])
def test_reduce_moments(B):
    cases.reduce_moments(_Sim, B)


@pytest.mark.parametrize("beta", [0.5, 3.0, 10.0])
@pytest.mark.parametrize("ns,B", [(1, 1), (1, 5000), (7, 403), (7, 5000), (300, 5000)])
def test_beta_estimator(ns, B, beta):
    for shift in (0.0, 29.5):
        cases.beta_estimator(_Sim, ns, B, beta, shift)


def test_beta_estimator_every_walker_in_state_zero():
    cases.beta_estimator(_Sim, 7, 5000, 10.0, 29.5, one_state=True)


@pytest.mark.parametrize("B", [1, 511, 513, 4100, 5000])
def test_schedule(B):
    cases.schedule(_Sim, B)


@pytest.mark.parametrize("B,e,shift,logits", R.ZERO_VARIANCE)
def test_zero_variance(B, e, shift, logits):
    """A constant local energy (non-interacting known-answer flows: constant to the ODE tolerance; and the first sweep of every run has
    shift 0): the centred sums of squares are differences of large numbers and came out negative, so E_std / F_std were NaN.  The
    kernels as they were, under this simulator (beta = 3, three equally weighted states):

        B      e     shift   ff_energy_estimate est[1]   ff_beta_finish est[3] (F_ss)
        1000   20.1  0       -1.98e-09                   -4.07e-10
        4097   20.1  0       -1.00e-08                   -7.2e-09
        65536  20.1  0       -1.60e-07                   +2.6e-07
        65536  20.1  20.1     0                          -2.79e-07
        65536  13.7  0       +1.3e-07                    -9.1e-07

    Every one of these rows failed this test (a negative sum of squares), and a clamp alone mends them: with equal logits f is constant
    and the exact sum (f - F)^2 is 0.  The rows with logits (0, -1, -2) and the shift at the mean are about the formula: there
    sum (f - F)^2 = 4854.55..., its bound 256 eps (sum (f - c0)^2 + n (F - c0)^2) = 1.9e-09, and F_ss formed from moments about zero
    -- its error about n E^2 eps whatever the shift -- misses it with or without the clamp.  The old formula with the clamp kept, run
    once under this simulator, against the formula about the shift (error as a fraction of the bound):

        65536  20.1  20.1   old 141.5 (-2.7e-07)   new 0.043
        65536  13.7  13.7   old  79.2 (+1.5e-07)   new 0.001
        65536  30.0  30.0   old  0.43 (+8.3e-10)   new 0.002    (30 n and 900 n are exact in binary: little to lose)

    (With equal logits and the same fourth row the bound is 1.0e-09 and the parent's -2.79e-07 is 280 times past it.)  What the formula
    about the shift keeps is the rounding the per-state sums of e already carry, about n_s |E| eps each, times 2 |c_s - (F - c0)|:
    linear in E, 1e-10 here."""
    cases.zero_variance(_Sim, B, e, shift, logits)

