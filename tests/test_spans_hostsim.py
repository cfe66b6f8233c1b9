"""The ODE kernels at time spans other than (0, 1) under the host simulator: the CPU twin of tests/test_gpu_spans.py (the same cases,
tests/span_cases.py).  A simulated launch costs seconds whatever its size, so the simulator takes a stated subset: one plain solve per
call (the flow at 3 x 2 over (2, 0.5), the local energy at 2 + 1 over (1, 0), the tabulated adjoint at 3 + 3 over (0.25, 1.75)), the
slot checks at 3 x 2 reversed, the opening steps of the flow at 3 x 2 over (1, 0) and of the local energy at 2 + 1 over (2, 0.5), the
equal steps over (2, 0.5), the clamp over (0.1, 0.7), and the empty interval at 3 x 2 and 2 + 1.  The simulator's build has no
matrix-core kernel (tests/hostsim/Makefile): that kernel, its heavy route, every other shape and span, the autograd wrappers and the
sweeps are the device's.  The device's second reference of the autograd wrappers (RK4 with autograd) is checked against the oracle here."""
import contextlib

import numpy as np
import pytest

from tests import span_cases as cases
from tests.hostsim import simlib as S

_NETS = {}


def _backend(golden):
    from fermiflow_amd import native

    @contextlib.contextmanager
    def warmed(hout, h_init=None, h_scale=1.0, uniform=False, equal=False, max_steps=0):
        S.warm(h_out=hout, h_init=None if h_init is None else np.ascontiguousarray(h_init, dtype=np.float64), h_scale=h_scale, uniform=uniform,
               max_steps=max_steps, h_equal=equal)
        try:
            yield
        finally:
            S.warm()

    class Sim:
        gp_reproducible = False

        @staticmethod
        def plan(call, n, d):
            fam, g, _ = S.kernel_plan(native.PLAN_CALLS.index(call), n, d, 2)
            return native.PLAN_FAMILIES[fam], g

        @staticmethod
        def net(s, table):
            if (s, table) not in _NETS:
                _NETS[s, table] = S.Net(*cases.weights(golden, s), table=table)
            return _NETS[s, table]

        @staticmethod
        def generate(net, z, t0, t1, order=None, **warm):
            B = len(z)
            cost = np.full(B, -1, dtype=np.int32); hout = np.zeros(B)
            with warmed(hout, **warm):
                x, st = S.cnf_generate(z, net, t0, t1, cases.RT, cases.AT, steps=cost, order=order)
            return x, cost, hout, st

        @staticmethod
        def delta_logp(net, x, t0, t1):
            return S.cnf_delta_logp(x, net, t0, t1, cases.RT, cases.AT)

        @staticmethod
        def eloc(net, x, nup, ndn, Z, t0, t1, **warm):
            hout = np.zeros(len(x))
            with warmed(hout, **warm):
                r = S.eloc_nd(x, nup, ndn, net, Z, True, t0, t1, cases.RT, cases.AT, compact=False)
            r["hout"] = hout
            return r

        @staticmethod
        def adjoint(net, y, a_z, a_d, t0, t1, **warm):
            with warmed(None, **warm):
                return S.cnf_adjoint(y, a_z, a_d, net, t0, t1, cases.RT, cases.AT)
    return Sim


def test_plain_solves_vs_oracle_and_identity(golden):
    K = _backend(golden)
    cases.flow_case(K, golden, 3, 2, True, (2.0, 0.5))
    cases.eloc_case(K, golden, 2, 1, 2, True, (1.0, 0.0))
    cases.adjoint_case(K, golden, 6, 2, True, (0.25, 1.75))
    cases.report("host simulator")


def test_walker_is_the_same_in_every_batch_slot_and_order(golden):
    cases.slots_case(_backend(golden), golden, 3, 2, (1.0, 0.0))


def test_opening_steps(golden):
    K = _backend(golden)
    cases.open_flow_case(K, golden, 3, 2, (1.0, 0.0))
    cases.open_eloc_case(K, golden, 2, 1, (2.0, 0.5))
    cases.equal_case(K, golden, (2.0, 0.5))
    cases.clamp_case(K, golden, (0.1, 0.7))


def test_empty_interval(golden):
    K = _backend(golden)
    cases.empty_flow_case(K, golden, 3, 2, True)
    cases.empty_eloc_case(K, golden, 2, 1, 2, 4.0, True)


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("n,d", cases.AUTOGRAD_SHAPES)
def test_rk4_reference_agrees_with_the_oracle(golden, n, d, use_mu):
    """The two references of the device's autograd tests against each other at the span with the largest truncation error, (2, 0.5):
    autograd through 128 RK4 steps of the plain field and the oracle's hand-derived adjoint agree within a tenth of BAR_GP (measured:
    3.6e-11 at the worst of all spans, shapes and nets)."""
    e_gen, e_dl = cases.rk4_vs_oracle(golden, n, d, use_mu, (2.0, 0.5))
    assert e_gen < cases.BAR_GP / 10 and e_dl < cases.BAR_GP / 10, (e_gen, e_dl)
