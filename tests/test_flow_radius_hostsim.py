"""The tabulated flow kernel's radius and component phases under the host simulator: the CPU twin of tests/test_gpu_flow_radius.py (the
same cases, tests/flow_radius_cases.py).  A simulated launch costs seconds whatever its size, so the simulator takes the benchmark's
shape (6 particles in two dimensions: the largest walker, a half-full second radius slot) with and without a one-body net and the
three-dimensional shape with four particles with one, each at the batches of 2 G + 3 and G + 1 walkers, the special walkers at 6 x 2
with a one-body net and at 3 x 2 without; every other shape and batch is the device's."""
import numpy as np
import pytest

from tests import flow_radius_cases as cases
from tests import frames_ref as F
from tests.common import cu_count
from tests.hostsim import simlib as S

_NETS = {}


def _backend(golden):
    from fermiflow_amd import native

    class Sim:
        @staticmethod
        def group(n, d):
            fam, g, _ = S.kernel_plan(native.PLAN_CALLS.index("flow"), n, d, cu_count(hostsim=True))
            assert native.PLAN_FAMILIES[fam] == "narrow"
            return g

        @staticmethod
        def net(use_mu, table):
            if (use_mu, table) not in _NETS:
                _NETS[use_mu, table] = S.Net(*cases.weights(golden, use_mu), table=table)
            return _NETS[use_mu, table]

        @staticmethod
        def generate(net, z, order):
            B = len(z)
            cost = np.full(B, -1, dtype=np.int32); hout = np.zeros(B)
            S.warm(h_out=hout)
            try:
                x, st = S.cnf_generate(z, net, rtol=cases.RT, atol=cases.AT, steps=cost, order=order)
            finally:
                S.warm()
            return x, cost, hout, st

        @staticmethod
        def frames(net, z, nframes, order):
            return F.sim_frames(S, z, net, nframes, rtol=cases.RT, atol=cases.AT, order=order)[1]
    return Sim


@pytest.mark.parametrize("n,d,use_mu", [(6, 2, True), (6, 2, False), (4, 3, True)])
def test_batches_orders_and_oracle(golden, n, d, use_mu):
    cases.flow_case(_backend(golden), golden, n, d, use_mu, which=(-2,))


@pytest.mark.parametrize("n,d,use_mu", [(6, 2, True), (3, 2, False)])
def test_off_table_radius_and_nan_coordinate(golden, n, d, use_mu):
    cases.special_case(_backend(golden), golden, n, d, use_mu)
