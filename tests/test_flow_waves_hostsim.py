"""The tabulated flow kernel's walker-group head and tail under the host simulator: the CPU twin of tests/test_gpu_flow_waves.py (the
same cases, tests/flow_waves_cases.py).  A simulated launch costs seconds whatever its size, so the simulator takes a stated subset:
the slot checks at the benchmark's shape (6 particles in two dimensions, with a one-body net, the benchmark's weights) and at three
particles in three dimensions without one at the stiff weights, each at the batches of G and G + 1 walkers; the warm start at 6 x 2 with
a one-body net; the table's end and the non-finite coordinate at 2 x 2 with one.  Every other shape, scale and batch is the device's."""
import numpy as np
import pytest

from tests import flow_waves_cases as cases
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
        def net(scale, use_mu, table):
            if (scale, use_mu, table) not in _NETS:
                _NETS[scale, use_mu, table] = S.Net(*cases.weights(golden, scale, use_mu), table=table)
            return _NETS[scale, use_mu, table]

        @staticmethod
        def generate(net, z, order=None, h_init=None, uniform=False, max_steps=0):
            B = len(z)
            cost = np.full(B, -1, dtype=np.int32); hout = np.zeros(B)
            S.warm(h_out=hout, h_init=None if h_init is None else np.ascontiguousarray(h_init, dtype=np.float64), uniform=uniform,
                   max_steps=max_steps)
            try:
                x, st = S.cnf_generate(z, net, rtol=cases.RT, atol=cases.AT, steps=cost, order=order)
            finally:
                S.warm()
            return x, cost, hout, st

        @staticmethod
        def frames(net, z, nframes, order=None):
            return F.sim_frames(S, z, net, nframes, rtol=cases.RT, atol=cases.AT, order=order)[1]
    return Sim


@pytest.mark.parametrize("scale,n,d,use_mu", [("bench", 6, 2, True), ("stiff", 3, 3, False)])
def test_walker_is_the_same_in_every_batch_slot_and_order(golden, scale, n, d, use_mu):
    cases.slots_case(_backend(golden), golden, scale, n, d, use_mu, which=(-3, -2))


def test_uniform_and_per_walker_warm_start(golden):
    cases.warm_case(_backend(golden), golden, "bench", 6, 2, True)


def test_table_end_and_non_finite_coordinate(golden):
    cases.special_case(_backend(golden), golden, "bench", 2, 2, True)
