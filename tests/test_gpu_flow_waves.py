"""The tabulated flow kernel's walker-group head and tail on the device (tests/flow_waves_cases.py): native.cnf_generate
and CNF.generate(z, nframes = 3) at n = 1 .. 6 in two dimensions and 2, 3 in three, with and without a one-body net, at the benchmark's
weights and at the finest table's (max|w1| = 25), at batches of 1, G - 1, G, G + 1 and 2 G + 3 walkers, in reverse and under an explicit
order -- x, walker_cost and walker_h_out bit-identical whatever batch and slot a walker sits in, within the bar of the existing flow
tests of the oracle; the uniform and the per-walker warm start; a radius just below, at and beyond the table's end; a non-finite
coordinate.  The stiff scale runs the slot checks and the warm start at every shape and leaves the special walkers to the benchmark's."""
import numpy as np
import pytest
import torch

from tests import flow_waves_cases as cases
from tests.common import N, T, cu_count, make_flow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K(golden):
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    from fermiflow_amd import native
    nets = {}

    class Dev:
        @staticmethod
        def group(n, d):
            fam, g, _ = native.kernel_plan("flow", n, d, cu_count())
            assert fam == "narrow"
            return g

        @staticmethod
        def net(scale, use_mu, table):
            if (scale, use_mu, table) not in nets:
                cnf = make_flow(*cases.weights(golden, scale, use_mu), dev)
                cnf.rtol, cnf.atol = cases.RT, cases.AT
                nets[scale, use_mu, table] = (cnf, cnf.v_wrapper.v.net(radial="table" if table else "exact"), table)
            return nets[scale, use_mu, table]

        @staticmethod
        def generate(h, z, order=None, h_init=None, uniform=False, max_steps=0):
            B = len(z)
            cost = torch.full((B,), -1, dtype=torch.int32, device=dev)
            hout = torch.zeros(B, dtype=torch.float64, device=dev)
            warm = {} if h_init is None else dict(walker_h_init=T(h_init, dev), walker_h_uniform=uniform, max_steps=max_steps)
            x, st = native.cnf_generate(h[1], T(z, dev), 0.0, 1.0, cases.RT, cases.AT, want_stats=True, walker_cost=cost,
                                        walker_order=None if order is None else T(order, dev, torch.int32), walker_h_out=hout, **warm)
            return N(x), N(cost), N(hout), N(st)

        @staticmethod
        def frames(h, z, nframes, order=None):
            fr, _ = native.cnf_generate_frames(h[1], T(z, dev), nframes, 0.0, 1.0, cases.RT, cases.AT,
                                               walker_order=None if order is None else T(order, dev, torch.int32))
            return N(fr)
    return Dev


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("n,d", cases.SHAPES)
@pytest.mark.parametrize("scale", cases.SCALES)
def test_walker_is_the_same_in_every_batch_slot_and_order(K, golden, scale, n, d, use_mu):
    cases.slots_case(K, golden, scale, n, d, use_mu)


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("n,d", cases.SHAPES)
@pytest.mark.parametrize("scale", cases.SCALES)
def test_uniform_and_per_walker_warm_start(K, golden, scale, n, d, use_mu):
    cases.warm_case(K, golden, scale, n, d, use_mu)


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("n,d", cases.SHAPES)
def test_table_end_and_non_finite_coordinate(K, golden, n, d, use_mu):
    cases.special_case(K, golden, "bench", n, d, use_mu)
