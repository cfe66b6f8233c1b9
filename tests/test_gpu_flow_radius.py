"""The tabulated flow kernel's radius and component phases on the device (tests/flow_radius_cases.py): native.cnf_generate and
CNF.generate(z, nframes = 3) at n = 1, 2, 3, 5, 6 in two dimensions and n = 2, 4 in three, with and without a one-body net, at batches
of 1, G - 1, G + 1 and 2 G + 3 walkers and under an explicit order -- bit-identical across batches and orders (outputs, walker_cost,
walker_h_out), within the bar of test_flow_at_looping_batch_vs_oracle of the oracle; a radius beyond the table, a NaN coordinate."""
import numpy as np
import pytest
import torch

from tests import flow_radius_cases as cases
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
        def net(use_mu, table):
            if (use_mu, table) not in nets:
                cnf = make_flow(*cases.weights(golden, use_mu), dev)
                cnf.rtol, cnf.atol = cases.RT, cases.AT
                nets[use_mu, table] = (cnf, cnf.v_wrapper.v.net(radial="table" if table else "exact"), table)
            return nets[use_mu, table]

        @staticmethod
        def generate(h, z, order):
            B = len(z)
            cost = torch.full((B,), -1, dtype=torch.int32, device=dev)
            hout = torch.zeros(B, dtype=torch.float64, device=dev)
            x, st = native.cnf_generate(h[1], T(z, dev), 0.0, 1.0, cases.RT, cases.AT, want_stats=True, walker_cost=cost,
                                        walker_order=None if order is None else T(order, dev, torch.int32), walker_h_out=hout)
            return N(x), N(cost), N(hout), N(st)

        @staticmethod
        def frames(h, z, nframes, order):
            if order is None and h[2]:
                return N(h[0].generate(T(z, dev), nframes=nframes))
            fr, _ = native.cnf_generate_frames(h[1], T(z, dev), nframes, 0.0, 1.0, cases.RT, cases.AT,
                                               walker_order=None if order is None else T(order, dev, torch.int32))
            return N(fr)
    return Dev


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("n,d", cases.SHAPES)
def test_batches_orders_and_oracle(K, golden, n, d, use_mu):
    cases.flow_case(K, golden, n, d, use_mu)


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("n,d", cases.SHAPES)
def test_off_table_radius_and_nan_coordinate(K, golden, n, d, use_mu):
    cases.special_case(K, golden, n, d, use_mu)
