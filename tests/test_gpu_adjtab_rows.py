"""The tabulated adjoint on the device at every deposit-row length (6, 8, 10, 12 coefficients), at 1+1, 3+0, 2+2 and 3+3 particles, on
batches of 1, 2, 2 G + 1 and 193 walkers, with and without a one-body net (tests/adjtab_cases.py): parameter gradient against the
direct-evaluation kernel, bit-reproducibility, finite gradients from the zeroed diagonal of the exchange buffer."""
import pytest
import torch

from tests import adjtab_cases as cases
from tests.common import N, T, cu_count, make_flow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


def _backend(dev):
    from fermiflow_amd import native

    class K:
        ordered_atomics = True

        @staticmethod
        def net(eta, mu, table):
            return make_flow(eta, mu, dev).v_wrapper.v.net(radial="table" if table else "exact")

        @staticmethod
        def header(net):
            return N(net.t[-1])[:6]

        @staticmethod
        def group(n, d):
            fam, g, _ = native.kernel_plan("adjoint", n, d, cu_count())
            assert fam == "tabulated"
            return g

        @staticmethod
        def adjoint(net, z, a_z, a_d, rtol, atol):
            gx, gp, st = native.cnf_adjoint(net, T(z, dev), T(a_z, dev), T(a_d, dev), 0.0, 1.0, rtol, atol, want_stats=True)
            assert int(st[3]) == 0
            return N(gx), N(gp)
    return K


@pytest.mark.parametrize("rows", sorted(cases.ROWS))
@pytest.mark.parametrize("nup,ndn", cases.SHAPES)
def test_tabulated_adjoint_rows_batches_and_missing_one_body_net(dev, nup, ndn, rows):
    cases.rows_case(_backend(dev), nup, ndn, rows)
