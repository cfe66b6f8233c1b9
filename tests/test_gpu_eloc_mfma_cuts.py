"""The matrix-core local-energy kernel on the device at 1+1, 2+1, 2+2, 3+2 and 3+3 particles (one to three 4 x 4 blocks per side, a last
block that is full and one that is not, one and two radius slots per lane, the fused finish at the even shapes and the workspace path at
the odd ones), with and without a one-body net, radial table and direct evaluation, on batches of 3, 4, 5 and 9 walkers and with an
explicit walker order (tests/eloc_mfma_cases.py): E_loc, gradient and Laplacian against the oracle, every output of a walker bit for
bit the same in every batch it appears in, no failed walker."""
import pytest

from tests import eloc_mfma_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nup,ndn", cases.SHAPES)
def test_matrix_core_local_energy_shapes_batches_order_and_missing_one_body_net(nup, ndn):
    cases.run_child("gpu", nup, ndn, "full", timeout=300)
