"""The matrix-core local-energy kernel under the host simulator at one to three blocks per side: the CPU twin of
tests/test_gpu_eloc_mfma_cuts.py (the same cases, tests/eloc_mfma_cases.py).  A simulated launch of this kernel costs seconds
per walker group (every lane is a host thread, every exchange a barrier of 64 of them), so the simulator
takes one walker group with an idle slot (three walkers) per shape, alternating the two combinations that differ in every cut -- the
table kernel with a one-body net at 2+2 and 3+3 (the fused finish), the direct kernel without one at 2+1 and 3+2 (the workspace
stores) -- and at 1+1, where a launch is cheap, both of them, the table kernel at five walkers (two groups, the second with idle
slots) in the given order and in an explicit one.  The full groups, the three groups of nine walkers and the remaining combinations
are the device's: 7 of the 100 (shape, net, kernel, batch / order) launches run here."""
import pytest

from tests import eloc_mfma_cases as cases


@pytest.mark.parametrize("nup,ndn,plan", [(1, 1, "mt:5o,nd:3"), (2, 1, "nd:3"), (2, 2, "mt:3"), (3, 2, "nd:3"), (3, 3, "mt:3")])
def test_matrix_core_local_energy_shapes_batches_order_and_missing_one_body_net(nup, ndn, plan):
    cases.run_child("sim", nup, ndn, plan)
