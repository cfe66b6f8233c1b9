"""The tabulated adjoint under the host simulator at every deposit-row length, on ragged batches, with and without a one-body net:
the CPU twin of tests/test_gpu_adjtab_rows.py (the same cases, tests/adjtab_cases.py).  A simulated launch costs seconds whatever
its size (every lane is a host thread that spends its time in barrier wake-ups), so the simulator takes each shape and each row
length once, at the batch of 2 G + 1 walkers -- three groups, the last one ragged, the second workgroup with one live wave --, the
batches of 1 and 2 walkers at 3+3 with eight coefficients (the benchmark's kernel and row length) and 2+2 at eight coefficients (the
eight-coefficient copy of the deposit at a second shape).  The 193 walkers, the remaining combinations and the repeated call (the
simulator's atomics are unordered) are the device's: 7 of the 64 (shape, rows, batch) combinations run here."""
import numpy as np
import pytest

from tests import adjtab_cases as cases
from tests.hostsim import simlib as S


class _Sim:
    ordered_atomics = False

    @staticmethod
    def net(eta, mu, table):
        return S.Net(eta, mu, table=table)

    @staticmethod
    def header(net):
        return net.tab[:6]

    @staticmethod
    def group(n, d):
        from fermiflow_amd import native
        fam, g, _ = S.kernel_plan(native.PLAN_CALLS.index("adjoint"), n, d, 2)
        assert native.PLAN_FAMILIES[fam] == "tabulated"
        return g

    @staticmethod
    def adjoint(net, z, a_z, a_d, rtol, atol):
        gx, gp, st = S.cnf_adjoint(z, a_z, a_d, net, rtol=rtol, atol=atol)
        assert int(st[3]) == 0
        return gx, gp


@pytest.mark.parametrize("nup,ndn,rows,which", [(1, 1, 6, (2,)), (3, 0, 8, (2,)), (2, 2, 10, (2,)), (3, 3, 12, (2,)), (3, 3, 8, (0, 1)),
                                                   (2, 2, 8, (2,))])
def test_tabulated_adjoint_rows_batches_and_missing_one_body_net(nup, ndn, rows, which):
    cases.rows_case(_Sim, nup, ndn, rows, which=which)
