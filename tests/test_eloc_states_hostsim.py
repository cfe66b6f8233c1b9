"""The finish paths of the local energy at excited and per-walker orbital sets under the host simulator: the CPU twin of
tests/test_gpu_eloc_states.py (the same cases, tests/eloc_states_cases.py, at the sizes its SIM table gives: a simulated workgroup
of the one-walker-per-workgroup kernels costs seconds per walker).  The matrix-core kernel (F1) and the heavy-walker route beside it
(F6, at 2+2 and 3+3 with the simulator's batch of 13 walkers: routed_setup) run in child processes with FF_ELOC_KERNEL=mfma."""
import pytest

from tests import eloc_states_cases as cases


@pytest.fixture(scope="module")
def K():
    return cases.sim_backend()


@pytest.mark.parametrize("name", cases.sim_cases())
def test_finish_path_at_per_walker_orbital_sets(K, name):
    if cases.CASES[name][4] == "mfma":
        cases.forced_kernel_ran("sim", name, timeout=1800)
    else:
        cases.run_case(K, name)


def test_wide_fused_finish_common_excited_table(K):
    cases.run_common_table(K)


def test_wide_fused_finish_two_states_in_one_workgroup(K):
    cases.run_looping(K)


@pytest.mark.parametrize("nup,ndn", [(2, 2), (3, 3)])
def test_heavy_route_finishes_walkers_of_different_states(nup, ndn):
    cases.run_child("sim", f"F6-{nup}+{ndn}", timeout=1800)


@pytest.mark.parametrize("nup,ndn,d", cases.LOGPROB_SHAPES)
def test_logprob_derivatives_under_walker_state(K, nup, ndn, d):
    cases.run_logprob(K, nup, ndn, d)
