"""The Philox-fed samplers' ground dispatch under the host simulator: the CPU twin of tests/test_gpu_sampler_ground.py (the same
cases, tests/sampler_ground_cases.py).  A simulated lane exchange is a barrier of host threads, and the pair kernels exchange every
matrix entry, so the simulator runs a subset: on a ground launch the smallest, the benchmark's and the largest spin shape and the
two smallest pair shapes, at every batch; the four launches that are not ground at 3 + 3 and the one whose last orbital differs at
3 + 0; the special walkers at 3 + 3.  The remaining shapes and combinations are the device's."""
import numpy as np
import pytest

from tests import sampler_ground_cases as cases
from tests.hostsim import simlib as S


class _Sim:
    @staticmethod
    def rng_fill(B, n, steps, seed, offset):
        return S.rng_fill(B, n, steps, seed, offset=offset)

    @staticmethod
    def noise(nup, ndn, g0, g, u, tu, td, ws):
        return S.mcmc_noise(g0, g, u, nup, ndn, tab_up=tu, tab_dn=td, wstate=ws)

    @staticmethod
    def sample(B, nup, ndn, steps, seed, offset, tu, td, ws):
        tu, td = S._tabs(nup, ndn, tu, td); ws = None if ws is None else S._i(ws)
        x = np.empty((B, nup + ndn, 2)); lp = np.empty(B); cnt = np.empty(B, dtype=np.int32)
        S._ck(S.lib().ff_mcmc_sample(None, B, nup, ndn, S._p(tu), S._p(td), S._p(ws), steps, 0.1, seed, offset, S._p(x), S._p(lp), S._p(cnt)))
        return x, lp, cnt

    @staticmethod
    def cont(x0, nup, ndn, steps, seed, offset, tu, td, ws):
        x0 = S._d(x0); B = x0.shape[0]
        tu, td = S._tabs(nup, ndn, tu, td); ws = None if ws is None else S._i(ws)
        x = np.empty_like(x0); lp = np.empty(B); cnt = np.empty(B, dtype=np.int32)
        S._ck(S.lib().ff_mcmc_continue(None, B, nup, ndn, S._p(tu), S._p(td), S._p(ws), steps, 0.1, seed, offset, S._p(x0), S._p(x), S._p(lp),
                                       S._p(cnt)))
        return x, lp, cnt


@pytest.mark.parametrize("nup,ndn", [(1, 1), (3, 3), (6, 6), (2, 0), (3, 0)])
def test_ground_launch_is_the_noise_fed_chain(nup, ndn):
    cases.chain_case(_Sim, nup, ndn)


@pytest.mark.parametrize("nup,ndn,kind", cases.nonground_cases([(3, 3)]) + [(3, 0, "up_last")])
def test_launch_one_step_from_ground_takes_the_run_time_degrees(nup, ndn, kind):
    cases.chain_case(_Sim, nup, ndn, kind)


@pytest.mark.parametrize("nup,ndn", [(3, 3)])
def test_special_walkers_on_a_ground_launch(nup, ndn):
    cases.special_case(_Sim, nup, ndn)
