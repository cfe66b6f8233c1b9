"""The Philox-fed samplers' ground dispatch on the device (tests/sampler_ground_cases.py): every spin shape (1, 1) .. (6, 6) and every
pair shape (2, 0) .. (6, 0) on a ground launch, the four kinds of launch that are NOT ground at every one of those shapes that has
them, and the special walkers on a ground launch -- the Philox-fed chain, the continued chain and the noise-fed chain on the
materialised stream are one chain, bit for bit, at batches of 1, 7 and 130 walkers."""
import pytest
import torch

from tests import sampler_ground_cases as cases
from tests.common import N, T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    from fermiflow_amd import native

    def tab(t):
        return None if t is None else T(t, dev, torch.int32)

    def st(ws):
        return None if ws is None else T(ws, dev, torch.int32)

    class Dev:
        @staticmethod
        def rng_fill(B, n, steps, seed, offset):
            return tuple(N(t) for t in native.rng_fill(B, n, steps, seed, dev, walker_offset=offset))

        @staticmethod
        def noise(nup, ndn, g0, g, u, tu, td, ws):
            return tuple(N(t) for t in native.mcmc_sample_noise(tab(tu), tab(td), nup, ndn, T(g0, dev), T(g, dev), T(u, dev),
                                                                walker_state=st(ws)))

        @staticmethod
        def sample(B, nup, ndn, steps, seed, offset, tu, td, ws):
            return tuple(N(t) for t in native.mcmc_sample(tab(tu), tab(td), nup, ndn, B, steps, 0.1, seed, dev, walker_offset=offset,
                                                          walker_state=st(ws)))

        @staticmethod
        def cont(x0, nup, ndn, steps, seed, offset, tu, td, ws):
            return tuple(N(t) for t in native.mcmc_continue(tab(tu), tab(td), nup, ndn, T(x0, dev), steps, 0.1, seed,
                                                            walker_offset=offset, walker_state=st(ws)))
    return Dev


@pytest.mark.parametrize("nup,ndn", cases.SPIN_SHAPES + cases.PAIR_SHAPES)
def test_ground_launch_is_the_noise_fed_chain(K, nup, ndn):
    cases.chain_case(K, nup, ndn)


@pytest.mark.parametrize("nup,ndn,kind", cases.nonground_cases(cases.SPIN_SHAPES + cases.PAIR_SHAPES))
def test_launch_one_step_from_ground_takes_the_run_time_degrees(K, nup, ndn, kind):
    cases.chain_case(K, nup, ndn, kind)


@pytest.mark.parametrize("nup,ndn", [(2, 2), (3, 3), (6, 6), (3, 0), (6, 0)])
def test_special_walkers_on_a_ground_launch(K, nup, ndn):
    cases.special_case(K, nup, ndn)
