"""The samplers and log-densities at walkers where the Slater matrix is singular or its entries leave the double range.

Every other sampler test starts from normal walkers.  Here the walkers are crafted (tests/golden/g8_sampler_edges.npz, written by
make_golden.py edges from the reference itself, and tests/common.py):
  * every particle at the origin or on one axis: a column of the Slater matrix is exactly zero, log p = -inf (LAPACK's zero
    pivot), and a chain started there accepts its first proposal (p = exp(+inf));
  * rings at radius 8 .. 30: log p down to about -2 10^4, where the product of the pivots -- each carries its row's Gaussian --
    is far below the smallest double;
  * a NaN coordinate: the walker never moves, log p stays NaN, and nothing else changes;
  * coincident same-spin particles (identical rows): the determinant is exactly 0, log p = -inf, as in the oracle and in exact
    arithmetic.  The reference returns a finite value there that depends on LAPACK's rounding; that is a deliberate deviation
    ("Behavioural differences"), not a tolerance.
Families (csrc/ff_mcmc.h): ff_mcmc_kernel (register-resident one lane per walker: (10, 0)), ff_mcmc_spin_kernel /
ff_mcmc_spin_philox_kernel (nup = ndn), ff_mcmc_pair_kernel (ndn = 0); csrc/ff_ho3d.hip: ff_mcmc_rows_kernel (sixteen lanes: (2, 1),
(4, 3), (7, 6), (0, 7) and d = 3).  ff_mcmc_kernel has compile-time sizes only; shapes outside the template list go to the sixteen-lane kernel.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.common import (EDGE_CHAINS, EDGE_SHAPES, EDGE_SHAPES3D, N, T, assert_edge_logp, bits_equal, coincident_chains,
                          edge_chain, sampler_edges, special_starts)

pytestmark = pytest.mark.gpu

FAMILIES = [(3, 3), (6, 0), (10, 0), (2, 1), (4, 3), (7, 6), (0, 7)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g8():
    return sampler_edges()


def _tabs(nup, ndn, dev):
    from fermiflow_amd import native
    return (native.orbital_table(list(range(nup)), dev) if nup else None,
            native.orbital_table(list(range(ndn)), dev) if ndn else None)


def _noise(nup, ndn, x0, g, u, dev, ws=None, tabs=None):
    from fermiflow_amd import native
    tu, td = tabs or _tabs(nup, ndn, dev)
    fn = native.mcmc_sample_noise3d if x0.shape[-1] == 3 else native.mcmc_sample_noise
    x, lp, acc = fn(tu, td, nup, ndn, T(x0, dev), T(g, dev), T(u, dev), walker_state=None if ws is None else T(ws, dev, torch.int32))
    return N(x), N(lp), N(acc)


def _philox(nup, ndn, x0, steps, seed, dev, ws=None, tabs=None):
    from fermiflow_amd import native
    tu, td = tabs or _tabs(nup, ndn, dev)
    x, lp, cnt = native.mcmc_continue(tu, td, nup, ndn, T(x0, dev), steps, 0.1, seed,
                                      walker_state=None if ws is None else T(ws, dev, torch.int32))
    return N(x), N(lp), N(cnt)


def test_logprob_probes_vs_reference(dev, g8):
    """log p at the origin / axis / ring probes through every entry that evaluates it: ff_logprob, ff_slater_logabsdet_fwd (one
    species), the samplers' own evaluation (logp_out of a chain of 0 steps: noise-fed and Philox-fed kernels) and ff_logprob3d /
    the 3-D sampler.  -inf exactly at a zero column, the tail to 1e-12."""
    from fermiflow_amd import native
    for nup, ndn in EDGE_SHAPES:
        x, ref = g8[f"p{nup}_{ndn}_x"], g8[f"p{nup}_{ndn}_logp"]
        tu, td = _tabs(nup, ndn, dev)
        assert_edge_logp(N(native.logprob(tu, td, nup, ndn, T(x, dev))), ref)
        if ndn == 0:
            assert_edge_logp(2 * N(native.slater_fwd(tu, T(x, dev))), ref)
        empty = np.zeros((0,) + x.shape), np.zeros((0, len(x)))
        assert_edge_logp(_noise(nup, ndn, x, *empty, dev)[1], ref)
        assert_edge_logp(_philox(nup, ndn, x, 0, 1, dev)[1], ref)
    for nup, ndn in EDGE_SHAPES3D:
        x, ref = g8[f"p3d{nup}_{ndn}_x"], g8[f"p3d{nup}_{ndn}_logp"]
        tu, td = _tabs(nup, ndn, dev)
        assert_edge_logp(N(native.logprob3d(tu, td, nup, ndn, T(x, dev))), ref)
        assert_edge_logp(_noise(nup, ndn, x, np.zeros((0,) + x.shape), np.zeros((0, len(x))), dev)[1], ref)


@pytest.mark.parametrize("name", EDGE_CHAINS + ["c3d4_3"])
def test_chains_vs_reference(dev, g8, name):
    """The reference's chains from origin, axis, ring (r = 16, 22, 30), NaN and ordinary starts, fed its crafted noise through
    FreeFermion.sample_with_noise: accept masks and walkers bit for bit, log p to 1e-12; the NaN walker never moves."""
    import fermiflow_amd as ff
    nup, ndn, g0, g, u, accept, x_ref, lp_ref, lp0_ref = edge_chain(g8, name)
    if g0.shape[-1] == 2:
        h = ff.HO2D()
        x, lp, acc = (N(t) for t in ff.FreeFermion(device=dev).sample_with_noise(h.orbitals[:nup], h.orbitals[:ndn], T(g0, dev),
                                                                                  T(g, dev), T(u, dev)))
    else:
        x, lp, acc = _noise(nup, ndn, g0, g, u, dev)
    assert (acc == accept).all()
    assert bits_equal(x, x_ref)
    assert_edge_logp(lp, lp_ref)
    assert np.isneginf(lp0_ref[0]) and acc[0, 0] == 1
    assert not acc[:, 6].any() and np.isnan(lp[6]) and bits_equal(x[6], g0[6])


@pytest.mark.parametrize("nup,ndn", FAMILIES)
def test_coincident_particles_vs_oracle(dev, nup, ndn):
    """Identical rows: log p = -inf (ff_logprob, and the chain's own log p), pairs and triples kept together by the noise never
    accept, separated ones accept step 1; the whole chain equals the oracle's bit for bit (log p to 1e-12)."""
    from fermiflow_amd import native
    g0, g, u, kept, sep = coincident_chains(nup, ndn, 40, 8, seed=nup + 10 * ndn)
    tu, td = _tabs(nup, ndn, dev)
    assert np.isneginf(N(native.logprob(tu, td, nup, ndn, T(g0[:5], dev)))).all()
    x, lp, acc = _noise(nup, ndn, g0, g, u, dev)
    xo, lpo, acco = O.mcmc_noise(g0, g, u, nup, ndn)
    assert (acc == acco).all() and bits_equal(x, xo)
    assert np.allclose(lp, lpo, rtol=1e-12, atol=0, equal_nan=True)
    assert not acc[:, kept].any() and np.isneginf(lp[kept]).all() and acc[0, sep].all()


@pytest.mark.parametrize("nup,ndn", FAMILIES)
def test_philox_equals_noise_path_from_special_starts(dev, nup, ndn):
    """ff_mcmc_continue (the Philox-fed kernels, accept test on the polynomial determinants) from origin, axis, ring, NaN and
    coincident-pair starts equals the noise-fed kernel on the materialised stream: walkers and log p bit for bit, accept counts;
    and the noise-fed chain equals the oracle's."""
    from fermiflow_amd import native
    B, steps, seed = 67, 12, 77
    x0, _ = special_starts(nup, ndn, B, list(range(16)), seed=nup + ndn)
    _, g, u = native.rng_fill(B, nup + ndn, steps, seed, dev)
    g, u = N(g), N(u)
    x1, lp1, acc1 = _noise(nup, ndn, x0, g, u, dev)
    x2, lp2, cnt = _philox(nup, ndn, x0, steps, seed, dev)
    assert bits_equal(x1, x2) and bits_equal(lp1, lp2) and (acc1.sum(0) == cnt).all()
    xo, lpo, acco = O.mcmc_noise(x0, g, u, nup, ndn)
    assert (acc1 == acco).all() and bits_equal(x1, xo) and np.allclose(lp1, lpo, rtol=1e-12, atol=0, equal_nan=True)
    assert acc1[0, 0] and not acc1[:, 6].any() and np.isnan(lp1[6]) and bits_equal(x1[6], x0[6])


def test_walker_state_orbital_sets(dev):
    """Several orbital sets (BetaVMC, one spin species): higher orbitals vanish on more lines, so the origin and the axes zero
    more columns.  ff_logprob and both feeds of the pair kernel against the oracle."""
    from fermiflow_amd import native
    sets = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 5], [1, 3, 4], [3, 4, 5], [0, 4, 9]], dtype=np.int32)
    B, steps = 48, 10
    x0, _ = special_starts(3, 0, B, list(range(24)), seed=3)
    ws = np.sort(np.random.default_rng(4).integers(0, len(sets), size=B)).astype(np.int32)
    tabs = (native.orbital_table(sets.tolist(), dev), None)
    lp = N(native.logprob(tabs[0], None, 3, 0, T(x0, dev), walker_state=T(ws, dev, torch.int32)))
    lpo = O.logprob(x0, 3, 0, tab_up=sets, wstate=ws, derivs=False)
    assert (np.isneginf(lp) == np.isneginf(lpo)).all() and np.isneginf(lp[:3]).all()
    assert np.allclose(lp, lpo, rtol=1e-12, atol=0, equal_nan=True)
    _, g, u = native.rng_fill(B, 3, steps, 5, dev)
    g, u = N(g), N(u)
    x1, lp1, acc1 = _noise(3, 0, x0, g, u, dev, ws=ws, tabs=tabs)
    xo, lpo, acco = O.mcmc_noise(x0, g, u, 3, 0, tab_up=sets, wstate=ws)
    assert (acc1 == acco).all() and bits_equal(x1, xo) and np.allclose(lp1, lpo, rtol=1e-12, atol=0, equal_nan=True)
    x2, lp2, cnt = _philox(3, 0, x0, steps, 5, dev, ws=ws, tabs=tabs)
    assert bits_equal(x1, x2) and bits_equal(lp1, lp2) and (acc1.sum(0) == cnt).all()


@pytest.mark.parametrize("nup,ndn", [(3, 3), (6, 0), (10, 0), (4, 3)])
def test_special_walkers_at_large_ragged_batch(dev, nup, ndn):
    """B = 131 075 (ragged last workgroup), special walkers at both lanes of a walker and the edges of the workgroups
    (0, 63, 64, 127, 128, B - 2, B - 1), at the edges of the sixteen-lane groups (two walkers per wave: 1, 2, 3, 31, 32) and at a
    seeded sample: every other walker is bit-identical to the same launch with ordinary walkers in their place -- noise-fed and
    Philox-fed -- and the special walkers equal the oracle."""
    B, steps = 131075, 4
    rng = np.random.default_rng(nup * 10 + ndn)
    pos = sorted(set([0, 1, 2, 3, 31, 32, 63, 64, 127, 128, B - 2, B - 1] + rng.choice(B, 20, replace=False).tolist()))
    x0, plain = special_starts(nup, ndn, B, pos, seed=7)
    g = rng.standard_normal((steps, B, nup + ndn, 2)); u = rng.random((steps, B))
    keep = np.ones(B, bool); keep[pos] = False
    xa, lpa, aa = _noise(nup, ndn, x0, g, u, dev)
    xb, lpb, ab = _noise(nup, ndn, plain, g, u, dev)
    assert bits_equal(xa[keep], xb[keep]) and bits_equal(lpa[keep], lpb[keep]) and (aa[:, keep] == ab[:, keep]).all()
    xo, lpo, acco = O.mcmc_noise(x0[pos], g[:, pos], u[:, pos], nup, ndn)
    assert (aa[:, pos] == acco).all() and bits_equal(xa[pos], xo) and np.allclose(lpa[pos], lpo, rtol=1e-12, atol=0, equal_nan=True)
    xa, lpa, ca = _philox(nup, ndn, x0, steps, 31, dev)
    xb, lpb, cb = _philox(nup, ndn, plain, steps, 31, dev)
    assert bits_equal(xa[keep], xb[keep]) and bits_equal(lpa[keep], lpb[keep]) and (ca[keep] == cb[keep]).all()
