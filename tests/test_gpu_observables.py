"""Observables on the MI355X: the device histograms against numpy on the same walkers, against the exact laws of Gaussian
walkers, inside GSVMC / BetaVMC sweeps (which they must not change by a bit) and through the driver's --observe_out."""
import math

import numpy as np
import pytest
import torch

import fermiflow_amd as ff
from fermiflow_amd import Observables
from tests import observe_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def raw(obs):
    torch.cuda.synchronize()
    return obs._buf.cpu().numpy().copy()


def assert_counts(obs, ref, n_edge, calls, walkers):
    """device counts == numpy's, up to 2 slots per sample within 1e-9 of a bin edge (device code contracts a * b + c into FMAs)"""
    c = obs.counts()
    got = np.stack([c[k] for k in R.CLASSES])
    dev_total = int(np.abs(got - ref).sum())
    print("deviation", dev_total, "edge samples", n_edge)
    assert dev_total <= 2 * n_edge
    assert np.array_equal(got.sum(1), ref.sum(1))
    assert (c["calls"], c["walkers"]) == (calls, walkers)


# config 2 of the benchmark (3 + 3 particles in 2-D, 65 536 walkers) and configs[4] (10 + 10 in 3-D, 16 384 walkers per GPU)
@pytest.mark.parametrize("nup,ndn,d,B,seed", [(3, 3, 2, 65536, 11), (10, 10, 3, 16384, 12)], ids=["config2", "configs4"])
def test_device_counts_equal_numpy(dev, nup, ndn, d, B, seed):
    rmax, nbins = 6.0, 240
    x = np.random.default_rng(seed).standard_normal((B, nup + ndn, d)) * 1.3
    n_edge = R.edge_samples(x, nup, rmax, nbins)
    assert n_edge == 0          # a property of the seeded input, from numpy alone: the comparison below is exact equality
    ref = R.histogram(x, nup, rmax, nbins)
    xd = torch.from_numpy(x).to(dev)
    a, b = Observables(nup, ndn, dim=d, rmax=rmax, nbins=nbins), Observables(nup, ndn, dim=d, rmax=rmax, nbins=nbins)
    a.accumulate(xd)
    b.accumulate(xd)
    assert_counts(a, ref, n_edge, 1, B)
    ra, rb = raw(a), raw(b)
    assert np.array_equal(ra, rb)                                   # the same call twice: the raw buffers bit for bit
    S = 5 * (nbins + 2)
    assert not ra[2 + 2 * S:].any()                                 # scratch and ticket are zero again
    assert np.array_equal(ra[2 + S:2 + 2 * S].reshape(5, -1), ref ** 2)
    a.accumulate(xd)
    assert_counts(a, 2 * ref, n_edge, 2, 2 * B)
    with pytest.raises(ValueError):
        a.accumulate(xd[:100])                                      # equal blocks only


def test_a_call_of_more_walkers_than_one_launch_takes_is_one_block(dev):
    """Above 2^22 walkers a call is several launches (no uint32 slot of the LDS histograms may wrap); only the last one folds: calls
    is 1, walkers is B and sumsq is the square of the WHOLE call's counts, not the sum of the launches' squares."""
    nbins, rmax, B = 16, 6.0, (1 << 22) + 65
    x = np.random.default_rng(77).standard_normal((B, 1, 2)) * 1.3
    n_edge = R.edge_samples(x, 1, rmax, nbins)
    assert n_edge == 0
    ref = R.histogram(x, 1, rmax, nbins)
    obs = Observables(1, 0, rmax=rmax, nbins=nbins)
    obs.accumulate(torch.from_numpy(x).to(dev))
    assert_counts(obs, ref, n_edge, 1, B)
    ra = raw(obs)
    S = 5 * (nbins + 2)
    assert np.array_equal(ra[2 + S:2 + 2 * S].reshape(5, -1), ref ** 2)
    assert not ra[2 + 2 * S:].any()


def test_an_empty_call_fixes_no_block_size(dev):
    obs = Observables(2, 1, nbins=8)
    obs.accumulate(torch.zeros(0, 3, 2, dtype=torch.float64, device=dev))
    assert obs.counts()["calls"] == 0
    x = torch.randn(100, 3, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(dev)
    obs.accumulate(x)                                               # the first call that counts sets the block size
    with pytest.raises(ValueError):
        obs.accumulate(x[:50])
    c = obs.counts()
    assert (c["calls"], c["walkers"]) == (1, 100)


def _cdf_radius(a, sigma2, d):
    """P(|g| < a) for g ~ N(0, sigma2 I_d)"""
    if d == 2:
        return 1.0 - np.exp(-a * a / (2.0 * sigma2))
    s = math.sqrt(sigma2)
    return np.array([math.erf(t / (s * math.sqrt(2.0))) for t in a]) - math.sqrt(2.0 / math.pi) * (a / s) * np.exp(-a * a / (2.0 * sigma2))


def _within_5_sigma(counts, N, sigma2, d, rmax, nbins):
    edges = np.arange(nbins + 1) * (rmax / nbins)
    p = np.diff(_cdf_radius(edges, sigma2, d))
    sel = N * p >= 50.0
    assert sel.sum() >= 20
    z = (counts[:nbins][sel] - N * p[sel]) / np.sqrt(N * p[sel] * (1.0 - p[sel]))
    return float(np.abs(z).max())


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [1, 2])
def test_gaussian_walkers_follow_the_exact_laws(dev, n, d):
    """Walkers drawn by torch.randn / sqrt(2) on the CPU (nothing of the sampler): the radial law is e^{-r^2} / pi^{d/2}, the pair distance
    that of a unit-variance Gaussian difference.  Expected counts per bin from the exact bin integrals; every bin expecting >= 50 samples
    within 5 standard deviations, sigma^2 = N p (1 - p) -- first for numpy's histogram of the same walkers (the criterion is a property of
    the input), then for the device's."""
    N, rmax, nbins = 1 << 18, 5.0, 100
    x = torch.randn(N, n, d, generator=torch.Generator().manual_seed(1000 + 10 * n + d), dtype=torch.float64) / math.sqrt(2.0)
    nup, ndn = (1, 0) if n == 1 else (1, 1)
    ref = R.histogram(x.numpy(), nup, rmax, nbins)
    obs = Observables(nup, ndn, dim=d, rmax=rmax, nbins=nbins)
    obs.accumulate(x.to(dev))
    c = obs.counts()
    laws = [("up", 0, 0.5)] + ([("down", 1, 0.5), ("ud", 3, 1.0)] if n == 2 else [])
    for name, k, sigma2 in laws:
        z_ref = _within_5_sigma(ref[k], N, sigma2, d, rmax, nbins)
        z_dev = _within_5_sigma(c[name], N, sigma2, d, rmax, nbins)
        print(name, "max |z| numpy", z_ref, "device", z_dev)
        assert z_ref <= 5.0
        assert z_dev <= 5.0
    # and the normalised density is the law itself at the bin centres of the bulk (within 10 %: about 1e4 samples per bin there)
    r, n_up, _, _, _ = obs.radial_density()
    bulk = (r > 0.5) & (r < 1.2)
    law = np.exp(-r * r) / math.pi ** (d / 2.0)
    assert np.abs(n_up[bulk] / law[bulk] - 1.0).max() < 0.1


def _gs_model(dev):
    from __graft_entry__ import _model
    return _model(dev)


def _beta_model(dev):
    eta, mu = ff.MLP(1, 50), ff.MLP(1, 50)
    eta.init_gaussian(3); mu.init_gaussian(4)
    with torch.no_grad():
        for m in (eta, mu):
            m.fc2.weight *= 30.0
            m.fc1.weight *= 300.0
    cnf = ff.CNF(ff.Backflow(eta, mu=mu), (0.0, 1.0))
    model = ff.BetaVMC(10.0, 3, 0, 2.0, True, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    model.to(device=dev)
    return model


def _run(model, iters, B, obs):
    model.observables = obs
    torch.manual_seed(7)
    out = []
    for _ in range(iters):
        res = model(B)
        for p in model.parameters():
            p.grad = None
        for g in (res if isinstance(res, tuple) else (res,)):
            g.backward()
        torch.cuda.synchronize()
        out.append(dict(E=model.E, E_std=model.E_std, x=model.x.cpu().numpy().copy(),
                        grads=[p.grad.detach().cpu().numpy().copy() for p in model.parameters()]))
    return out


@pytest.mark.parametrize("kind,iters,nup,ndn", [("gs", 3, 3, 3), ("beta", 2, 3, 0)])
def test_inside_a_sweep(dev, kind, iters, nup, ndn):
    B, rmax, nbins = 4096, 6.0, 240
    make = _gs_model if kind == "gs" else _beta_model
    obs = Observables(nup, ndn, rmax=rmax, nbins=nbins)
    assert make(dev).observables is None
    with_obs = _run(make(dev), iters, B, obs)
    without = _run(make(dev), iters, B, None)
    for a, b in zip(with_obs, without):
        # the observable is one more launch on the stream: not a bit of the sweep changes
        assert np.float64(a["E"]).tobytes() == np.float64(b["E"]).tobytes()
        assert np.float64(a["E_std"]).tobytes() == np.float64(b["E_std"]).tobytes()
        assert len(a["grads"]) == len(b["grads"]) and all(u.tobytes() == v.tobytes() for u, v in zip(a["grads"], b["grads"]))
        assert a["x"].tobytes() == b["x"].tobytes()
    ref = sum(R.histogram(a["x"], nup, rmax, nbins) for a in with_obs)
    n_edge = sum(R.edge_samples(a["x"], nup, rmax, nbins) for a in with_obs)
    assert_counts(obs, ref, n_edge, iters, iters * B)
    r, n_up, n_dn, e_up, e_dn = obs.radial_density()
    assert np.isfinite(e_up).all() and (e_up[n_up > 0] > 0).any()


def test_driver_writes_the_observables(dev, tmp_path):
    from fermiflow_amd import FermionHO2D
    out = str(tmp_path / "obs.npz")
    torch.manual_seed(3)
    FermionHO2D.main(["--nup", "3", "--ndown", "3", "--Z", "2.0", "--batch", "2048", "--iternum", "2", "--observe_out", out,
                      "--observe_rmax", "4.0", "--observe_bins", "80"])
    f = np.load(out)
    assert int(f["calls"]) == 2 and int(f["walkers"]) == 2 * 2048 and f["r_mid"].shape == (80,)
    V = f["shell_volumes"]
    for dens, cnt, number in ((f["n_up"], f["counts_up"], 3), (f["n_dn"], f["counts_down"], 3), (f["g_uu"], f["counts_uu"], 3),
                              (f["g_ud"], f["counts_ud"], 9), (f["g_dd"], f["counts_dd"], 3)):
        lost = cnt[80:].sum() / float(f["walkers"])          # the reported overflow (and invalid) share per walker
        assert abs((dens * V).sum() - (number - lost)) < 1e-12 * number
        assert cnt.sum() == number * int(f["walkers"])
    assert np.isfinite(f["err_up"]).all()


def test_a_resumed_driver_continues_its_averages(dev, tmp_path):
    from fermiflow_amd import FermionHO2D
    ck, first, second = str(tmp_path / "ck.pt"), str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    common = ["--nup", "3", "--ndown", "3", "--Z", "2.0", "--batch", "2048", "--observe_rmax", "4.0", "--observe_bins", "80"]
    torch.manual_seed(3)
    FermionHO2D.main(common + ["--iternum", "2", "--save", ck, "--observe_out", first])
    FermionHO2D.main(common + ["--iternum", "1", "--resume", ck, "--observe_out", second])
    a, b = np.load(first), np.load(second)
    assert int(a["calls"]) == 2 and int(b["calls"]) == 3 and int(b["walkers"]) == 3 * 2048
    for name in R.CLASSES:
        later = b["counts_" + name] - a["counts_" + name]          # the third iteration's own counts
        assert (later >= 0).all() and later.sum() == a["counts_" + name].sum() // 2
