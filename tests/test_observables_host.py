"""fermiflow_amd.observables on the host: normalisation, block errors, state_dict and the rank sum, on counts loaded through
load_state_dict -- no kernel runs here."""
import numpy as np
import pytest
import torch

from fermiflow_amd import Observables
from tests import observe_ref as R


def load(obs, blocks, B):
    """counts of `blocks` (a list of (5, nbins + 2) per-call histograms of B walkers each) into obs"""
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    acc = np.concatenate([[len(blocks), B * len(blocks)], sum(blocks).reshape(-1), sum(b ** 2 for b in blocks).reshape(-1)])
    st = obs.state_dict()
    st["acc"] = torch.from_numpy(acc.astype(np.int64))
    obs.load_state_dict(st)


@pytest.mark.parametrize("dim", [2, 3])
def test_normalisation_integrals_are_particle_and_pair_numbers(dim):
    nup, ndn, nbins, rmax, B = 4, 3, 60, 5.0, 500
    obs = Observables(nup, ndn, dim=dim, rmax=rmax, nbins=nbins)
    blocks = [R.histogram(np.random.default_rng(s).standard_normal((B, nup + ndn, dim)) * 1.2, nup, rmax, nbins) for s in range(4)]
    load(obs, blocks, B)
    c = obs.counts()
    assert (c["calls"], c["walkers"]) == (4, 4 * B)
    V = obs.shell_volumes()
    edges = np.arange(nbins + 1) * (rmax / nbins)
    assert np.allclose(V, np.pi * np.diff(edges ** 2) if dim == 2 else 4.0 * np.pi / 3.0 * np.diff(edges ** 3), rtol=1e-13)
    r, n_up, n_dn, _, _ = obs.radial_density()
    assert np.allclose(r, 0.5 * (edges[1:] + edges[:-1]))
    _, uu, ud, dd, _, _, _ = obs.pair_distribution()
    per = R.pair_counts(nup, ndn)
    for k, (name, val) in enumerate(zip(R.CLASSES, (n_up, n_dn, uu, ud, dd))):
        lost = c[name][nbins:].sum() / c["walkers"]          # the class's overflow and invalid share, per walker
        assert abs((val * V).sum() - (per[k] - lost)) < 1e-12 * per[k]


def test_error_is_the_block_standard_error():
    nup, ndn, nbins, rmax, B = 2, 2, 20, 4.0, 300
    obs = Observables(nup, ndn, rmax=rmax, nbins=nbins)
    blocks = [R.histogram(np.random.default_rng(10 + s).standard_normal((B, 4, 2)), nup, rmax, nbins) for s in range(7)]
    load(obs, blocks, B)
    V = obs.shell_volumes()
    per_block = np.stack(blocks)[:, :, :nbins] / (B * V)                 # the estimate of every block
    want = per_block.std(axis=0, ddof=1) / np.sqrt(len(blocks))
    _, n_up, n_dn, e_up, e_dn = obs.radial_density()
    _, uu, ud, dd, e_uu, e_ud, e_dd = obs.pair_distribution()
    got = np.stack([e_up, e_dn, e_uu, e_ud, e_dd])
    assert np.allclose(got, want, rtol=1e-9, atol=1e-15)
    assert np.allclose(np.stack([n_up, n_dn, uu, ud, dd]), per_block.mean(axis=0), rtol=1e-13)


def test_error_is_nan_for_one_call():
    obs = Observables(1, 1, rmax=3.0, nbins=10)
    load(obs, [R.histogram(np.random.default_rng(0).standard_normal((50, 2, 2)), 1, 3.0, 10)], 50)
    r, n_up, n_dn, e_up, e_dn = obs.radial_density()
    assert np.isfinite(n_up).all() and np.isnan(e_up).all() and np.isnan(e_dn).all()
    assert all(np.isnan(e).all() for e in obs.pair_distribution()[4:])


def test_state_dict_round_trip_and_geometry_check():
    obs = Observables(3, 3, rmax=6.0, nbins=24)
    load(obs, [R.histogram(np.random.default_rng(s).standard_normal((40, 6, 2)), 3, 6.0, 24) for s in range(3)], 40)
    st = obs.state_dict()
    other = Observables(3, 3, rmax=6.0, nbins=24)
    other.load_state_dict(st)
    a, b = obs.counts(), other.counts()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(obs.pair_distribution(), other.pair_distribution()))
    assert torch.equal(other.state_dict()["acc"], st["acc"])
    with pytest.raises(ValueError):
        Observables(3, 3, rmax=6.0, nbins=25).load_state_dict(st)
    other.reset()
    assert other.counts()["calls"] == 0 and not other.counts()["uu"].any()


def test_checkpoint_carries_the_counts(tmp_path):
    from fermiflow_amd import checkpoint
    model = torch.nn.Linear(2, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    obs = Observables(2, 1, rmax=6.0, nbins=16)
    load(obs, [R.histogram(np.random.default_rng(s).standard_normal((30, 3, 2)), 2, 6.0, 16) for s in range(3)], 30)
    path = str(tmp_path / "ck.pt")
    checkpoint.save(path, model, opt, 3, observables=obs)
    other = Observables(2, 1, rmax=6.0, nbins=16)
    assert checkpoint.load(path, model, opt, observables=other) == 3
    assert torch.equal(other.state_dict()["acc"], obs.state_dict()["acc"]) and other.counts()["calls"] == 3
    assert checkpoint.load(path, model, opt) == 3                                     # nobody asks for them: ignored
    with pytest.raises(ValueError):
        checkpoint.load(path, model, opt, observables=Observables(2, 1, rmax=5.0, nbins=16))      # another geometry
    checkpoint.save(path, model, opt, 4)                                              # a checkpoint without observables
    assert checkpoint.load(path, model, opt, observables=other) == 4 and other.counts()["calls"] == 3


def test_all_reduce_in_one_process_is_the_identity():
    obs = Observables(2, 1, rmax=6.0, nbins=16)
    load(obs, [R.histogram(np.random.default_rng(s).standard_normal((30, 3, 2)), 2, 6.0, 16) for s in range(2)], 30)
    before = obs.state_dict()["acc"].clone()
    obs.all_reduce_()
    assert torch.equal(obs.state_dict()["acc"], before)
    st = obs.state_dict()
    st["acc"][5] = 2 ** 53          # a count the sum over ranks as doubles could not carry exactly
    obs.load_state_dict(st)
    with pytest.raises(OverflowError):
        obs.all_reduce_()


def test_accumulate_refuses_host_tensors_and_wrong_shapes():
    obs = Observables(3, 3)
    with pytest.raises(RuntimeError):
        obs.accumulate(torch.zeros(4, 6, 2))          # no CPU path
    with pytest.raises(ValueError):
        Observables(3, 3, nbins=0)
    with pytest.raises(ValueError):
        Observables(3, 3, rmax=float("inf"))
    with pytest.raises(NotImplementedError):
        Observables(13, 12)
