"""Density maps on the MI355X: the device histograms against numpy on the same walkers, against the exact law of Gaussian walkers,
inside GSVMC / BetaVMC sweeps (which they must not change by a bit), on the frames of CNF.generate, through the drivers' --maps_out /
--frames_maps_out and summed over two ranks."""
import math

import numpy as np
import pytest
import torch

import fermiflow_amd as ff
from fermiflow_amd import DensityMaps
from tests import maps_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def raw(maps):
    torch.cuda.synchronize()
    return maps._buf.cpu().numpy().copy()


def planes(maps, frame=0):
    c = maps.counts(frame)
    return np.stack([np.concatenate([c[k].reshape(-1), c["lost_" + k]]) for k in R.PLANES]), c


def assert_counts(maps, ref, n_edge, calls, walkers, frame=0):
    """device counts == numpy's, up to 2 slots per sample within 1e-9 of a cell edge (device code contracts a * b + c into FMAs)"""
    got, c = planes(maps, frame)
    dev_total = int(np.abs(got - ref).sum())
    print("deviation", dev_total, "edge samples", n_edge)
    assert dev_total <= 2 * n_edge
    assert np.array_equal(got.sum(1), ref.sum(1))
    assert (c["calls"], c["walkers"]) == (calls, walkers)


def test_device_counts_equal_numpy(dev):
    """config 2 of the benchmark (3 + 3 particles, 65 536 walkers) at the default geometry: 128 bins, two bands per plane"""
    nup, ndn, B, extent, nbins = 3, 3, 65536, 6.0, 128
    x = np.random.default_rng(11).standard_normal((B, nup + ndn, 2)) * 1.3
    n_edge = R.edge_samples(x, nup, extent, nbins)
    assert n_edge == 0          # a property of the seeded input, from numpy alone: the comparison below is exact equality
    ref = R.histogram(x, nup, extent, nbins)
    assert np.array_equal(ref.sum(1), B * R.samples_per_walker(nup, ndn))
    xd = torch.from_numpy(x).to(dev)
    a, b = DensityMaps(nup, ndn, extent=extent, nbins=nbins), DensityMaps(nup, ndn, extent=extent, nbins=nbins)
    a.accumulate(xd)
    b.accumulate(xd)
    assert_counts(a, ref, n_edge, 1, B)
    assert np.array_equal(raw(a), raw(b))                           # the same call on a second object: the raw buffers bit for bit
    a.accumulate(xd)
    assert_counts(a, 2 * ref, n_edge, 2, 2 * B)
    with pytest.raises(ValueError):
        a.accumulate(xd[:100])                                      # equal calls only
    with pytest.raises(ValueError, match="two-dimensional"):
        a.accumulate(torch.zeros(8, 6, 3, dtype=torch.float64, device=dev))


@pytest.mark.parametrize("B,seed", [((1 << 20) + 77, 21), ((1 << 22) + 65, 22)], ids=["looping", "two_launches"])
def test_large_batches(dev, B, seed):
    """1 + 1 particles, 16 bins: four planes of one band.  2^20 + 77 walkers are 4097 tiles of 256 for 256 slices (1024 workgroups over
    four planes): every workgroup takes 16 tiles, one of them a 17th, the last tile ragged.  2^22 + 65 walkers are more than one launch
    takes (no uint32 LDS counter may wrap) and still ONE call: calls == 1, walkers == B."""
    nbins, extent = 16, 6.0
    x = np.random.default_rng(seed).standard_normal((B, 2, 2)) * 1.3
    n_edge = R.edge_samples(x, 1, extent, nbins)
    assert n_edge == 0
    ref = R.histogram(x, 1, extent, nbins)
    maps = DensityMaps(1, 1, extent=extent, nbins=nbins)
    maps.accumulate(torch.from_numpy(x).to(dev))
    assert_counts(maps, ref, n_edge, 1, B)


def _cell_probabilities(extent, nbins):
    """P(cell) for a point ~ N(0, I / 2): products of erf differences"""
    edges = np.linspace(-extent, extent, nbins + 1)
    cdf = np.array([0.5 * (1.0 + math.erf(t)) for t in edges])
    p1 = np.diff(cdf)
    return np.outer(p1, p1)


def _max_z(counts, N, p):
    sel = N * p >= 50.0
    assert sel.sum() >= 200
    z = (counts[sel] - N * p[sel]) / np.sqrt(N * p[sel] * (1.0 - p[sel]))
    return float(np.abs(z).max())


def test_gaussian_walkers_follow_the_exact_law(dev):
    """Walkers drawn by torch.randn / sqrt(2) on the CPU (nothing of the sampler), 1 + 1 particles.  An isotropic Gaussian is unchanged
    by a rotation independent of it, so up, down, ud and du all follow the same cell probabilities, products of erf differences.  Every
    cell expecting >= 50 samples within 5 standard deviations, sigma^2 = N p (1 - p) -- first for numpy's counts of the same walkers
    (the criterion is a property of the input), then for the device's."""
    N, extent, nbins = 1 << 18, 3.0, 32
    x = torch.randn(N, 2, 2, generator=torch.Generator().manual_seed(1211), dtype=torch.float64) / math.sqrt(2.0)
    ref = R.histogram(x.numpy(), 1, extent, nbins)
    maps = DensityMaps(1, 1, extent=extent, nbins=nbins)
    maps.accumulate(x.to(dev))
    c = maps.counts()
    p = _cell_probabilities(extent, nbins)
    for k, name in enumerate(R.PLANES):
        if name in ("uu", "dd"):
            assert not c[name].any() and c["lost_" + name] == (0, 0)
            continue
        z_ref = _max_z(ref[k, :nbins * nbins].reshape(nbins, nbins), N, p)
        z_dev = _max_z(c[name], N, p)
        print(name, "max |z| numpy", z_ref, "device", z_dev)
        assert z_ref <= 5.0
        assert z_dev <= 5.0
    # and the normalised density is the law itself at the cell centres of the bulk (within 10 %: about 2000 samples per cell there)
    xm, ym = maps.xy_mid()
    law = np.exp(-(xm[:, None] ** 2 + ym[None, :] ** 2)) / math.pi
    bulk = (xm[:, None] ** 2 + ym[None, :] ** 2) < 0.5
    assert np.abs(maps.density()["up"][bulk] / law[bulk] - 1.0).max() < 0.1
    assert np.abs(maps.pair_density()["ud"][bulk] / law[bulk] - 1.0).max() < 0.1


def test_sign_convention_known_answer(dev):
    """the 60-degree pair of tests/test_maps_hostsim.py::test_sign_convention_known_answer, on the device"""
    B, L, nbins = 4096, 4.0, 64
    phi = np.random.default_rng(61).uniform(0.0, 2.0 * np.pi, B)
    x = np.empty((B, 2, 2))
    x[:, 0, 0], x[:, 0, 1] = 1.1 * np.cos(phi), 1.1 * np.sin(phi)
    x[:, 1, 0], x[:, 1, 1] = 1.7 * np.cos(phi + np.pi / 3.0), 1.7 * np.sin(phi + np.pi / 3.0)
    maps = DensityMaps(1, 1, extent=L, nbins=nbins)
    maps.accumulate(torch.from_numpy(x).to(dev))
    c = maps.counts()
    assert c["ud"][38, 43] == B and c["ud"].sum() == B
    assert c["du"][36, 24] == B and c["du"].sum() == B
    assert c["up"].sum() == B and c["down"].sum() == B and not c["uu"].any() and not c["dd"].any()


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


def _run(model, iters, B, maps):
    model.density_maps = maps
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
    B, extent, nbins = 4096, 6.0, 128
    make = _gs_model if kind == "gs" else _beta_model
    maps = DensityMaps(nup, ndn, extent=extent, nbins=nbins)
    assert make(dev).density_maps is None
    with_maps = _run(make(dev), iters, B, maps)
    without = _run(make(dev), iters, B, None)
    for a, b in zip(with_maps, without):
        # the maps are one more launch on the stream: not a bit of the sweep changes
        assert np.float64(a["E"]).tobytes() == np.float64(b["E"]).tobytes()
        assert np.float64(a["E_std"]).tobytes() == np.float64(b["E_std"]).tobytes()
        assert len(a["grads"]) == len(b["grads"]) and all(u.tobytes() == v.tobytes() for u, v in zip(a["grads"], b["grads"]))
        assert a["x"].tobytes() == b["x"].tobytes()
    ref = sum(R.histogram(a["x"], nup, extent, nbins) for a in with_maps)
    n_edge = sum(R.edge_samples(a["x"], nup, extent, nbins) for a in with_maps)
    assert_counts(maps, ref, n_edge, iters, iters * B)


def test_frames(dev):
    """accumulate_frames on the trajectory of CNF.generate: frame k's maps are numpy's on frames[k]; frame 0 is the base walkers"""
    K, B, extent, nbins = 5, 1024, 6.0, 64
    cnf = _gs_model(dev).cnf
    z = (torch.randn(B, 6, 2, generator=torch.Generator().manual_seed(17), dtype=torch.float64) * 1.2).to(dev)
    frames = cnf.generate(z, nframes=K)
    assert tuple(frames.shape) == (K, B, 6, 2)
    maps = DensityMaps(3, 3, extent=extent, nbins=nbins, nframes=K)
    maps.accumulate_frames(frames)
    host = frames.cpu().numpy()
    for k in range(K):
        assert_counts(maps, R.histogram(host[k], 3, extent, nbins), R.edge_samples(host[k], 3, extent, nbins), 1, B, frame=k)
    assert not np.array_equal(planes(maps, K - 1)[0], planes(maps, 0)[0])          # (the flow moves the walkers)
    base = DensityMaps(3, 3, extent=extent, nbins=nbins)
    base.accumulate(z)
    assert np.array_equal(raw(base)[0], raw(maps)[0])
    with pytest.raises(ValueError):
        maps.accumulate_frames(frames[:4])


def _check_file(f, nup, ndn, frames, walkers, nbins):
    per = R.samples_per_walker(nup, ndn)
    area = float(f["cell_area"])
    assert f["x_mid"].shape == (nbins,) and list(f["walkers"]) == [walkers] * frames
    for k, name in enumerate(R.PLANES):
        val = f[("rho_" if k < 2 else "g_") + name]
        cnt, lost = f["counts_" + name], f["lost_" + name]
        assert val.shape == (frames, nbins, nbins) and lost.shape == (frames, 2)
        for fr in range(frames):
            share = lost[fr].sum() / float(walkers)          # the reported overflow (and invalid) share per walker
            assert abs((val[fr] * area).sum() - (per[k] - share)) < 1e-12 * max(per[k], 1)
            assert cnt[fr].sum() + lost[fr].sum() == per[k] * walkers


def test_driver_writes_the_maps(dev, tmp_path):
    from fermiflow_amd import FermionHO2D
    out, fout = str(tmp_path / "maps.npz"), str(tmp_path / "fmaps.npz")
    torch.manual_seed(3)
    FermionHO2D.main(["--nup", "3", "--ndown", "3", "--Z", "2.0", "--batch", "2048", "--iternum", "2", "--maps_out", out,
                      "--maps_extent", "5.0", "--maps_bins", "48", "--frames_maps_out", fout, "--nframes", "3", "--frames_batch", "512"])
    f = np.load(out)
    assert list(f["calls"]) == [2] and int(f["nbins"]) == 48 and float(f["extent"]) == 5.0
    _check_file(f, 3, 3, 1, 2 * 2048, 48)
    g = np.load(fout)          # the K maps of the trajectory's walkers, with no --frames_out: no trajectory went to the host
    assert list(g["calls"]) == [1, 1, 1] and int(g["nframes"]) == 3
    _check_file(g, 3, 3, 3, 512, 48)


def test_a_resumed_driver_continues_its_counts(dev, tmp_path):
    from fermiflow_amd import BetaFermionHO2D
    ck, first, second = str(tmp_path / "ck.pt"), str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    common = ["--beta", "10.0", "--nup", "3", "--boltzmann", "--batch", "2048", "--maps_extent", "5.0", "--maps_bins", "48"]
    torch.manual_seed(3)
    BetaFermionHO2D.main(common + ["--iternum", "2", "--save", ck, "--maps_out", first])
    BetaFermionHO2D.main(common + ["--iternum", "1", "--resume", ck, "--maps_out", second])
    a, b = np.load(first), np.load(second)
    assert list(a["calls"]) == [2] and list(b["calls"]) == [3] and list(b["walkers"]) == [3 * 2048]
    _check_file(b, 3, 0, 1, 3 * 2048, 48)
    for name in R.PLANES:
        later = (b["counts_" + name] - a["counts_" + name]).sum() + (b["lost_" + name] - a["lost_" + name]).sum()
        assert (b["counts_" + name] >= a["counts_" + name]).all()
        assert later == (a["counts_" + name].sum() + a["lost_" + name].sum()) // 2          # the third iteration's own samples


# ------------------------------------------------------------------------------------------------------------ data parallelism
def _dp_walkers(B):
    return torch.randn(B, 5, 2, generator=torch.Generator().manual_seed(31), dtype=torch.float64) * 1.3


def _dp_run(rank, world, port, B, out):
    """this rank's shard of B given walkers into its own maps, then the sum over the ranks"""
    import os
    import torch.distributed as dist
    from fermiflow_amd import dist as D
    dev = torch.device("cuda:0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    off, cnt = D.shard(B)
    maps = DensityMaps(3, 2, extent=5.0, nbins=40, nframes=2)
    x = _dp_walkers(B)[off:off + cnt].to(dev)
    maps.accumulate(x, frame=0)
    maps.accumulate(-x, frame=1)
    maps.all_reduce_()
    out[rank] = (maps.state_dict()["acc"].numpy().copy(), off, cnt)
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_single_process_counts(dev):
    """1025 walkers on two ranks sharing the GPU (gloo; shards of 513 and 512): all_reduce_() leaves the single process's counts on
    both ranks exactly; calls counts one call per rank."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dist import _free_port
    B = 1025
    one = DensityMaps(3, 2, extent=5.0, nbins=40, nframes=2)
    x = _dp_walkers(B).to(dev)
    one.accumulate(x, frame=0)
    one.accumulate(-x, frame=1)
    want = one.state_dict()["acc"].numpy()
    two = mp.get_context("spawn").Manager().dict()
    mp.spawn(_dp_run, args=(2, _free_port(), B, two), nprocs=2, join=True)
    assert [two[r][2] for r in (0, 1)] == [513, 512]
    for r in (0, 1):
        got = two[r][0]
        assert np.array_equal(got[:, 1:], want[:, 1:])          # walkers and every slot of every plane and frame
        assert list(got[:, 0]) == [2, 2] and list(want[:, 0]) == [1, 1]
