"""CNF.generate(z, nframes=K) on the MI355X (ff_cnf_generate_frames) through the package: the frames of one launch
against CNF(v, (t0, t_k)).generate(z), the project's own flow pass over the sub-interval.  Walkers, frame times and bars are those
of the host-simulator test (tests/frames_ref.py, derived in tests/test_frames_hostsim.py)."""
import numpy as np
import pytest
import torch

from tests import frames_ref as F
from tests.common import N, T, cu_count, kernel_families, looping_batch, assert_loops, make_flow, net_arrays

pytestmark = pytest.mark.gpu

SHAPES = F.GPU_SHAPES
IDS = [f"{n}x{d}_B{B}" for n, d, B in SHAPES]
radial_modes = pytest.mark.parametrize("radial", ["table", "exact"])
shapes = pytest.mark.parametrize("n,d,B", SHAPES, ids=IDS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(golden):
    return net_arrays(golden["g3_backflow"], "c1_")          # the benchmark's weights, with mu


@pytest.fixture
def flow(dev, weights, monkeypatch):
    """flow(radial, t1=..., tol=...) -> a CNF over (t0, t1) whose kernels evaluate eta and mu from the table / directly"""
    from fermiflow_amd import _lib

    def make(radial, t1=F.T1, tol=F.LOOSE):
        monkeypatch.setattr(_lib, "RADIAL_MODE", radial)
        cnf = make_flow(weights[0], weights[1], dev)
        cnf.t_span, cnf.t_span_reverse = (F.T0, t1), (t1, F.T0)
        cnf.rtol, cnf.atol = tol["rtol"], tol["atol"]
        return cnf
    return make


def bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all())


@radial_modes
@shapes
def test_frame_zero_and_two_frames(dev, flow, n, d, B, radial):
    """Cases 1 and 2: frames[0] is z; with nframes = 2 frames[1] and the stats are ff_cnf_generate's bit for bit."""
    from fermiflow_amd import native
    z = T(F.walkers(n, d, B), dev)
    cnf = flow(radial)
    fr = cnf.generate(z, nframes=2)
    assert fr.shape == (2, B, n, d) and fr.dtype == torch.float64 and fr.device == z.device and not fr.requires_grad
    assert bits(fr[0], z)
    assert bits(fr[1], cnf.generate(z))
    net = cnf.v_wrapper.v.net()
    x, st = native.cnf_generate(net, z, F.T0, F.T1, cnf.rtol, cnf.atol, want_stats=True)
    fr2, stf = native.cnf_generate_frames(net, z, 2, F.T0, F.T1, cnf.rtol, cnf.atol)
    assert bits(fr2[1], x) and torch.equal(stf[:4], st[:4]) and int(st[3]) == 0
    assert bits(cnf.generate(z, nframes=5)[0], z)
    one = cnf.generate(z, nframes=1)
    assert one.shape == (1, B, n, d) and bits(one[0], z)


def _frames_against_generate(dev, flow, n, d, B, radial, nframes, tol):
    z = T(F.walkers(n, d, B), dev)
    fr = flow(radial, tol=tol).generate(z, nframes=nframes)
    assert fr.shape == (nframes, B, n, d) and bool(torch.isfinite(fr).all())
    worst = 0.0
    for k, tk in enumerate(F.frame_times(nframes)):
        if k:
            worst = max(worst, float((fr[k] - flow(radial, t1=tk, tol=tol).generate(z)).abs().max()))
    return worst


@radial_modes
@shapes
def test_each_frame_against_generate_tight(dev, flow, n, d, B, radial):
    """Case 3: nframes = 5 at 1e-10 / 1e-12 against generate over (t0, t_k); the bar of tests/frames_ref.py (6.139e-12)."""
    worst = _frames_against_generate(dev, flow, n, d, B, radial, F.NF_TIGHT, F.TIGHT)
    print(f"FRAMES tight {n}x{d} B={B} {radial}: {worst:.3e} (bar {F.BAR_TIGHT:.3e})")
    assert worst <= F.BAR_TIGHT, worst


@radial_modes
@shapes
def test_each_frame_against_generate_default_tolerances(dev, flow, n, d, B, radial):
    """Case 4: nframes = 9 at the defaults 1e-6 / 1e-8; the bar of tests/frames_ref.py (3.145e-07)."""
    worst = _frames_against_generate(dev, flow, n, d, B, radial, F.NF_LOOSE, F.LOOSE)
    print(f"FRAMES defaults {n}x{d} B={B} {radial}: {worst:.3e} (bar {F.BAR_LOOSE:.3e})")
    assert worst <= F.BAR_LOOSE, worst


@shapes
def test_off_table_walker_redoes_every_frame(dev, flow, n, d, B):
    """Case 6: a particle at radius 40 (the table ends at 32) in one walker: every frame of every walker is the direct kernels'."""
    z = F.walkers(n, d, B).copy()
    z[B // 2, 0] = 0.0
    z[B // 2, 0, 0] = 40.0
    z = T(z, dev)
    ft = flow("table").generate(z, nframes=4)
    fd = flow("exact").generate(z, nframes=4)
    assert bool(torch.isfinite(fd).all()) and bits(ft, fd)


def test_two_frames_at_a_batch_that_loops_the_grid(dev, flow):
    """Cases 1 and 2 where a flow grid loops.  The table kernel takes one workgroup per group and never does; the capped direct
    kernel behind it does, when it has to redo the launch: one walker of the batch has a particle beyond the table (radius 40), so
    the direct frame-writing kernel strides over every walker in more than two rounds with a ragged end and rewrites both frames."""
    n, d = 6, 2
    fams = {}
    for call in ("flow", "flow_fb"):
        fams.update(kernel_families(call, n, d, cu_count()))
    assert any(r for _, r in fams.values()), fams          # at least one grid of the call is capped
    B = looping_batch(fams)
    assert_loops(fams, B)
    z = torch.randn(B, n, d, generator=torch.Generator().manual_seed(62), dtype=torch.float64)
    z[B - 2, 0] = 0.0
    z[B - 2, 0, 0] = 40.0
    z = z.to(dev)
    cnf = flow("table")
    fr = cnf.generate(z, nframes=2)
    x = cnf.generate(z)
    assert bits(fr[0], z) and bits(fr[1], x)
    # the direct kernels did serve both calls (the fallback's results are the exact net's), and the far rounds hold real frames
    exact = flow("exact")
    assert bits(x, exact.generate(z)) and bits(fr, exact.generate(z, nframes=2))
    assert bool(torch.isfinite(fr).all()) and not bits(fr[1], z)


def test_betavmc_sample_with_frames(dev):
    import fermiflow_amd as ff
    eta, mu = ff.MLP(1, 50), ff.MLP(1, 50)
    eta.init_gaussian(1); mu.init_gaussian(2)
    cnf = ff.CNF(ff.Backflow(eta, mu=mu), (0.0, 1.0))
    model = ff.BetaVMC(2.0, 3, 0, 2.0, True, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    model.to(device=dev)
    torch.manual_seed(3)
    z, x = model.sample((64,), nframes=4)
    assert z.shape == (64, 3, 2) and x.shape == (4, 64, 3, 2)
    assert bits(x[0], z) and bool(torch.isfinite(x).all())
    z2, x2 = model.sample((64,))
    assert x2.shape == (64, 3, 2)


def test_nframes_zero_is_a_value_error(dev, flow):
    z = T(F.walkers(3, 2, 13), dev)
    with pytest.raises(ValueError):
        flow("table").generate(z, nframes=0)


def test_generate_without_nframes_is_unchanged(dev, flow):
    from fermiflow_amd import native
    z = T(F.walkers(6, 2, 7), dev)
    cnf = flow("table")
    x = cnf.generate(z)
    assert x.shape == z.shape and bits(x, native.cnf_generate(cnf.v_wrapper.v.net(), z, F.T0, F.T1, cnf.rtol, cnf.atol))


def test_driver_writes_the_frames(dev, tmp_path):
    """--frames_out of the ground-state driver: t, frames, nup, ndown, dim of a fresh batch after the last iteration."""
    from fermiflow_amd import FermionHO2D
    out = str(tmp_path / "frames.npz")
    FermionHO2D.main(["--nup", "2", "--ndown", "1", "--Z", "2.0", "--batch", "512", "--iternum", "1", "--frames_out", out, "--nframes", "5",
                      "--frames_batch", "33"])
    with np.load(out) as f:
        assert f["frames"].shape == (5, 33, 3, 2) and np.isfinite(f["frames"]).all()
        assert np.array_equal(f["t"], np.linspace(0.0, 1.0, 5))
        assert (int(f["nup"]), int(f["ndown"]), int(f["dim"])) == (2, 1, 2)


def test_finite_temperature_driver_writes_the_frames(dev, tmp_path):
    from fermiflow_amd import BetaFermionHO2D
    out = str(tmp_path / "frames.npz")
    BetaFermionHO2D.main(["--nup", "2", "--ndown", "1", "--Z", "1.0", "--deltaE", "1.0", "--boltzmann", "--batch", "512", "--iternum", "1",
                          "--frames_out", out, "--nframes", "3", "--frames_batch", "40"])
    with np.load(out) as f:
        assert f["frames"].shape == (3, 40, 3, 2) and np.isfinite(f["frames"]).all()
        assert np.array_equal(f["t"], np.linspace(0.0, 1.0, 3)) and int(f["dim"]) == 2
