"""CNF.generate(z, nframes) and the drivers' --frames_out flags without a GPU: argument validation only.  The kernels are tested
under the host simulator (tests/test_frames_hostsim.py) and on the device (tests/test_gpu_frames.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fermiflow_amd as ff
from fermiflow_amd import BetaFermionHO2D, FermionHO2D, _lib, frames, native


@pytest.fixture(scope="module")
def cnf():
    return ff.CNF(ff.Backflow(ff.MLP(1, 8), mu=ff.MLP(1, 8)), (0.0, 1.0))


@pytest.mark.parametrize("bad", [0, -1, 2.0, 2.5, "3", True, [2]])
def test_nframes_must_be_an_integer_of_at_least_one(cnf, bad):
    z = torch.zeros(4, 3, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="nframes"):
        cnf.generate(z, nframes=bad)


@pytest.mark.parametrize("k", [1, 2, np.int64(5)])
def test_a_cpu_tensor_is_refused_as_everywhere(cnf, k):
    """no fallback: the frames path raises what every native call raises for a CPU tensor, not NotImplementedError"""
    z = torch.zeros(4, 3, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device") as e:
        cnf.generate(z, nframes=k)
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="ROCm device"):
        native.cnf_generate_frames(None, z, 3, 0.0, 1.0, 1e-6, 1e-8)


def test_the_symbol_is_bound_and_exported():
    assert "ff_cnf_generate_frames" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "ff_cnf_generate_frames")
    assert _lib.lib().ff_version() == _lib.ABI_VERSION          # no struct of the header changed


@pytest.mark.parametrize("driver", [FermionHO2D, BetaFermionHO2D], ids=["ground_state", "finite_temperature"])
def test_driver_flags(driver, capsys):
    p = driver.build_parser()
    a = p.parse_args([])
    assert a.frames_out is None and (a.nframes, a.frames_batch) == (50, 1024)      # absent from the run when not given
    a = p.parse_args(["--frames_out", "f.npz", "--nframes", "7", "--frames_batch", "96"])
    assert (a.frames_out, a.nframes, a.frames_batch) == ("f.npz", 7, 96)
    frames.check_arguments(p, a)
    for flags in (["--nframes", "0"], ["--frames_batch", "0"]):
        with pytest.raises(SystemExit):
            frames.check_arguments(p, p.parse_args(["--frames_out", "f.npz"] + flags))
    frames.check_arguments(p, p.parse_args(["--nframes", "0"]))          # without --frames_out the other two are not looked at
    with pytest.raises(SystemExit):
        p.parse_args(["--nframes", "many"])
    capsys.readouterr()


def test_npz_layout(tmp_path):
    fr = torch.arange(3 * 2 * 3 * 2, dtype=torch.float64).reshape(3, 2, 3, 2)
    out = str(tmp_path / "frames.npz")
    frames.save_npz(out, fr, (0.5, 1.5), 2, 1, 2)
    with np.load(out) as f:
        assert sorted(f.files) == ["dim", "frames", "ndown", "nup", "t"]
        assert np.array_equal(f["frames"], fr.numpy()) and np.array_equal(f["t"], [0.5, 1.0, 1.5])
        assert (int(f["nup"]), int(f["ndown"]), int(f["dim"])) == (2, 1, 2)


def test_frame_kernels_round_like_their_mode_0_twins():
    """nframes = 2 promises the bits of generate(z): in the built library every frame-writing flow kernel contracts the
    Dormand-Prince sums into the same multiplications and fused multiply-adds as its mode-0 twin (csrc/ff_dp5.h, PIN_B)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_frames_contraction.py"), _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "34 pair(s) of kernels compared, 0 differ" in r.stdout, r.stdout
