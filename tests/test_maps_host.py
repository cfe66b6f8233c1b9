"""Host-side surface of the density maps (fermiflow_amd.DensityMaps; include/fermiflow_maps.h), no GPU needed: the third public header
against its ctypes table, the class's argument checks, normalisation, state_dict and the rank sum on counts loaded through
load_state_dict, the drivers' flags, the checkpoint -- no kernel runs here."""
import os
import re

import numpy as np
import pytest
import torch

from tests import maps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(maps, hists, B):
    """counts of `hists` (per frame: a list of (6, nbins^2 + 2) per-call histograms of B walkers each) into maps"""
    rows = []
    for calls in hists:
        calls = [np.asarray(h, dtype=np.int64) for h in calls]
        rows.append(np.concatenate([[len(calls), B * len(calls)], sum(calls).reshape(-1)]))
    st = maps.state_dict()
    st["acc"] = torch.from_numpy(np.stack(rows).astype(np.int64))
    maps.load_state_dict(st)


def hist(seed, B, nup, ndn, extent, nbins, scale=1.2):
    return R.histogram(np.random.default_rng(seed).standard_normal((B, nup + ndn, 2)) * scale, nup, extent, nbins)


def test_third_header_is_plain_c99():
    import subprocess
    import tempfile
    src = ('#include "fermiflow_maps.h"\n#include <stdio.h>\n'
           'int main(void) { printf("%d %d\\n", FF_MAPS_PLANES, FF_MAPS_MAX_BINS); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        planes, max_bins = (int(v) for v in subprocess.check_output([exe]).split())
    from fermiflow_amd import _abi, observables
    assert planes == _abi.MAPS_PLANES == len(observables.PLANES) == len(R.PLANES)
    assert max_bins == _abi.MAPS_MAX_BINS == observables.MAPS_MAX_BINS


def test_maps_signature_table_is_the_third_header():
    """fermiflow_amd/_abi.py MAPS_SIGNATURES against include/fermiflow_maps.h, prototype by prototype (the method of
    tests/test_robust_host.py::test_robust_signature_table_is_the_second_header), and bind() has put the table on the library."""
    import ctypes as C
    from fermiflow_amd import _abi, _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fermiflow_maps.h")).read(), flags=re.S)
    protos = re.findall(r"^(int|int64_t|size_t|const char\*)\s+(ff_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    assert [name for _, name, _ in protos] == re.findall(r"\b(ff_\w+)\s*\(", hdr) and len(protos) == 2
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t,
             **dict.fromkeys(("const double*", "double*", "void*"), C.c_void_p)}
    parsed = {}
    for ret, name, params in protos:
        spellings = [re.sub(r"\s*\*", "*", re.sub(r"\w+$", "", " ".join(p.split())).strip()) for p in params.split(",") if p.strip() != "void"]
        for t in [ret] + spellings:
            assert t in ctype, f"{name}: the C type {t!r} is not in this test's dictionary"
        parsed[name] = (ctype[ret], tuple(ctype[t] for t in spellings))
    assert list(parsed) == list(_abi.MAPS_SIGNATURES)
    assert not set(parsed) & (set(_abi.SIGNATURES) | set(_abi.ROBUST_SIGNATURES))      # the other headers' tables are untouched
    assert not set(parsed) & set(_lib.SYMBOLS)
    for name, sig in parsed.items():
        fn = getattr(_lib.lib(), name)      # the library exports it ...
        assert _abi.MAPS_SIGNATURES[name] == sig == (fn.restype, tuple(fn.argtypes)), name
    assert _lib.lib().ff_version() == _abi.ABI_VERSION == 110


def test_library_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from fermiflow_amd import _lib
    lib, p8 = _lib.lib(), C.c_void_p(8)
    assert lib.ff_maps_accumulate(None, 4, 3, 3, None, 6.0, 16, p8) == 1
    assert lib.ff_maps_accumulate(None, 4, 3, 3, p8, 6.0, 16, None) == 1
    assert lib.ff_maps_accumulate(None, -1, 3, 3, p8, 6.0, 16, p8) == 1
    assert lib.ff_maps_accumulate(None, 4, 0, 0, p8, 6.0, 16, p8) == 1
    for extent in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ff_maps_accumulate(None, 4, 3, 3, p8, extent, 16, p8) == 1
    assert lib.ff_maps_accumulate(None, 4, 3, 3, p8, 6.0, 129, p8) == 2
    assert lib.ff_maps_accumulate(None, 4, 13, 12, p8, 6.0, 16, p8) == 2
    assert lib.ff_last_error().decode().startswith("ff_maps:")
    assert lib.ff_maps_buffer_bytes(128) == 8 * (2 + 6 * (128 * 128 + 2)) and lib.ff_maps_buffer_bytes(129) == 0


def test_class_argument_checks():
    from fermiflow_amd import DensityMaps
    m = DensityMaps(3, 3)
    assert (m.extent, m.nbins, m.nframes) == (6.0, 128, 1)
    for kw in (dict(nbins=0), dict(nbins=129), dict(extent=0.0), dict(extent=float("inf")), dict(extent=float("nan")), dict(nframes=0)):
        with pytest.raises(ValueError):
            DensityMaps(3, 3, **kw)
    for nup, ndn in ((0, 0), (-1, 3), (3, -1)):
        with pytest.raises(ValueError):
            DensityMaps(nup, ndn)
    with pytest.raises(NotImplementedError):
        DensityMaps(13, 12)
    with pytest.raises(RuntimeError):
        m.accumulate(torch.zeros(4, 6, 2, dtype=torch.float64))          # no CPU path
    with pytest.raises(IndexError):
        m.counts(frame=1)
    # shapes are checked before anything is launched (on tensors the device check has let through: here, meta tensors cannot be used, so
    # the check itself is called)
    for shape in ((4, 6), (4, 5, 2), (4, 6, 1), (2, 4, 6, 2)):
        with pytest.raises(ValueError):
            m._check_x(torch.zeros(shape, dtype=torch.float64), "accumulate")
    with pytest.raises(ValueError, match="two-dimensional"):
        m._check_x(torch.zeros(4, 6, 3, dtype=torch.float64), "accumulate")
    m._check_x(torch.zeros(4, 6, 2, dtype=torch.float64), "accumulate")
    k = DensityMaps(3, 3, nframes=5)
    k._check_x(torch.zeros(5, 4, 6, 2, dtype=torch.float64), "accumulate_frames", lead=(5,))
    for shape in ((4, 4, 6, 2), (4, 6, 2), (5, 4, 6, 1)):
        with pytest.raises(ValueError):
            k._check_x(torch.zeros(shape, dtype=torch.float64), "accumulate_frames", lead=(5,))
    with pytest.raises(ValueError, match="two-dimensional"):
        k._check_x(torch.zeros(5, 4, 6, 3, dtype=torch.float64), "accumulate_frames", lead=(5,))


def test_normalisation_identities_on_hand_made_counts():
    from fermiflow_amd import DensityMaps
    nup, ndn, nbins, extent, B = 4, 3, 20, 3.0, 400          # a window the walkers leave: the lost share is not zero
    maps = DensityMaps(nup, ndn, extent=extent, nbins=nbins, nframes=2)
    hs = [[hist(s, B, nup, ndn, extent, nbins) for s in range(3)], [hist(10 + s, B, nup, ndn, extent, nbins) for s in range(2)]]
    full = int(np.argmax(hs[1][0][2, :nbins * nbins]))        # (and an invalid share, by hand: five samples of the fullest uu cell)
    assert hs[1][0][2, full] >= 5
    hs[1][0][2, full] -= 5
    hs[1][0][2, nbins * nbins + 1] += 5
    load(maps, hs, B)
    x_mid, y_mid = maps.xy_mid()
    edges = np.linspace(-extent, extent, nbins + 1)
    assert np.allclose(x_mid, 0.5 * (edges[1:] + edges[:-1]), rtol=0, atol=1e-14) and np.array_equal(x_mid, y_mid)
    assert abs(maps.cell_area - (2 * extent / nbins) ** 2) < 1e-15
    per = maps.samples_per_walker()
    assert [per[k] for k in R.PLANES] == list(R.samples_per_walker(nup, ndn))
    for frame, calls in enumerate(hs):
        c = maps.counts(frame)
        total = sum(calls)
        assert (c["calls"], c["walkers"]) == (len(calls), B * len(calls))
        vals = {**maps.density(frame), **maps.pair_density(frame)}
        assert set(maps.density(frame)) == {"up", "down"} and set(maps.pair_density(frame)) == {"uu", "ud", "du", "dd"}
        for k, name in enumerate(R.PLANES):
            assert c[name].shape == (nbins, nbins) and c[name].dtype == np.int64
            assert np.array_equal(c[name].reshape(-1), total[k, :nbins * nbins])
            assert c["lost_" + name] == (total[k, nbins * nbins], total[k, nbins * nbins + 1])
            lost = sum(c["lost_" + name]) / c["walkers"]
            assert lost > 0
            assert abs((vals[name] * maps.cell_area).sum() - (per[name] - lost)) < 1e-12 * per[name]
    # the first index is x: a walker at (x, y) = (1.0, -2.0) is counted at [ix, iy] with x_mid[ix] ~ 1, y_mid[iy] ~ -2
    one = DensityMaps(1, 0, extent=extent, nbins=nbins)
    load(one, [[R.histogram(np.array([[[1.0, -2.0]]]), 1, extent, nbins)]], 1)
    ix, iy = np.argwhere(one.counts()["up"] == 1)[0]
    assert abs(x_mid[ix] - 1.0) <= extent / nbins and abs(y_mid[iy] + 2.0) <= extent / nbins


def test_state_dict_round_trip_reset_and_geometry_check(tmp_path):
    from fermiflow_amd import DensityMaps
    maps = DensityMaps(2, 1, extent=4.0, nbins=12, nframes=2)
    load(maps, [[hist(s, 50, 2, 1, 4.0, 12) for s in range(3)], [hist(7, 50, 2, 1, 4.0, 12)]], 50)
    st = maps.state_dict()
    other = DensityMaps(2, 1, extent=4.0, nbins=12, nframes=2)
    other.load_state_dict(st)
    assert torch.equal(other.state_dict()["acc"], st["acc"]) and other._B == [50, 50]
    for frame in (0, 1):
        a, b = maps.counts(frame), other.counts(frame)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    for kw in (dict(nbins=13), dict(extent=5.0), dict(nframes=1)):
        with pytest.raises(ValueError):
            DensityMaps(2, 1, **{**dict(extent=4.0, nbins=12, nframes=2), **kw}).load_state_dict(st)
    out = str(tmp_path / "maps.npz")
    maps.save_npz(out)
    f = np.load(out)
    assert f["rho_up"].shape == (2, 12, 12) and f["g_ud"].shape == (2, 12, 12) and f["lost_du"].shape == (2, 2)
    assert list(f["calls"]) == [3, 1] and list(f["walkers"]) == [150, 50] and int(f["nbins"]) == 12 and float(f["extent"]) == 4.0
    assert np.array_equal(f["counts_uu"][1], maps.counts(1)["uu"]) and np.array_equal(f["rho_down"][0], maps.density(0)["down"])
    assert np.array_equal(f["x_mid"], maps.xy_mid()[0])
    other.reset()
    assert other.counts()["calls"] == 0 and not other.counts(1)["ud"].any() and other._B == [None, None]


def test_all_reduce_in_one_process_is_the_identity():
    from fermiflow_amd import DensityMaps
    maps = DensityMaps(2, 1, extent=4.0, nbins=12)
    load(maps, [[hist(s, 30, 2, 1, 4.0, 12) for s in range(2)]], 30)
    before = maps.state_dict()["acc"].clone()
    maps.all_reduce_()
    assert torch.equal(maps.state_dict()["acc"], before)
    st = maps.state_dict()
    st["acc"][0, 5] = 2 ** 53          # a count the sum over ranks as doubles could not carry exactly
    maps.load_state_dict(st)
    with pytest.raises(OverflowError):
        maps.all_reduce_()


def test_checkpoint_carries_the_maps(tmp_path):
    from fermiflow_amd import DensityMaps, Observables, checkpoint
    model = torch.nn.Linear(2, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    maps = DensityMaps(2, 1, extent=4.0, nbins=12)
    load(maps, [[hist(s, 30, 2, 1, 4.0, 12) for s in range(3)]], 30)
    path = str(tmp_path / "ck.pt")
    checkpoint.save(path, model, opt, 3, maps=maps)
    other = DensityMaps(2, 1, extent=4.0, nbins=12)
    assert checkpoint.load(path, model, opt, maps=other) == 3
    assert torch.equal(other.state_dict()["acc"], maps.state_dict()["acc"]) and other.counts()["calls"] == 3
    assert checkpoint.load(path, model, opt) == 3                                     # nobody asks for them: ignored
    obs = Observables(2, 1, rmax=6.0, nbins=16)
    assert checkpoint.load(path, model, opt, observables=obs) == 3 and obs.counts()["calls"] == 0
    with pytest.raises(ValueError):
        checkpoint.load(path, model, opt, maps=DensityMaps(2, 1, extent=5.0, nbins=12))      # another geometry
    checkpoint.save(path, model, opt, 4)                                              # a checkpoint without maps
    assert checkpoint.load(path, model, opt, maps=other) == 4 and other.counts()["calls"] == 3


def test_sweeps_have_the_attribute():
    import fermiflow_amd as ff
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=ff.MLP(1, 4)), (0.0, 1.0))
    m = ff.GSVMC(3, 3, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(2.0), sp_potential=ff.HO())
    assert m.density_maps is None and m.observables is None
    b = ff.BetaVMC(2.0, 2, 1, 2, True, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    assert b.density_maps is None
    assert "density_maps" not in m.state_dict() and not any("maps" in k for k in m.state_dict())      # a setting, not sweep state


@pytest.mark.parametrize("driver", ["FermionHO2D", "BetaFermionHO2D"])
def test_driver_flags_and_parser_errors(driver):
    import importlib
    from fermiflow_amd import frames
    mod = importlib.import_module("fermiflow_amd." + driver)
    p = mod.build_parser()
    a = p.parse_args([])
    assert (a.maps_out, a.maps_extent, a.maps_bins, a.frames_maps_out) == (None, 6.0, 128, None)
    frames.check_arguments(p, a)
    a = p.parse_args(["--maps_out", "m.npz", "--maps_extent", "4.5", "--maps_bins", "64", "--frames_maps_out", "f.npz"])
    assert (a.maps_out, a.maps_extent, a.maps_bins, a.frames_maps_out) == ("m.npz", 4.5, 64, "f.npz")
    frames.check_arguments(p, a)
    bad = [["--maps_out", "m.npz", "--maps_bins", "129"], ["--maps_out", "m.npz", "--maps_bins", "0"], ["--maps_out", "m.npz", "--maps_extent", "0"],
           ["--frames_maps_out", "f.npz", "--maps_extent", "inf"], ["--frames_maps_out", "f.npz", "--nframes", "0"],
           ["--frames_maps_out", "f.npz", "--frames_batch", "0"]]
    if driver == "FermionHO2D":
        bad += [["--dim", "3", "--maps_out", "m.npz"], ["--dim", "3", "--frames_maps_out", "f.npz"]]
        frames.check_arguments(p, p.parse_args(["--dim", "3"]))          # --dim 3 alone is fine
    for flags in bad:
        with pytest.raises(SystemExit):
            mod.main(flags)          # refused by the parser, before the device is touched
