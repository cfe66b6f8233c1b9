"""Host-side surface of the one-body density matrix (fermiflow_amd.OneBodyDensityMatrix; include/fermiflow_obdm.h), no GPU needed: the
fourth public header against its ctypes table, the class's argument checks, the n(k), density and occupation formulas on hand-made
matrices, state_dict and save_npz, the drivers' flags, the sweeps' attribute -- no kernel runs here."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import obdm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(obj, mats, B, invalid=(0, 0)):
    """the per-call matrices `mats` (calls, 2, nb, nb) of B walkers each into obj"""
    mats = np.asarray(mats, dtype=np.float64)
    st = obj.state_dict()
    head = np.array([len(mats), B * len(mats), invalid[0], invalid[1], 0], dtype=np.int64)
    body = np.concatenate([mats.sum(0).reshape(-1), (mats * mats).sum(0).reshape(-1)]).view(np.int64)
    st["acc"] = torch.from_numpy(np.concatenate([head, body]))
    obj.load_state_dict(st)


def test_fourth_header_is_plain_c99():
    import subprocess
    import tempfile
    src = ('#include "fermiflow_obdm.h"\n#include <stdio.h>\n'
           'int main(void) { printf("%d %d %d\\n", FF_OBDM_MAX_SHELLS, FF_OBDM_CHUNK, FF_OBDM_HEAD); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        shells, chunk, head = (int(v) for v in subprocess.check_output([exe]).split())
    from fermiflow_amd import _abi, observables
    assert shells == _abi.OBDM_MAX_SHELLS == observables.OBDM_MAX_SHELLS == 8
    assert chunk == _abi.OBDM_CHUNK == R.CHUNK and head == _abi.OBDM_HEAD == R.HEAD == observables._OBDM_HEAD


def test_obdm_signature_table_is_the_fourth_header():
    """fermiflow_amd/_abi.py OBDM_SIGNATURES against include/fermiflow_obdm.h, prototype by prototype (the method of
    tests/test_maps_host.py), disjoint from the other three tables, and bind() has put the table on the library."""
    import ctypes as C
    from fermiflow_amd import _abi, _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fermiflow_obdm.h")).read(), flags=re.S)
    protos = re.findall(r"^(int|int64_t|size_t|const char\*)\s+(ff_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    assert [name for _, name, _ in protos] == re.findall(r"\b(ff_\w+)\s*\(", hdr) and len(protos) == 4
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t,
             **dict.fromkeys(("const double*", "double*", "void*", "const int32_t*"), C.c_void_p)}
    parsed = {}
    for ret, name, params in protos:
        spellings = [re.sub(r"\s*\*", "*", re.sub(r"\w+$", "", " ".join(p.split())).strip()) for p in params.split(",") if p.strip() != "void"]
        for t in [ret] + spellings:
            assert t in ctype, f"{name}: the C type {t!r} is not in this test's dictionary"
        parsed[name] = (ctype[ret], tuple(ctype[t] for t in spellings))
    assert list(parsed) == list(_abi.OBDM_SIGNATURES)
    assert not set(parsed) & (set(_abi.SIGNATURES) | set(_abi.ROBUST_SIGNATURES) | set(_abi.MAPS_SIGNATURES))
    assert not set(parsed) & set(_lib.SYMBOLS)
    for name, sig in parsed.items():
        fn = getattr(_lib.lib(), name)      # the library exports it ...
        assert _abi.OBDM_SIGNATURES[name] == sig == (fn.restype, tuple(fn.argtypes)), name
    assert _lib.lib().ff_version() == _abi.ABI_VERSION == 110


def test_library_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from fermiflow_amd import _lib
    lib, p8 = _lib.lib(), C.c_void_p(8)
    ok = (p8,) * 6
    assert lib.ff_obdm_accumulate(None, 4, 3, 3, None, p8, p8, p8, p8, p8, 1.0, 4, p8, p8) == 1
    assert lib.ff_obdm_accumulate(None, 4, 3, 3, *ok, 1.0, 4, None, p8) == 1
    assert lib.ff_obdm_accumulate(None, 4, 3, 3, *ok, 1.0, 4, p8, None) == 1
    assert lib.ff_obdm_accumulate(None, -1, 3, 3, *ok, 1.0, 4, p8, p8) == 1
    assert lib.ff_obdm_accumulate(None, 4, 0, 0, *ok, 1.0, 4, p8, p8) == 1
    assert lib.ff_obdm_accumulate(None, 4, 3, 3, *ok, 1.0, 0, p8, p8) == 1
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ff_obdm_accumulate(None, 4, 3, 3, *ok, sigma, 4, p8, p8) == 1
    assert lib.ff_obdm_accumulate(None, 4, 3, 3, *ok, 1.0, 9, p8, p8) == 2
    assert lib.ff_obdm_accumulate(None, 4, 13, 12, *ok, 1.0, 4, p8, p8) == 2
    assert lib.ff_obdm_accumulate(None, 4, 13, 3, *ok, 1.0, 4, p8, p8) == 2
    assert lib.ff_obdm_accumulate(None, 1 << 31, 3, 3, *ok, 1.0, 4, p8, p8) == 2
    assert lib.ff_last_error().decode().startswith("ff_obdm:")
    assert lib.ff_slater_sign(None, 4, 3, 3, p8, p8, None, None, p8) == 1
    assert lib.ff_slater_sign(None, 4, 3, 3, None, p8, None, p8, p8) == 1
    assert lib.ff_slater_sign(None, 4, 13, 3, p8, p8, None, p8, p8) == 2
    assert lib.ff_last_error().decode().startswith("ff_obdm:")
    assert lib.ff_obdm_buffer_bytes(4) == 8 * (5 + 400) and lib.ff_obdm_buffer_bytes(9) == 0 and lib.ff_obdm_buffer_bytes(0) == 0
    assert lib.ff_obdm_workspace_bytes(65536, 4) == 8 * 200 * 256 and lib.ff_obdm_workspace_bytes(1 << 31, 4) == 0


def test_class_argument_checks():
    from fermiflow_amd import OneBodyDensityMatrix
    m = OneBodyDensityMatrix(3, 3)
    assert (m.nshells, m.sigma, m.every, m.stride, m.seed, m.nb) == (4, 1.0, 1, 1, 0, 10)
    for kw in (dict(nshells=0), dict(nshells=9), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma=float("nan")),
               dict(every=0), dict(stride=0)):
        with pytest.raises(ValueError):
            OneBodyDensityMatrix(3, 3, **kw)
    for nup, ndn in ((0, 0), (-1, 3), (3, -1)):
        with pytest.raises(ValueError):
            OneBodyDensityMatrix(nup, ndn)
    for nup, ndn in ((13, 12), (13, 0), (0, 13)):
        with pytest.raises(NotImplementedError):
            OneBodyDensityMatrix(nup, ndn)
    z = torch.zeros(4, 6, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):          # no CPU path
        m.accumulate_raw(z, torch.zeros(4, 2, 2, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                         torch.zeros(4, 6, dtype=torch.float64), torch.zeros(4, 6, dtype=torch.float64))
    c = m.counts()
    assert c["calls"] == 0 and c["walkers"] == 0 and c["invalid_up"] == 0
    assert np.isnan(m.matrix_err()["up"]).all()


def _ground(nb, nocc):
    rho = np.zeros((nb, nb))
    rho[range(nocc), range(nocc)] = 1.0
    return rho


def test_momentum_distribution_and_density_of_a_closed_shell():
    """rho = the identity on the occupied orbitals of (3, 0): n(k) integrates to 3 on a grid and, the occupied shells being closed,
    n(k) = rho(r = k) (an oscillator eigenfunction is its own Fourier transform up to a phase)."""
    from fermiflow_amd import OneBodyDensityMatrix, observables
    obj = OneBodyDensityMatrix(3, 0, nshells=3)
    load(obj, [np.stack([_ground(6, 3), np.zeros((6, 6))])] * 2, 1)
    assert obj.degrees() == R.degrees(6) == [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]
    g = np.linspace(-7.0, 7.0, 281)
    kx, ky = np.meshgrid(g, g, indexing="ij")
    h2 = (g[1] - g[0]) ** 2
    nk, rho = obj.momentum_distribution(kx, ky), obj.density(kx, ky)
    assert abs(nk["up"].sum() * h2 - 3.0) < 1e-9 and abs(rho["up"].sum() * h2 - 3.0) < 1e-9
    assert np.abs(nk["up"] - rho["up"]).max() < 1e-14 and not nk["down"].any()
    # against the closed form: (1 + 2 k^2) exp(-k^2) / pi
    k2 = kx * kx + ky * ky
    assert np.abs(nk["up"] - (1.0 + 2.0 * k2) * np.exp(-k2) / math.pi).max() < 1e-13
    # the basis on the host is the reference's
    assert np.abs(observables.ho2d_basis(8, kx[::7, ::9], ky[::7, ::9]) - np.moveaxis(R.orbitals(range(36), kx[::7, ::9], ky[::7, ::9]), -1, 0)).max() < 1e-15


def test_momentum_distribution_phases():
    """A coherence between shells N and N + 1 carries the phase cos(pi / 2) = 0, between N and N + 2 the phase -1: it leaves n(k) or
    enters it with the opposite sign of the density's; the integral of n(k) is the trace whatever the coherences."""
    from fermiflow_amd import OneBodyDensityMatrix
    obj = OneBodyDensityMatrix(1, 0, nshells=3)
    rho = np.diag([0.5, 0.2, 0.1, 0.1, 0.05, 0.05])
    rho[0, 1] = rho[1, 0] = 0.07          # shells 0, 1
    rho[0, 5] = rho[5, 0] = 0.03          # shells 0, 2
    load(obj, [np.stack([rho, np.zeros((6, 6))])], 1)
    g = np.linspace(-8.0, 8.0, 321)
    kx, ky = np.meshgrid(g, g, indexing="ij")
    h2 = (g[1] - g[0]) ** 2
    nk, dens = obj.momentum_distribution(kx, ky)["up"], obj.density(kx, ky)["up"]
    assert abs(nk.sum() * h2 - np.trace(rho)) < 1e-9 and abs(dens.sum() * h2 - np.trace(rho)) < 1e-9
    phi = np.moveaxis(R.orbitals(range(6), kx, ky), -1, 0)
    diag = np.einsum("a,a...->...", np.diag(rho), phi * phi)
    assert np.abs(nk - (diag - 2 * 0.03 * phi[0] * phi[5])).max() < 1e-14
    assert np.abs(dens - (diag + 2 * 0.07 * phi[0] * phi[1] + 2 * 0.03 * phi[0] * phi[5])).max() < 1e-14


def test_occupations_of_a_known_matrix():
    from fermiflow_amd import OneBodyDensityMatrix
    rng = np.random.default_rng(4)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    occ = np.array([0.97, 0.9, 0.6, 0.3, 0.05, 0.01])
    rho = (Q * occ) @ Q.T
    rho = 0.5 * (rho + rho.T)
    obj = OneBodyDensityMatrix(2, 2, nshells=3)
    load(obj, [np.stack([rho, _ground(6, 2)]) * 8.0] * 3, 8)          # three calls of 8 walkers: sum / walkers = rho
    out = obj.occupations()
    w, v = out["up"]
    assert np.abs(w - occ).max() < 1e-14 and (np.diff(w) <= 0).all()
    assert np.abs(np.abs(v.T @ Q) - np.eye(6)).max() < 1e-12          # column k is natural orbital k (up to its sign)
    assert np.abs(out["down"][0] - np.array([1, 1, 0, 0, 0, 0])).max() < 1e-14
    assert np.abs(obj.matrix()["up"] - rho).max() < 1e-15
    # equal blocks: no spread, up to the cancellation in sumsq / m - mean^2 (a variance of a few eps T^2: an error of sqrt(eps) |rho|)
    assert obj.matrix_err()["up"].max() < 4.0 * math.sqrt(R.EPS)


def test_block_errors_follow_the_observables_formula():
    from fermiflow_amd import OneBodyDensityMatrix
    rng = np.random.default_rng(6)
    mats = rng.standard_normal((5, 2, 3, 3))
    mats = mats + mats.transpose(0, 1, 3, 2)
    obj = OneBodyDensityMatrix(1, 1, nshells=2)
    load(obj, mats, 10)
    err = obj.matrix_err()
    want = mats.std(0, ddof=1) / math.sqrt(5) / 10.0
    assert np.abs(err["up"] - want[0]).max() < 1e-12 and np.abs(err["down"] - want[1]).max() < 1e-12
    assert np.abs(obj.matrix()["down"] - mats.sum(0)[1] / 50.0).max() < 1e-15


def test_state_dict_round_trip_reset_and_npz(tmp_path):
    from fermiflow_amd import OneBodyDensityMatrix
    rng = np.random.default_rng(8)
    mats = rng.standard_normal((4, 2, 6, 6))
    mats = mats + mats.transpose(0, 1, 3, 2)
    obj = OneBodyDensityMatrix(2, 1, nshells=3, sigma=1.25)
    load(obj, mats, 20, invalid=(3, 1))
    st = obj.state_dict()
    other = OneBodyDensityMatrix(2, 1, nshells=3, sigma=1.25)
    other.load_state_dict(st)
    assert torch.equal(other.state_dict()["acc"], st["acc"]) and other._B == 20
    assert other.counts() == obj.counts() == {"calls": 4, "walkers": 80, "invalid_up": 3, "invalid_down": 1, "samples_up": 160, "samples_down": 80}
    for kw in (dict(nshells=4), dict(sigma=1.0), dict(nup=1, ndown=2)):
        with pytest.raises(ValueError):
            OneBodyDensityMatrix(**{**dict(nup=2, ndown=1, nshells=3, sigma=1.25), **kw}).load_state_dict(st)
    before = st["acc"].clone()
    obj.all_reduce_()                                                  # one process: the identity, bit for bit
    assert torch.equal(obj.state_dict()["acc"], before)
    out = str(tmp_path / "obdm.npz")
    obj.save_npz(out)
    f = np.load(out)
    assert f["rho_up"].shape == (6, 6) and np.array_equal(f["rho_down"], obj.matrix()["down"]) and np.array_equal(f["err_up"], obj.matrix_err()["up"])
    assert np.array_equal(f["occ_up"], obj.occupations()["up"][0]) and f["natorb_down"].shape == (6, 6)
    assert (int(f["calls"]), int(f["walkers"]), list(f["invalid"])) == (4, 80, [3, 1])
    assert (int(f["nshells"]), float(f["sigma"]), f["degrees"].tolist()) == (3, 1.25, [list(d) for d in R.degrees(6)])
    assert np.array_equal(f["sum"], mats.sum(0))
    other.reset()
    assert other.counts()["calls"] == 0 and not other.state_dict()["acc"].any() and other._B is None


def test_sweeps_have_the_attribute_and_three_dimensions_are_refused():
    import fermiflow_amd as ff
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=ff.MLP(1, 4)), (0.0, 1.0))
    m = ff.GSVMC(3, 3, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(2.0), sp_potential=ff.HO())
    assert m.obdm is None
    obj = ff.OneBodyDensityMatrix(3, 3)
    m.obdm = obj
    assert m.obdm is obj
    assert not any("obdm" in k for k in m.state_dict())      # a setting, not sweep state
    m.obdm = None
    b = ff.BetaVMC(2.0, 2, 1, 2, True, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    assert b.obdm is None
    b.obdm = ff.OneBodyDensityMatrix(2, 1)
    m3 = ff.GSVMC(2, 2, ff.HO3D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(2.0), sp_potential=ff.HO())
    assert m3.obdm is None
    with pytest.raises(NotImplementedError):
        m3.obdm = ff.OneBodyDensityMatrix(2, 2)
    m3.obdm = None


@pytest.mark.parametrize("driver", ["FermionHO2D", "BetaFermionHO2D"])
def test_driver_flags_and_parser_errors(driver):
    import importlib
    from fermiflow_amd import frames
    mod = importlib.import_module("fermiflow_amd." + driver)
    p = mod.build_parser()
    a = p.parse_args([])
    assert (a.obdm_out, a.obdm_shells, a.obdm_sigma, a.obdm_every, a.obdm_stride) == (None, 4, 1.0, 1, 1)
    frames.check_arguments(p, a)
    a = p.parse_args(["--obdm_out", "o.npz", "--obdm_shells", "6", "--obdm_sigma", "1.4", "--obdm_every", "5", "--obdm_stride", "8"])
    assert (a.obdm_out, a.obdm_shells, a.obdm_sigma, a.obdm_every, a.obdm_stride) == ("o.npz", 6, 1.4, 5, 8)
    frames.check_arguments(p, a)
    bad = [["--obdm_out", "o.npz", "--obdm_shells", "9"], ["--obdm_out", "o.npz", "--obdm_shells", "0"], ["--obdm_out", "o.npz", "--obdm_sigma", "0"],
           ["--obdm_out", "o.npz", "--obdm_sigma", "inf"], ["--obdm_out", "o.npz", "--obdm_every", "0"], ["--obdm_out", "o.npz", "--obdm_stride", "0"]]
    if driver == "FermionHO2D":
        bad += [["--dim", "3", "--obdm_out", "o.npz"]]
        frames.check_arguments(p, p.parse_args(["--dim", "3"]))          # --dim 3 alone is fine
    for flags in bad:
        with pytest.raises(SystemExit):
            mod.main(flags)          # refused by the parser, before the device is touched
