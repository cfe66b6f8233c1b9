"""Host-side surface of the energy components (fermiflow_amd.EnergyParts; include/fermiflow_energy.h), no GPU needed: the fifth public
header against its ctypes table, the library's refusals and sizes, the class's argument checks and formulas on hand-made moments,
state_dict and save_npz, the drivers' flag, the sweeps' attribute -- no kernel runs here."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import energy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES10 = list(R.NAMES) + list(R.DERIVED)


def load(obj, calls, invalid=0, state=None):
    """per-call component tables `calls` (list of (B, 6) arrays of valid walkers) into obj, about its centre; state: per-call state lists"""
    ctr = np.asarray(obj.centre)
    d = [np.asarray(c, dtype=np.float64) - ctr for c in calls]
    B = len(d[0]) + invalid
    head = np.array([len(d), sum(len(c) for c in d), invalid * len(d), 0], dtype=np.int64)
    s = sum(c.sum(0) for c in d)
    s2 = sum(c.T @ c for c in d)
    bsq = sum(c.sum(0) ** 2 for c in d)
    words = [head, s.view(np.int64), s2.reshape(-1).view(np.int64), bsq.view(np.int64)]
    if obj.nstates:
        S = obj.nstates
        cnt, ss, e2 = np.zeros(S, dtype=np.int64), np.zeros((S, 6)), np.zeros(S)
        for c, st in zip(d, state):
            for k in range(S):
                m = np.asarray(st) == k
                cnt[k] += m.sum()
                ss[k] += c[m].sum(0)
                e2[k] += (c[m][:, list(R.E_PARTS)].sum(1) ** 2).sum()
        words += [cnt, ss.reshape(-1).view(np.int64), e2.view(np.int64)]
    st = obj.state_dict()
    st["acc"] = torch.from_numpy(np.concatenate(words))
    obj.load_state_dict(st)
    return B


def test_fifth_header_is_plain_c99():
    import subprocess
    import tempfile
    src = ('#include "fermiflow_energy.h"\n#include <stdio.h>\n'
           'int main(void) { printf("%d %d %d %d %d %d\\n", FF_ENERGY_PARTS, FF_ENERGY_CHUNK, FF_ENERGY_PARTIAL, FF_ENERGY_HEAD, FF_ENERGY_FIXED, '
           'FF_ENERGY_MAX_STATES); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = tuple(int(v) for v in subprocess.check_output([exe]).split())
    from fermiflow_amd import _abi, observables
    assert got == (_abi.ENERGY_PARTS, _abi.ENERGY_CHUNK, _abi.ENERGY_PARTIAL, _abi.ENERGY_HEAD, _abi.ENERGY_FIXED, _abi.ENERGY_MAX_STATES)
    assert got == (R.K, R.CHUNK, R.PARTIAL, R.HEAD, R.FIXED, R.MAX_STATES) == (6, 256, 28, 4, 52, 65536)
    assert (observables._EN_K, observables._EN_HEAD, observables._EN_FIXED, observables.ENERGY_MAX_STATES) == (6, 4, 52, 65536)
    assert got[5] >= 65536 and got[4] == got[3] + 6 + 36 + 6
    assert observables.ENERGY_NAMES == R.NAMES and observables.ENERGY_DERIVED == R.DERIVED


def test_energy_signature_table_is_the_fifth_header():
    """fermiflow_amd/_abi.py ENERGY_SIGNATURES against include/fermiflow_energy.h, prototype by prototype (the method of
    tests/test_obdm_host.py), disjoint from the other four tables, and bind() has put the table on the library."""
    import ctypes as C
    from fermiflow_amd import _abi, _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fermiflow_energy.h")).read(), flags=re.S)
    protos = re.findall(r"^(int|int64_t|size_t|const char\*)\s+(ff_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    assert [name for _, name, _ in protos] == re.findall(r"\b(ff_\w+)\s*\(", hdr) and len(protos) == 3
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t,
             **dict.fromkeys(("const double*", "double*", "void*", "const int32_t*"), C.c_void_p)}
    parsed = {}
    for ret, name, params in protos:
        spellings = [re.sub(r"\s*\*", "*", re.sub(r"\w+$", "", " ".join(p.split())).strip()) for p in params.split(",") if p.strip() != "void"]
        for t in [ret] + spellings:
            assert t in ctype, f"{name}: the C type {t!r} is not in this test's dictionary"
        parsed[name] = (ctype[ret], tuple(ctype[t] for t in spellings))
    assert list(parsed) == list(_abi.ENERGY_SIGNATURES)
    assert not set(parsed) & (set(_abi.SIGNATURES) | set(_abi.ROBUST_SIGNATURES) | set(_abi.MAPS_SIGNATURES) | set(_abi.OBDM_SIGNATURES))
    assert not set(parsed) & set(_lib.SYMBOLS)
    for name, sig in parsed.items():
        fn = getattr(_lib.lib(), name)      # the library exports it ...
        assert _abi.ENERGY_SIGNATURES[name] == sig == (fn.restype, tuple(fn.argtypes)), name
    assert _lib.lib().ff_version() == _abi.ABI_VERSION == 110


def test_library_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from fermiflow_amd import _lib
    lib, p8 = _lib.lib(), C.c_void_p(8)

    def call(B=4, nup=3, ndn=3, d=2, Z=2.0, x=p8, grad=p8, lap=p8, ws=None, nstates=0, centre=None, parts=None, acc=p8, work=p8):
        st = lib.ff_energy_parts_accumulate(None, B, nup, ndn, d, Z, x, grad, lap, ws, nstates, centre, parts, acc, work)
        if st:
            assert lib.ff_last_error().decode().startswith("ff_energy_parts:"), lib.ff_last_error()
        return st
    # FF_EINVAL: null pointers, a negative size, no particle, Z not finite, nstates < 0, walker_state NULL with states
    for kw in (dict(x=None), dict(grad=None), dict(lap=None), dict(acc=None), dict(work=None), dict(B=-1), dict(nup=-1, ndn=4), dict(nup=3, ndn=-1),
               dict(nup=0, ndn=0), dict(d=0), dict(d=-3), dict(Z=float("nan")), dict(Z=float("inf")), dict(Z=-float("inf")), dict(nstates=-1),
               dict(nstates=3, ws=None)):
        assert call(**kw) == 1, kw
    # FF_EUNSUPPORTED: n > 24, n d > 60, d not 2 or 3, B >= 2^31, too many states
    for kw in (dict(nup=13, ndn=12), dict(nup=25, ndn=0), dict(nup=11, ndn=10, d=3), dict(d=1), dict(d=4), dict(B=1 << 31),
               dict(nstates=R.MAX_STATES + 1, ws=p8)):
        assert call(**kw) == 2, kw
    # B = 0 is a no-op, whatever the data pointers
    assert call(B=0, x=None, grad=None, lap=None, work=None) == 0 and call(B=0, nstates=3) == 0
    assert lib.ff_energy_parts_buffer_bytes(0) == 8 * 52 and lib.ff_energy_parts_buffer_bytes(5) == 8 * (52 + 40)
    assert lib.ff_energy_parts_buffer_bytes(-1) == 0 and lib.ff_energy_parts_buffer_bytes(R.MAX_STATES + 1) == 0
    assert lib.ff_energy_parts_workspace_bytes(65536, 0) == 8 * 28 * 256 and lib.ff_energy_parts_workspace_bytes(65536, 7) == 8 * (28 * 256 + 6 * 65536)
    assert lib.ff_energy_parts_workspace_bytes(0, 0) == 8 * 28 and lib.ff_energy_parts_workspace_bytes(1, 0) == 8 * 28
    assert lib.ff_energy_parts_workspace_bytes(1 << 31, 0) == 0 and lib.ff_energy_parts_workspace_bytes(-1, 0) == 0
    assert lib.ff_energy_parts_workspace_bytes(8, -1) == 0 and lib.ff_energy_parts_workspace_bytes(8, R.MAX_STATES + 1) == 0


def test_class_argument_checks():
    from fermiflow_amd import EnergyParts
    m = EnergyParts(3, 3, 2.0)
    assert (m.nup, m.ndown, m.Z, m.dim, m.nstates, m.centre) == (3, 3, 2.0, 2, 0, (0.0,) * 6)
    for kw in (dict(dim=1), dict(dim=4), dict(Z=float("nan")), dict(Z=float("inf")), dict(nstates=-1), dict(centre=[1.0] * 5),
               dict(centre=[float("nan")] + [0.0] * 5)):
        with pytest.raises(ValueError):
            EnergyParts(**{**dict(nup=3, ndown=3, Z=2.0), **kw})
    for nup, ndn in ((0, 0), (-1, 3), (3, -1)):
        with pytest.raises(ValueError):
            EnergyParts(nup, ndn, 2.0)
    for kw in (dict(nup=13, ndown=12), dict(nup=11, ndown=10, dim=3), dict(nstates=R.MAX_STATES + 1)):
        with pytest.raises(NotImplementedError):
            EnergyParts(**{**dict(nup=3, ndown=3, Z=2.0), **kw})
    z = torch.zeros(4, 6, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):          # no CPU path
        m.accumulate_raw(z, z, torch.zeros(4, dtype=torch.float64))
    assert m.counts() == (0, 0, 0) and m.counts().walkers == 0
    assert all(np.isnan(v) for v in m.block_errors().values()) and list(m.means()) == NAMES10 == list(m.errors()) == list(m.block_errors())
    assert np.isnan(EnergyParts(3, 3, 0.0).dE_dZ()[0])
    with pytest.raises(ValueError):
        m.per_state()


@pytest.mark.parametrize("centre", [None, [7.0, 6.5, 5.0, 1.0, 2.0, 0.5]])
def test_means_errors_and_covariance_of_known_tables(centre):
    """three calls of 50 walkers with hand-made components: every statistic against numpy on the tables themselves"""
    from fermiflow_amd import EnergyParts
    rng = np.random.default_rng(21)
    mix = rng.standard_normal((6, 6))
    calls = [rng.standard_normal((50, 6)) @ mix + np.array([7.0, 6.5, 5.0, 1.0, 2.0, 0.5]) for _ in range(3)]
    obj = EnergyParts(2, 2, 1.5, centre=centre)
    B = load(obj, calls, invalid=2)
    assert obj.counts() == (3, 150, 6) and obj._B == B == 52
    allc = np.concatenate(calls)
    combos = {**{k: np.eye(6)[i] for i, k in enumerate(R.NAMES)}, **{k: np.array(v, dtype=np.float64) for k, v in R.DERIVED.items()}}
    m, e, b = obj.means(), obj.errors(), obj.block_errors()
    cov = np.cov(allc.T, bias=True)
    assert np.abs(obj.cov() - cov).max() < 1e-11 and np.array_equal(obj.cov(), obj.cov().T)
    for name, a in combos.items():
        v = allc @ a
        assert abs(m[name] - v.mean()) < 1e-12 and abs(e[name] - v.std(ddof=0) / math.sqrt(149)) < 1e-11, name
    block_means = np.array([c.sum(0) for c in calls])
    want = block_means.std(0, ddof=1) / math.sqrt(3) / 50.0
    for k, name in enumerate(R.NAMES):
        assert abs(b[name] - want[k]) < 1e-11
    assert all(np.isnan(b[name]) for name in R.DERIVED)
    val, err = obj.dE_dZ()
    assert abs(val - m["V_ee"] / 1.5) < 1e-15 and abs(err - e["V_ee"] / 1.5) < 1e-15


def test_variances_clamp_at_zero():
    """equal walkers: the variance formula's difference may round below zero; the errors are 0, never NaN"""
    from fermiflow_amd import EnergyParts
    obj = EnergyParts(1, 1, 2.0)
    row = np.array([0.1, 0.7, 1.3, 0.0, 0.3, 0.0]) * math.pi
    load(obj, [np.tile(row, (37, 1))] * 2)
    e, b = obj.errors(), obj.block_errors()
    assert all(np.isfinite(v) and 0.0 <= v < 1e-7 for v in e.values())
    assert all(np.isfinite(b[k]) and 0.0 <= b[k] < 1e-7 for k in R.NAMES)


def test_per_state_table():
    from fermiflow_amd import EnergyParts
    rng = np.random.default_rng(5)
    calls = [rng.standard_normal((40, 6)) + 3.0 for _ in range(2)]
    state = [np.sort(rng.choice([0, 2, 3], 40)) for _ in range(2)]
    obj = EnergyParts(2, 1, 2.0, nstates=4, centre=[3.0] * 6)
    load(obj, calls, state=state)
    ps = obj.per_state()
    allc, alls = np.concatenate(calls), np.concatenate(state)
    assert np.array_equal(ps["count"], np.bincount(alls, minlength=4)) and ps["count"][1] == 0
    for s in (0, 2, 3):
        c = allc[alls == s]
        E = c[:, list(R.E_PARTS)].sum(1)
        assert abs(ps["E"][s] - E.mean()) < 1e-12 and abs(ps["E_err"][s] - E.std(ddof=0) / math.sqrt(len(E) - 1)) < 1e-11
        for k, name in enumerate(R.NAMES):
            assert abs(ps[name][s] - c[:, k].mean()) < 1e-12
    assert np.isnan(ps["E"][1]) and np.isnan(ps["E_err"][1])


def test_state_dict_round_trip_reset_and_npz(tmp_path):
    from fermiflow_amd import EnergyParts
    rng = np.random.default_rng(8)
    calls = [rng.standard_normal((20, 6)) + 2.0 for _ in range(4)]
    state = [np.sort(rng.integers(0, 3, 20)) for _ in range(4)]
    kw = dict(nup=2, ndown=1, Z=2.0, dim=3, nstates=3, centre=[2.0] * 6)
    obj = EnergyParts(**kw)
    load(obj, calls, invalid=1, state=state)
    st = obj.state_dict()
    other = EnergyParts(**kw)
    other.load_state_dict(st)
    assert torch.equal(other.state_dict()["acc"], st["acc"]) and other._B == 21 and other.counts() == obj.counts() == (4, 80, 4)
    for bad in (dict(Z=1.0), dict(dim=2), dict(nstates=0), dict(nup=1, ndown=2), dict(centre=None)):
        with pytest.raises(ValueError):
            EnergyParts(**{**kw, **bad}).load_state_dict(st)
    before = st["acc"].clone()
    obj.all_reduce_()                                                  # one process, no process group: the identity, bit for bit
    assert torch.equal(obj.state_dict()["acc"], before)
    out = str(tmp_path / "energy.npz")
    obj.save_npz(out)
    f = np.load(out)
    assert set(f.files) == {"names", "mean", "err", "block_err", "cov", "dE_dZ", "sum", "sum2", "blocksq", "calls", "walkers", "invalid", "centre",
                            "nup", "ndown", "Z", "dim", "nstates", "state_count", "state_E", "state_E_err", "state_mean", "state_sum", "state_sumE2"}
    assert list(f["names"]) == NAMES10 and f["mean"].shape == f["err"].shape == f["block_err"].shape == (10,)
    m = obj.means()
    assert np.array_equal(f["mean"], np.array([m[k] for k in NAMES10])) and np.array_equal(f["cov"], obj.cov())
    assert (int(f["calls"]), int(f["walkers"]), int(f["invalid"]), int(f["nstates"]), int(f["dim"]), float(f["Z"])) == (4, 80, 4, 3, 3, 2.0)
    assert f["state_mean"].shape == (3, 6) and np.array_equal(f["state_E"], obj.per_state()["E"])
    plain = EnergyParts(2, 1, 2.0)
    plain.save_npz(str(tmp_path / "plain.npz"))
    assert not any(k.startswith("state_") for k in np.load(str(tmp_path / "plain.npz")).files)
    other.reset()
    assert other.counts() == (0, 0, 0) and not other.state_dict()["acc"].any() and other._B is None


def test_all_reduce_refuses_inexact_counts():
    from fermiflow_amd import EnergyParts
    obj = EnergyParts(1, 1, 2.0)
    st = obj.state_dict()
    st["acc"][1] = 2 ** 53
    st["acc"][0] = 1
    obj.load_state_dict(st)
    with pytest.raises(OverflowError):
        obj.all_reduce_()


def test_sweeps_have_the_attribute_and_refuse_another_hamiltonian():
    import fermiflow_amd as ff
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=ff.MLP(1, 4)), (0.0, 1.0))
    m = ff.GSVMC(3, 3, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(2.0), sp_potential=ff.HO())
    assert m.energy_parts is None
    obj = ff.EnergyParts(3, 3, 2.0)
    m.energy_parts = obj
    assert m.energy_parts is obj
    assert not any("energy" in k for k in m.state_dict())      # a setting, not sweep state
    for bad in (ff.EnergyParts(3, 3, 1.0), ff.EnergyParts(2, 3, 2.0), ff.EnergyParts(3, 2, 2.0), ff.EnergyParts(3, 3, 2.0, dim=3),
                ff.EnergyParts(3, 3, 2.0, nstates=2)):
        with pytest.raises(ValueError):
            m.energy_parts = bad
    assert m.energy_parts is obj
    m.energy_parts = None

    from fermiflow_amd.potentials import PairPotential

    class Soft(PairPotential):
        def v(self, r):
            return 1.0 / (r + 0.1)
    for pair, sp in ((Soft(), ff.HO()), (ff.CoulombPairPotential(2.0), None)):
        other = ff.GSVMC(3, 3, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, pair, sp_potential=sp)
        with pytest.raises(ValueError):
            other.energy_parts = ff.EnergyParts(3, 3, 2.0)
    b = ff.BetaVMC(2.0, 2, 1, 2, True, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    assert b.energy_parts is None
    Ns = len(b.Es_original)
    b.energy_parts = ff.EnergyParts(2, 1, 0.5, nstates=Ns)
    b.energy_parts = ff.EnergyParts(2, 1, 0.5)                  # without per-state sums: fine too
    with pytest.raises(ValueError):
        b.energy_parts = ff.EnergyParts(2, 1, 0.5, nstates=Ns + 1)
    m3 = ff.GSVMC(2, 2, ff.HO3D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(2.0), sp_potential=ff.HO())
    m3.energy_parts = ff.EnergyParts(2, 2, 2.0, dim=3)
    with pytest.raises(ValueError):
        m3.energy_parts = ff.EnergyParts(2, 2, 2.0)


@pytest.mark.parametrize("driver", ["FermionHO2D", "BetaFermionHO2D"])
def test_driver_flag_and_line(driver):
    import importlib
    from fermiflow_amd import EnergyParts, frames
    mod = importlib.import_module("fermiflow_amd." + driver)
    p = mod.build_parser()
    assert p.parse_args([]).energy_out is None
    a = p.parse_args(["--energy_out", "e.npz"])
    assert a.energy_out == "e.npz"
    frames.check_arguments(p, a)
    obj = EnergyParts(1, 1, 2.0)
    load(obj, [np.tile(np.array([1.0, 1.25, 2.0, 0.0, 0.5, 0.0]), (8, 1))] * 2)
    line = frames.energy_line(obj)
    assert line.startswith("energy parts: E = 3.500000 +- ") and all(k in line for k in ("T = 1.000000", "V_trap = 2.000000", "V_ee = 0.500000",
                                                                                          "virial = -1.500000", "dT = -0.250000"))
