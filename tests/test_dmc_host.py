"""Host-side surface of fixed-node diffusion Monte Carlo (fermiflow_amd.DMC; include/fermiflow_dmc.h), no GPU needed: the sixth public
header against its ctypes table, the library's refusals, the class's argument checks, the driver's flags, and the restatement's own
sanity checks on wave functions whose answer is known -- no kernel runs here."""
import os
import re

import numpy as np
import pytest

from tests import dmc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sixth_header_is_plain_c99():
    import subprocess
    import tempfile
    src = ('#include "fermiflow_dmc.h"\n#include <stdio.h>\n'
           'int main(void) { printf("%d %d %d\\n", FF_DMC_REC, FF_DMC_CHUNK, FF_DMC_U_SLOT); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = tuple(int(v) for v in subprocess.check_output([exe]).split())
    from fermiflow_amd import _abi, native
    assert got == (_abi.DMC_REC, _abi.DMC_CHUNK, _abi.DMC_U_SLOT) == (R.REC, R.CHUNK, R.U_SLOT) == (9, 256, 64)
    assert native.DMC_REC == 9 and got[2] > 12          # (no quad of 24 particles reaches the uniform's slot)


def test_dmc_signature_table_is_the_sixth_header():
    """fermiflow_amd/_abi.py DMC_SIGNATURES against include/fermiflow_dmc.h, prototype by prototype (the method of
    tests/test_energy_parts_host.py), disjoint from the other five tables, and bind() has put the table on the library."""
    import ctypes as C
    from fermiflow_amd import _abi, _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fermiflow_dmc.h")).read(), flags=re.S)
    protos = re.findall(r"^(int|int64_t|size_t|const char\*)\s+(ff_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    assert [name for _, name, _ in protos] == re.findall(r"\b(ff_\w+)\s*\(", hdr) and len(protos) == 5
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "size_t": C.c_size_t,
             **dict.fromkeys(("const double*", "double*", "void*", "int32_t*", "uint8_t*"), C.c_void_p)}
    parsed = {}
    for ret, name, params in protos:
        spellings = [re.sub(r"\s*\*", "*", re.sub(r"\w+$", "", " ".join(p.split())).strip()) for p in params.split(",") if p.strip() != "void"]
        for t in [ret] + spellings:
            assert t in ctype, f"{name}: the C type {t!r} is not in this test's dictionary"
        parsed[name] = (ctype[ret], tuple(ctype[t] for t in spellings))
    assert list(parsed) == list(_abi.DMC_SIGNATURES)
    others = (set(_abi.SIGNATURES) | set(_abi.ROBUST_SIGNATURES) | set(_abi.MAPS_SIGNATURES) | set(_abi.OBDM_SIGNATURES) | set(_abi.ENERGY_SIGNATURES))
    assert not set(parsed) & others and not set(parsed) & set(_lib.SYMBOLS)
    for name, sig in parsed.items():
        fn = getattr(_lib.lib(), name)      # the library exports it ...
        assert _abi.DMC_SIGNATURES[name] == sig == (fn.restype, tuple(fn.argtypes)), name
    assert _lib.lib().ff_version() == _abi.ABI_VERSION == 110


def test_library_refuses_bad_arguments_before_any_launch():
    """Every pointer is the address 8: a launch would fault, a refusal returns."""
    import ctypes as C
    from fermiflow_amd import _lib
    lib, p8 = _lib.lib(), C.c_void_p(8)
    inf, nan = float("inf"), float("nan")

    def propose(B=4, nup=3, ndn=3, d=2, tau=0.01, a=1.0, x=p8, grad=p8, noise=None, seed=1, off=0, step=0, xn=p8, xi=None):
        return lib.ff_dmc_propose(None, B, nup, ndn, d, tau, a, x, grad, noise, seed, off, step, xn, xi)

    def accept(B=4, nup=3, ndn=3, d=2, tau=0.01, a=1.0, null=(), u=None, seed=1, off=0, step=0, slot=0, mask=None, groups=0):
        names = ("x", "logp", "grad", "eloc", "sign", "w", "x_new", "logp_new", "grad_new", "eloc_new", "sign_new")
        ptrs = [None if k in null else p8 for k in names]
        tail = {k: (None if k in null else p8) for k in ("ctrl", "rec", "workspace")}
        return lib.ff_dmc_accept(None, B, nup, ndn, d, tau, a, *ptrs, u, seed, off, step, tail["ctrl"], tail["rec"], slot, mask, groups,
                                 tail["workspace"])

    def comb(B=4, nup=3, ndn=3, d=2, null=(), u0=None, seed=1, step=0):
        names = ("w", "x", "logp", "grad", "eloc", "sign")
        outs = ("src", "x_out", "logp_out", "grad_out", "eloc_out", "sign_out", "info", "workspace")
        return lib.ff_dmc_comb(None, B, nup, ndn, d, *[None if k in null else p8 for k in names], u0, seed, step,
                               *[None if k in null else p8 for k in outs])
    common_inval = (dict(B=-1), dict(nup=-1, ndn=4), dict(nup=3, ndn=-1), dict(nup=0, ndn=0), dict(d=0), dict(d=-2), dict(step=-1), dict(step=1 << 32))
    common_unsup = (dict(d=3), dict(d=1), dict(nup=13, ndn=12), dict(nup=13, ndn=0), dict(nup=0, ndn=13), dict(B=1 << 31))
    step_kinds = (dict(tau=0.0), dict(tau=-0.1), dict(tau=nan), dict(tau=inf), dict(a=-1.0), dict(a=nan), dict(a=inf), dict(off=-1))
    cases = [(propose, 1, kw) for kw in common_inval + step_kinds + (dict(x=None), dict(grad=None), dict(xn=None))]
    cases += [(propose, 2, kw) for kw in common_unsup]
    cases += [(accept, 1, kw) for kw in common_inval + step_kinds + (dict(slot=-1), dict(groups=-1), dict(groups=65537))]
    cases += [(accept, 1, dict(null=(k,))) for k in ("x", "logp", "grad", "eloc", "sign", "w", "x_new", "logp_new", "grad_new", "eloc_new",
                                                     "sign_new", "ctrl", "rec", "workspace")]
    cases += [(accept, 2, kw) for kw in common_unsup]
    cases += [(comb, 1, kw) for kw in common_inval]
    cases += [(comb, 1, dict(null=(k,))) for k in ("w", "x", "logp", "grad", "eloc", "sign", "src", "x_out", "logp_out", "grad_out", "eloc_out",
                                                   "sign_out", "info", "workspace")]
    cases += [(comb, 2, kw) for kw in common_unsup]
    for fn, status, kw in cases:
        assert fn(**kw) == status, (fn.__name__, kw)
        assert lib.ff_last_error().decode().startswith("ff_dmc:"), lib.ff_last_error()
    # B = 0 is a no-op, whatever the data pointers
    assert propose(B=0, x=None, grad=None, xn=None) == 0
    assert accept(B=0, null=("x", "logp", "w", "ctrl", "rec", "workspace")) == 0
    assert comb(B=0, null=("w", "x", "src", "info", "workspace")) == 0
    assert lib.ff_dmc_accept_workspace_bytes(0) == 8 * 10 and lib.ff_dmc_accept_workspace_bytes(257) == 8 * 19
    assert lib.ff_dmc_accept_workspace_bytes(65536) == 8 * (1 + 9 * 256)
    assert lib.ff_dmc_comb_workspace_bytes(0) == 8 * 7 and lib.ff_dmc_comb_workspace_bytes(257) == 8 * (4 + 257 + 6)
    for f in (lib.ff_dmc_accept_workspace_bytes, lib.ff_dmc_comb_workspace_bytes):
        assert f(-1) == 0 and f(1 << 31) == 0


def _gsvmc(ff, dim=2):
    import torch  # noqa: F401
    eta, mu = ff.MLP(1, 6), ff.MLP(1, 6)
    eta.init_gaussian(1); mu.init_gaussian(2)
    cnf = ff.CNF(ff.Backflow(eta, mu=mu), (0.0, 1.0))
    orb = ff.HO2D() if dim == 2 else ff.HO3D()
    return ff.GSVMC(3, 3, orb, ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(2.0), sp_potential=ff.HO()), cnf


def test_class_argument_checks(monkeypatch):
    import fermiflow_amd as ff
    from fermiflow_amd import dmc as M
    model, cnf = _gsvmc(ff)
    d = ff.DMC(model)
    assert (d.tau, d.steps_per_block, d.drift_limit, d.ecut, d.comb, d.observables, d.density_maps) == (0.01, 50, 1.0, 0.2, True, None, None)
    b = ff.BetaVMC(2.0, 2, 1, 2, True, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    with pytest.raises(ValueError, match="BetaVMC"):
        ff.DMC(b)
    with pytest.raises(ValueError, match="two dimensions"):
        ff.DMC(_gsvmc(ff, dim=3)[0])
    with pytest.raises(ValueError, match="GSVMC"):
        ff.DMC(object())
    for kw in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(drift_limit=-0.5), dict(drift_limit=float("nan")),
               dict(ecut=0.0), dict(ecut=float("inf")), dict(steps_per_block=0), dict(observe_every=0)):
        with pytest.raises(ValueError):
            ff.DMC(model, **kw)
    with pytest.raises(RuntimeError, match="start"):
        d.run(1)
    with pytest.raises(ValueError):
        d.start(0)
    monkeypatch.setattr(M.D, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="one rank"):
        ff.DMC(model)


def test_driver_flags():
    from fermiflow_amd import FermionHO2D as F
    from fermiflow_amd.dmc import RESULT_KEYS
    a = F.build_parser().parse_args([])
    assert (a.dmc_blocks, a.dmc_tau, a.dmc_steps, a.dmc_equil, a.dmc_out) == (0, 0.01, 50, 2, None)
    a = F.build_parser().parse_args("--dmc_blocks 20 --dmc_tau 0.005 --dmc_steps 40 --dmc_equil 4 --dmc_out e.npz".split())
    assert (a.dmc_blocks, a.dmc_tau, a.dmc_steps, a.dmc_equil, a.dmc_out) == (20, 0.005, 40, 4, "e.npz")
    for bad in ("--dmc_blocks -1", "--dmc_blocks 2 --dmc_tau 0", "--dmc_blocks 2 --dmc_steps 0", "--dmc_blocks 2 --dim 3"):
        with pytest.raises(SystemExit):
            F.main(bad.split())
    assert set(RESULT_KEYS) >= {"E", "E_err", "E_vmc", "acceptance", "crossing", "invalid", "esf", "distinct", "blocks"}


# ---- the restatement's own sanity
def test_philox_restatement_matches_the_published_vectors():
    """Philox4x32-10 known-answer vectors (Random123 kat_vectors): counter and key all zero, and all ones"""
    z = R.philox(0, 0, 0, 0)
    assert [int(v[0]) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    o = R.philox(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v[0]) for v in o] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_reference_known_answer_three_plus_three():
    """Zero flow, Z = 0, 3 + 3: the guide is the exact ground state, E_loc = 10 for every walker -- every step's record gives E = 10,
    every weight stays equal (E_T = 10: exactly 1 up to the rounding of E_loc), nothing is invalid."""
    rng = np.random.default_rng(4)
    x0 = rng.standard_normal((256, 6, 2)) * np.sqrt(0.5)
    g = R.three_plus_three(x0)
    np.testing.assert_allclose(g["eloc"], 10.0, rtol=0, atol=1e-9)
    # the closed-form gradient against a central difference of the closed-form log p
    h = 1e-6
    for (i, k) in ((0, 0), (4, 1)):
        xp, xm = x0.copy(), x0.copy()
        xp[:, i, k] += h; xm[:, i, k] -= h
        fd = (R.three_plus_three(xp)["logp"] - R.three_plus_three(xm)["logp"]) / (2 * h)
        np.testing.assert_allclose(g["grad"][:, i, k], fd, rtol=1e-5, atol=1e-5)
    trace = []
    r = R.run(R.three_plus_three, x0, 0.02, 2, 10, seed=9, trace=trace)
    E = np.array([t[1] / t[0] for t in trace])
    assert len(E) == 20 and np.abs(E - 10.0).max() < 1e-9 and abs(r["E"] - 10.0) < 1e-9
    assert r["invalid"] == 0 and r["acceptance"] > 0.9 and r["esf"] > 1 - 1e-12 and 0 < r["crossing"] < 0.05


def test_reference_detailed_balance_without_the_comb():
    """With the comb off the accept step is a Metropolis chain in |psi|^2: <sum r^2> = 10 for the six free fermions (the virial value),
    within 4 standard errors over the final walkers of 200 steps from |psi|^2-ish starts."""
    rng = np.random.default_rng(12)
    x0 = rng.standard_normal((2048, 6, 2)) * np.sqrt(0.8)
    r = R.run(R.three_plus_three, x0, 0.05, 4, 50, seed=3, comb_on=False)
    r2 = (r["walkers"] ** 2).sum((1, 2))
    assert abs(r2.mean() - 10.0) < 4 * r2.std(ddof=1) / np.sqrt(len(r2)), (r2.mean(), r2.std())
