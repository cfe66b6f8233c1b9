"""Host-side logic and the C-ABI surface, no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from fermiflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fermiflow.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|size_t|const char\*)\s+(ff_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 20
    lib = _lib.lib()          # loads without a GPU (links against libamdhip64 only)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert declared == set(_lib.SYMBOLS)
    from fermiflow_amd import _abi
    assert declared == set(_abi.SIGNATURES) and _lib.SYMBOLS == list(_abi.SIGNATURES)
    from fermiflow_amd import _lib as L
    assert lib.ff_version() == L.ABI_VERSION


def test_header_is_plain_c_and_matches_the_ctypes_structs():
    """include/fermiflow.h compiles as C99 on its own (the boundary is a C ABI), and the ctypes mirrors of ff_net /
    ff_ode have the sizes the C compiler gives the structs."""
    import ctypes as C
    import subprocess
    import tempfile
    from fermiflow_amd import _lib
    src = '#include "fermiflow.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu\\n", sizeof(ff_net), sizeof(ff_ode)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        net_sz, ode_sz = (int(v) for v in subprocess.check_output([exe]).split())
    assert net_sz == C.sizeof(_lib.FFNet) and ode_sz == C.sizeof(_lib.FFOde)


def test_abi_argument_errors_without_gpu():
    """invalid arguments are rejected before any launch (status 1 / 2), so this runs on CPU."""
    import ctypes as C
    from fermiflow_amd import _lib
    lib = _lib.lib()
    assert lib.ff_potential(None, C.c_int64(4), 0, 2, C.c_double(1.0), 1, None, None) == 1
    assert lib.ff_slater_logabsdet_fwd(None, C.c_int64(4), 99, C.c_void_p(8), None, C.c_void_p(8), C.c_void_p(8)) == 2
    assert b"FF_MAX_NS" in lib.ff_last_error()
    net = _lib.FFNet(50, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 0, None, None, None)
    ode = _lib.FFOde(0.0, 1.0, 1e-6, 1e-8, 0)
    # (n, d) beyond the fused kernels (n <= 24, n d <= 60) -> 2; negative tolerance -> 1
    assert lib.ff_cnf_generate(None, C.c_int64(4), 25, 2, C.byref(net), C.byref(ode), C.c_void_p(8), C.c_void_p(8), None) == 2
    assert lib.ff_cnf_generate(None, C.c_int64(4), 21, 3, C.byref(net), C.byref(ode), C.c_void_p(8), C.c_void_p(8), None) == 2
    assert lib.ff_cnf_adjoint_workspace_bytes(C.c_int64(4), 20, 3, 50, 50) > 0      # BASELINE configs[4]: one walker per wave
    wide = _lib.FFNet(300, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 0, None, None, None)      # hidden width > 256
    assert lib.ff_cnf_generate(None, C.c_int64(4), 6, 2, C.byref(wide), C.byref(ode), C.c_void_p(8), C.c_void_p(8), None) == 2
    bad = _lib.FFOde(0.0, 1.0, -1.0, 1e-8, 0)
    assert lib.ff_cnf_generate(None, C.c_int64(4), 6, 2, C.byref(net), C.byref(bad), C.c_void_p(8), C.c_void_p(8), None) == 1
    # round-2 entry points: empty batches, null pointers and out-of-range arguments
    p8 = C.c_void_p(8)
    assert lib.ff_reduce_energy(None, C.c_int64(0), p8, p8, p8, p8) == 1
    assert lib.ff_reduce_energy(None, C.c_int64(4), p8, None, p8, p8) == 1
    assert lib.ff_energy_finish(None, p8, p8, C.c_int64(0), p8) == 1
    assert lib.ff_stream_delay(None, C.c_double(-1.0)) == 1 and lib.ff_stream_delay(None, C.c_double(1e9)) == 1
    assert lib.ff_cnf_adjoint_energy(None, C.c_int64(4), 6, 2, C.byref(net), C.byref(ode), p8, p8, None, p8, None, C.c_double(0.25),
                                     None, p8, p8, None) == 1                       # eloc missing
    assert lib.ff_cnf_adjoint(None, C.c_int64(4), 6, 2, C.byref(net), C.byref(ode), p8, p8, None, None, p8, p8, None) == 1   # a_d missing


def test_signature_table_is_the_header():
    """fermiflow_amd/_abi.py SIGNATURES against include/fermiflow.h, prototype by prototype, through a dictionary of C spellings
    written out HERE: a parameter type the header starts to use fails by name until it is added on purpose."""
    import ctypes as C
    from fermiflow_amd import _abi, _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fermiflow.h")).read(), flags=re.S)
    protos = re.findall(r"^(int|int64_t|size_t|const char\*)\s+(ff_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    assert [name for _, name, _ in protos] == re.findall(r"\b(ff_\w+)\s*\(", hdr) and len(protos) == 69      # no prototype the pattern misses
    data = ("const double*", "double*", "const int32_t*", "int32_t*", "const int64_t*", "uint8_t*", "void*", "const void*",
            "ff_comm*", "ff_comm**", "double* const*", "const double* const*")
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "size_t": C.c_size_t,
             "const char*": C.c_char_p, "const ff_net*": C.POINTER(_abi.FFNet), "const ff_ode*": C.POINTER(_abi.FFOde),
             "ff_kernel_plan_info*": C.POINTER(_abi.FFKernelPlanInfo), **dict.fromkeys(data, C.c_void_p)}
    parsed = {}
    for ret, name, params in protos:
        spellings = [re.sub(r"\s*\*", "*", re.sub(r"\w+$", "", " ".join(p.split())).strip()) for p in params.split(",") if p.strip() != "void"]
        for t in [ret] + spellings:
            assert t in ctype, f"{name}: the C type {t!r} is not in this test's dictionary"
        parsed[name] = (ctype[ret], tuple(ctype[t] for t in spellings))
    assert list(parsed) == list(_abi.SIGNATURES)      # the header's order
    for name, sig in parsed.items():      # ... and bind() has put it on the library
        assert _abi.SIGNATURES[name] == sig == (getattr(_lib.lib(), name).restype, tuple(getattr(_lib.lib(), name).argtypes)), name


def test_typed_calls_take_plain_numbers_and_refuse_wrong_types():
    """With argtypes set, plain Python numbers reach the library as the C types of the header, and a wrong type is an error of the
    call instead of a silent 32-bit int.  No GPU: every call is refused before any launch."""
    import ctypes as C
    from fermiflow_amd import _abi, _lib
    lib = _lib.lib()
    assert lib.ff_potential(None, 4, 0, 2, 1.0, 1, None, None) == 1
    for bad in ("4", 4.0):      # int64_t B
        with pytest.raises(C.ArgumentError):
            lib.ff_potential(None, bad, 0, 2, 1.0, 1, None, None)
    with pytest.raises(C.ArgumentError):      # const ff_net*: another struct
        lib.ff_backflow_v_div(None, 4, 6, 2, C.byref(_abi.FFOde()), None, None, None)
    assert lib.ff_backflow_v_div(None, 4, 6, 2, C.byref(_abi.FFNet()), None, None, None) == 1
    with pytest.raises(TypeError):      # FFOde by field name: all of them, no others
        _abi.ode_struct(t0=0.0, t1=1.0)
    # a size past 2^32 comes back whole (configs[4]); csrc/ff_eloc_ws.h: z(t0) (B,M) | Jt (B,M,M) | kbar, dDelta, lap parts (B,M) each |
    # Delta (B) | Slater table (B, nq) | 2 counters, nq = M + d (d + 1) / 2 n + d n^2 + 2
    B, n, d, M = 131072, 20, 3, 60
    doubles = B * (M * M + 4 * M + 1 + (M + d * (d + 1) // 2 * n + d * n * n + 2)) + 2
    assert lib.ff_eloc_workspace_bytes(B, n, d) == 8 * doubles > 2**32


def test_signatures_and_struct_mirrors_are_declared_in_one_place():
    """No restype / argtypes assignment and no ctypes mirror of ff_net / ff_ode outside fermiflow_amd/_abi.py, in the package, the tests
    and the tools: a second declaration is one that can be forgotten."""
    found = {}
    for top in ("fermiflow_amd", "tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for path in (os.path.join(dirpath, f) for f in files if f.endswith(".py")):
                src = open(path).read()
                hits = re.findall(r"\.(?:restype|argtypes)\b[^=\n]*=(?!=)", src) + [
                    m for m in re.findall(r"^class\s+\w+\s*\([^)]*Structure[^)]*\)\s*:.*?(?=^\S|\Z)", src, flags=re.S | re.M)
                    if re.search(r"\b(ew1|walker_cost)\b", m)]
                if hits:
                    found[os.path.relpath(path, ROOT)] = hits
    assert list(found) == [os.path.join("fermiflow_amd", "_abi.py")] and len(found[os.path.join("fermiflow_amd", "_abi.py")]) == 3, found


def test_no_cpu_fallback():
    import fermiflow_amd as ff
    x = torch.randn(4, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ff.HO().V(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ff.LogAbsSlaterDet.apply(tuple(ff.HO2D().orbitals[:3]), x)


def test_orbitals_and_state_enumeration(golden):
    import fermiflow_amd as ff
    G = golden["g2_slater"]
    h = ff.HO2D()
    assert len(h.orbitals) == 36 and h.Es == list(G["orb_Es"])
    pts = torch.tensor(G["orb_pts"])
    v = np.stack([o(pts).numpy() for o in h.orbitals])
    np.testing.assert_allclose(v, G["orb_vals"], rtol=1e-13, atol=1e-15)
    for N, dE in ((3, 2), (4, 2), (6, 4), (10, 3)):
        for de in range(dE + 1):
            s, e = h.fermion_states(N, 0, de)
            idx = np.array([[o.k for o in t[0]] for t in s])
            assert (idx == G[f"enum_N{N}_dE{de}_idx"]).all()
            assert (np.array(e) == G[f"enum_N{N}_dE{de}_E"]).all()
            ip, ep = h.subsets(N, sum(h.Es[:N]) + de, h.Es)      # the Python restatement of src/orbitals.py:14-31
            assert [tuple(r) for r in idx.tolist()] == list(ip) and list(e) == list(ep)
    assert len(h.fermion_states(3, 0, 2.0)[0]) == 21          # config 3 of BASELINE.json
    assert len(h.fermion_states(10, 0, 4)[0]) == 1781
    # two spin species (the reference raises here, src/orbitals.py:47-49): pairs of subsets within deltaE
    # of the ground state, by total energy, ties in (up, down)-lexicographic order
    s, e = h.fermion_states(2, 1, 1.0)
    got = [(tuple(o.k for o in a), tuple(o.k for o in b), E) for (a, b), E in zip(s, e)]
    assert got == [((0, 1), (0,), 4), ((0, 2), (0,), 4), ((0, 1), (1,), 5), ((0, 1), (2,), 5), ((0, 2), (1,), 5),
                   ((0, 2), (2,), 5), ((0, 3), (0,), 5), ((0, 4), (0,), 5), ((0, 5), (0,), 5), ((1, 2), (0,), 5)]
    s, e = h.fermion_states(3, 3, 2.0)
    assert len(s) == 77 and e[0] == 10 and e[-1] == 12 and list(e) == sorted(e)
    # brute force over all subset pairs gives the same set
    import itertools
    brute = {(u, d) for u in itertools.combinations(range(10), 3) for d in itertools.combinations(range(10), 3)
             if sum(h.Es[i] for i in u) + sum(h.Es[i] for i in d) <= 12}
    assert {(tuple(o.k for o in a), tuple(o.k for o in b)) for a, b in s} == brute
    with pytest.raises(ValueError):
        h.fermion_states(0, 0, 2.0)


def test_reference_error_behaviour():
    import fermiflow_amd as ff
    from fermiflow_amd.NeuralODE.nnModule import solve_ivp_nnmodule
    with pytest.raises(ValueError):                                # src/NeuralODE/nnModule.py:164-165
        solve_ivp_nnmodule(lambda t, x: x, (0.0, 1.0), torch.zeros(2, 3, 2))
    bd = ff.FreeFermion()
    states, _ = ff.HO2D().fermion_states(3, 0, 1.0)
    with pytest.raises(ValueError):                                # src/base_dist.py:74-76
        bd.log_prob_multstates(states, {0: 2}, torch.zeros(2, 1, 3, 2))
    with pytest.raises(ValueError):                                # src/base_dist.py:104-106
        bd.sample_multstates(states, {0: 2}, (1, 2))
    m = ff.MLP(1, 50)
    assert [n for n, _ in m.named_parameters()] == ["fc1.weight", "fc1.bias", "fc2.weight"]
    assert [tuple(p.shape) for p in m.parameters()] == [(50, 1), (50,), (1, 50)]
    m.init_zeros()
    assert all((p == 0).all() for p in m.parameters())


def test_shard_partition():
    from fermiflow_amd import dist as D
    for B in (1, 7, 65536, 65537, 262144):
        for W in (1, 2, 3, 8):
            parts = [D.shard(B, r, W) for r in range(W)]
            assert sum(c for _, c in parts) == B
            off = 0
            for o, c in parts:
                assert o == off
                off += c
            assert max(c for _, c in parts) - min(c for _, c in parts) <= 1


def test_no_agpr_copy_in_front_of_an_exec_restore():
    """Static check of the BUILT library (tools/check_agpr_spills.py): ROCm 7.2's register allocator can place a VGPR->AGPR
    copy in front of the `s_or_b64 exec` of a join block, where it runs under the mask of the branch that just ended --
    with exec = 0 when no lane took it (an optional ff_ode array that is NULL).  That was an aperture violation at run time
    for ff_ode_fwd_kernel<2,2,2> (docs/LOG.md, round 2); the kernels read optional inputs without a branch since, and this test keeps
    the pattern from coming back unnoticed with the next change of register pressure."""
    import importlib.util, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "fermiflow_amd", "libfermiflow_hip.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("library or llvm-objdump not present")
    spec = importlib.util.spec_from_file_location("check_agpr_spills", os.path.join(root, "tools", "check_agpr_spills.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    funcs = mod.parse_library(lib)
    assert len(funcs) > 100
    wrong = {k: [h for h in mod.masked_prologue_writes(v) if not h[2].startswith("harmless")] for k, v in funcs.items()}
    wrong = {k: v for k, v in wrong.items() if v}
    assert not wrong, wrong


def test_plain_parameter_state_dict_loads_as_a_cold_sweep_state():
    """weights trained with the reference (or another model's state_dict) carry no "_extra_state"; strict loading
    must accept them -- the sweep state (warm start, reduction shifts, prefetched walkers) then simply starts cold."""
    import torch
    import fermiflow_amd as ff

    def build():
        eta, mu = ff.MLP(1, 6), ff.MLP(1, 6)
        eta.init_gaussian(1); mu.init_gaussian(2)
        return ff.GSVMC(3, 3, ff.HO2D(), ff.FreeFermion(), ff.CNF(ff.Backflow(eta, mu=mu), (0.0, 1.0)), ff.CoulombPairPotential(2.0),
                        sp_potential=ff.HO())
    a, b = build(), build()
    with torch.no_grad():
        for p in a.parameters():
            p.mul_(3.0)
    bare = {k: v for k, v in a.state_dict().items() if not k.endswith("_extra_state")}
    assert len(bare) == len(a.state_dict()) - 1 and "_extra_state" in a.state_dict()
    b._h_flow = torch.ones(1)
    b.load_state_dict(bare)          # strict
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert b._h_flow is None and b._dev == {}
    assert "_extra_state" not in bare
    b.load_state_dict(a.state_dict())      # and the full one still loads


def test_potentials_are_never_silently_reinterpreted():
    """VMC.potential_plan: the stock CoulombPairPotential(Z) / HO() are fused into the native finish; any
    other pair or trap potential keeps the reference's generic semantics (its own V(x) is called, src/VMC.py:51-53) instead of
    being treated as Z = 0 / as a harmonic trap; an object without V raises."""
    import fermiflow_amd as ff
    from fermiflow_amd.VMC import potential_plan
    from fermiflow_amd.potentials import PairPotential, SPPotential
    assert potential_plan(ff.CoulombPairPotential(2.0), ff.HO()) == (2.0, True, [])
    assert potential_plan(ff.CoulombPairPotential(0.5), None) == (0.5, False, [])

    class Yukawa(PairPotential):
        def v(self, rij):
            return torch.exp(-rij) / rij

    class Quartic(SPPotential):
        def V(self, x):
            return (x ** 4).sum(dim=(-2, -1))

    class ScreenedCoulomb(ff.CoulombPairPotential):      # a SUBCLASS may override v(): not the stock formula any more
        def v(self, rij):
            return self.Z / (rij + 1.0)

    y, q, s = Yukawa(), Quartic(), ScreenedCoulomb(2.0)
    assert potential_plan(y, ff.HO()) == (0.0, True, [y])
    assert potential_plan(ff.CoulombPairPotential(2.0), q) == (2.0, False, [q])
    assert potential_plan(s, q) == (0.0, False, [s, q])
    # the generic pair potential's V(x) is the reference's formula (sum over i < j of v(r_ij))
    x = torch.randn(5, 4, 2, dtype=torch.float64)
    want = sum(torch.exp(-(x[:, i] - x[:, j]).norm(dim=-1)) / (x[:, i] - x[:, j]).norm(dim=-1) for i in range(4) for j in range(i + 1, 4))
    assert torch.allclose(y.V(x), want)
    with pytest.raises(TypeError):
        potential_plan(object(), ff.HO())
    with pytest.raises(TypeError):
        potential_plan(None, ff.HO())
    with pytest.raises(TypeError):
        potential_plan(ff.CoulombPairPotential(1.0), SPPotential())


def test_routing_controls_travel_in_ff_ode_not_in_the_environment():
    """heavy_class / heavy_tol / sum_weight are ff_ode fields (ABI 103): two callers in one process can choose differently, and the
    library's sources read no accuracy knob from the environment (the remaining getenv calls select kernels for A/B timing)."""
    from fermiflow_amd import _lib
    o = _lib.ode(0.0, 1.0, 1e-6, 1e-8, heavy_class=-1, heavy_tol=0.1, sum_weight=16.0)
    assert (o.heavy_class, o.heavy_tol, o.sum_weight) == (-1, 0.1, 16.0)
    o = _lib.ode(0.0, 1.0, 1e-6, 1e-8)
    assert (o.heavy_class, o.heavy_tol, o.sum_weight) == (0, 0.0, 0.0)
    csrc = os.path.join(ROOT, "fermiflow_amd", "csrc")
    envs = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".inc")):
            envs |= set(re.findall(r'getenv\("(\w+)"\)', open(os.path.join(csrc, f)).read()))
    assert not {e for e in envs if "TOL" in e or "HEAVY" in e or "SUMW" in e or "WEIGHT" in e}, envs
    assert _lib.lib().ff_shutdown() == 0          # nothing created yet: a no-op, and callable without a GPU


def test_environment_knobs_are_the_documented_dozen():
    """the A/B knobs of closed experiments are gone -- what the package and the library still read from the environment
    is exactly the table of INTEGRATION.md section 2 (FF_STATS_WORDS: diagnostic builds only; WORLD_SIZE & co.: the launcher's)."""
    pkg = os.path.join(ROOT, "fermiflow_amd")
    found = set()
    for d, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".inc")):
                t = open(os.path.join(d, f)).read()
                found |= set(re.findall(r'getenv\("(\w+)"\)', t)) | set(re.findall(r'environ(?:\.get|\.setdefault)?\(\s*"(\w+)"', t))
    found -= {"WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FF_STATS_WORDS"}
    documented = set(re.findall(r"^\| `((?:FERMIFLOW|FF)_[A-Z_]+)` \|", open(os.path.join(ROOT, "INTEGRATION.md")).read(), flags=re.M))
    assert found == documented and len(found) == 12, (sorted(found - documented), sorted(documented - found))


def test_reference_state_draw_reproduces_the_reference(golden):
    """VERDICT r05 missing #3: BetaVMC.state_draw = "reference" draws the many-body states as the reference does (src/VMC.py:90-96) -- after
    the same torch.manual_seed the Counter of sorted state indices is the one the reference's seeded forward produced (g6_betavmc.npz:
    keys / counts of three cases, captured by tests/golden/make_golden.py)."""
    from collections import Counter
    from fermiflow_amd.VMC import draw_states_reference
    G = golden["g6_betavmc"]
    for tag in ("boltz", "hot", "rand"):
        nup, B, seed = (int(v) for v in G[f"{tag}_cfg"])
        torch.manual_seed(seed)
        idx = draw_states_reference(torch.tensor(G[f"{tag}_logits"]), B)
        assert idx.dtype == torch.int64 and idx.shape == (B,) and bool((idx[1:] >= idx[:-1]).all())
        got = Counter(idx.tolist())
        assert list(got.keys()) == [int(k) for k in G[f"{tag}_keys"]] and list(got.values()) == [int(c) for c in G[f"{tag}_counts"]], tag


def test_fused_adam_refuses_what_it_does_not_implement():
    """FusedAdam.load_state_dict copies torch.optim.Adam's param_groups -- a state saved with amsgrad or maximize must not be
    continued as plain Adam (no GPU needed: the refusal happens before any launch)."""
    from fermiflow_amd.utils import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    for kw in ({"amsgrad": True}, {"maximize": True}):
        ref = torch.optim.Adam([p], lr=1e-2, **kw)
        p.grad = torch.ones_like(p)
        ref.step()
        with pytest.raises(RuntimeError):
            FusedAdam([p], lr=1e-2).load_state_dict(ref.state_dict())
    ok = torch.optim.Adam([p], lr=1e-2)
    ok.step()
    opt = FusedAdam([p], lr=1e-2)
    opt.load_state_dict(ok.state_dict())
    with pytest.raises(RuntimeError):      # a CPU parameter: refused by step(), and its step count stays where the state dict left it
        opt.step()
    assert float(opt.state[p]["step"]) == 1.0


def test_adjoint_workspace_serves_either_kernel_family():
    """ff_cnf_adjoint_workspace_bytes no longer depends on the mutable kernel family -- the size is the larger of the two
    layouts, so a family switch between the query and the call cannot overrun the caller's buffer."""
    from fermiflow_amd import _lib
    import ctypes as C
    lib = _lib.lib()
    q = lambda: lib.ff_cnf_adjoint_workspace_bytes(C.c_int64(4096), 6, 2, 50, 50)
    prev = lib.ff_set_kernel_family(0)
    try:
        a = q()
        lib.ff_set_kernel_family(1)
        b = q()
    finally:
        lib.ff_set_kernel_family(prev)
    assert a == b and a > 0


def test_compact_finish_workspace_sizes():
    """ff_ode.compact_finish (ABI 104): beyond 24 coordinates the workspace of ff_eloc_nd is z(t0) | Delta | two counters and nothing of
    size (n d)^2; up to 24 coordinates -- where kernels without a fused finish may serve a walker -- the full layout either way; the
    binding asks for it by itself only past COMPACT_WORKSPACE_BYTES of full workspace."""
    import ctypes as C
    from fermiflow_amd import _lib, native
    lib = _lib.lib()
    assert lib.ff_version() == _lib.ABI_VERSION >= 104
    assert C.sizeof(_lib.FFOde) % 8 == 0 and [f[0] for f in _lib.FFOde._fields_[-3:]] == ["compact_finish", "after_main_event", "walker_h_equal"]
    full = lambda B, n, d: lib.ff_eloc_workspace_bytes(C.c_int64(B), n, d)
    nd = lambda B, n, d, c: lib.ff_eloc_nd_workspace_bytes(C.c_int64(B), n, d, c)
    for (n, d) in ((6, 2), (12, 2), (8, 3)):                 # M <= 24
        assert nd(1000, n, d, 0) == full(1000, n, d) == nd(1000, n, d, 1)
    for (n, d) in ((13, 2), (24, 2), (20, 3)):               # M > 24
        M = n * d
        assert nd(1000, n, d, 0) == full(1000, n, d)
        assert nd(1000, n, d, 1) == 8 * (1000 * (M + 1) + 2)
    # configs[4]: 131 072 walkers of 20 particles in d = 3 -- 4.09 GB of J^T alone in the full layout, 64 MB compact
    assert full(131072, 20, 3) > 4.0e9 and nd(131072, 20, 3, 1) == 8 * (131072 * 61 + 2) < 64.1e6
    assert native.COMPACT_WORKSPACE_BYTES == 32 << 30 and full(1 << 20, 20, 3) > native.COMPACT_WORKSPACE_BYTES > full(1 << 19, 20, 3)


def test_stiff_regimes_cover_every_grid_row_length_and_refusal():
    """The weight regimes of tests/test_gpu_stiff_weights.py, through the header rule of ff_radial.h restated (tests/common.py
    radial_header): the narrow shapes meet every grid spacing, every deposit row length and both refusals; the wide and 3-D shapes the
    12-row, h = 1/128, deposit-refused, h = 1/512 and table-refused regimes.  A threshold change in the restatement that shrank this
    matrix fails here; the GPU node test asserts the device's header equals the restatement."""
    from tests.common import STIFF_BROAD_REGIMES, STIFF_NARROW_REGIMES, STIFF_REGIMES, radial_header, stiff_net
    hdr = {r: radial_header(STIFF_REGIMES[r][0]) for r in STIFF_REGIMES}
    usable = [hdr[r] for r in STIFF_NARROW_REGIMES if not hdr[r][3]]
    assert {h[0] for h in usable} == {64.0, 128.0, 256.0, 512.0}
    assert {h[5] for h in usable if not h[4]} == {6.0, 8.0, 10.0, 12.0}
    assert any(hdr[r][3] for r in STIFF_NARROW_REGIMES) and any(hdr[r][4] and not hdr[r][3] for r in STIFF_NARROW_REGIMES)
    broad = [hdr[r] for r in STIFF_BROAD_REGIMES]
    assert any(h[5] == 12 and h[0] == 64 and not h[4] for h in broad) and any(h[0] == 128 and not h[4] for h in broad)
    assert any(h[0] == 512 and not h[3] for h in broad)
    assert any(h[3] for h in broad) and any(h[4] and not h[3] for h in broad)
    assert STIFF_REGIMES["w5mu"][1] == "mu"
    for r, (target, stiff) in STIFF_REGIMES.items():        # the generator hits the target exactly, in the net it names
        eta, mu = stiff_net(target, stiff=stiff)
        top = eta if stiff == "eta" else mu
        assert np.abs(top[0]).max() == target and max(np.abs(eta[0]).max(), np.abs(mu[0]).max()) == target, r


def test_argument_refusals_keep_their_status_and_text():
    """Status code and full ff_last_error() text of every refusal that the entry points share through the argument validators of
    csrc/ff_host.h (net complete, hidden width, tolerances, orbital tables, determinant size) and of the shape refusals beside them.
    Callers match on these strings (fermiflow_amd/_lib.py check() passes them on).  Every call here is refused before anything is
    launched, so it runs without a GPU and is harmless with one; the pointers are never dereferenced."""
    import ctypes as C
    from fermiflow_amd import _lib
    lib = _lib.lib()
    p8, i64, f64 = C.c_void_p(8), C.c_int64, C.c_double
    B = i64(4)
    net_ok = _lib.FFNet(50, p8, p8, p8, 50, p8, p8, p8)
    bad_nets = [_lib.FFNet(50, None, p8, p8, 0, None, None, None), _lib.FFNet(50, p8, None, p8, 0, None, None, None),
                _lib.FFNet(50, p8, p8, None, 50, p8, p8, p8), _lib.FFNet(0, p8, p8, p8, 0, None, None, None),
                _lib.FFNet(50, p8, p8, p8, 50, None, p8, p8), _lib.FFNet(50, p8, p8, p8, 50, p8, p8, None)]
    wide_nets = [_lib.FFNet(300, p8, p8, p8, 50, p8, p8, p8), _lib.FFNet(50, p8, p8, p8, 300, p8, p8, p8)]
    ode_ok = _lib.FFOde(0.0, 1.0, 1e-6, 1e-8, 0)
    bad_odes = [_lib.FFOde(0.0, 1.0, 0.0, 1e-8, 0), _lib.FFOde(0.0, 1.0, 1e-6, -1.0, 0)]
    r = C.byref

    def refused(status, text, fn, *args):
        got = getattr(lib, fn)(None, *args)
        assert (got, lib.ff_last_error().decode()) == (status, text), (fn, got, lib.ff_last_error())

    # --- ff_net / ff_ode of the flow entry points: complete net (1), hidden width (2), tolerances (1), in that order
    flow = {
        "ff_cnf_generate": lambda n, o, nn=6, d=2: (B, nn, d, n, o, p8, p8, None),
        "ff_cnf_delta_logp": lambda n, o, nn=6, d=2: (B, nn, d, n, o, p8, p8, p8, None),
        "ff_eloc_sensitivities": lambda n, o, nn=6, d=2: (B, nn, d, n, o, p8, p8, None),
        "ff_eloc_nd": lambda n, o: (B, 3, 3, 2, p8, p8, None, n, o, f64(2.0), 1, p8, p8, p8, p8, p8, p8, p8, p8, p8, p8, None),
        "ff_eloc": lambda n, o: (B, 3, 3, p8, p8, None, n, o, f64(2.0), 1, p8, p8, p8, p8, p8, p8, p8, p8, p8, p8, None),
    }
    adjoint = {
        "ff_cnf_adjoint": lambda n, o, nn=6, d=2, gp=p8: (B, nn, d, n, o, p8, p8, p8, None, gp, p8, None),
        "ff_cnf_adjoint_energy": lambda n, o, nn=6, d=2, gp=p8: (B, nn, d, n, o, p8, p8, p8, p8, None, f64(0.25), None, gp, p8, None),
    }
    for who, fns in (("ff_cnf", flow), ("ff_cnf_adjoint", adjoint)):
        for fn, args in fns.items():
            for net in bad_nets:
                refused(1, f"{who}: bad net", fn, *args(r(net), r(ode_ok)))
                refused(1, f"{who}: bad net", fn, *args(r(net), r(bad_odes[0])))          # the net is looked at first
            for net in wide_nets:
                refused(2, f"{who}: hidden width > 256", fn, *args(r(net), r(ode_ok)))
                refused(2, f"{who}: hidden width > 256", fn, *args(r(net), r(bad_odes[1])))   # ... and its width before the tolerances
            for ode in bad_odes:
                refused(1, f"{who}: tolerances must be positive", fn, *args(r(net_ok), r(ode)))
            refused(1, f"{who}: bad argument", fn, *args(None, r(ode_ok)))
            refused(1, f"{who}: bad argument", fn, *args(r(net_ok), None))
    for fn in ("ff_cnf_generate", "ff_cnf_delta_logp", "ff_eloc_sensitivities"):
        refused(1, "ff_cnf: bad argument", fn, *flow[fn](r(bad_nets[0]), r(ode_ok), 0, 2))
        refused(1, "ff_cnf: bad argument", fn, *flow[fn](r(net_ok), r(ode_ok), 6, 0))
    for fn in adjoint:
        refused(1, "ff_cnf_adjoint: bad argument", fn, *adjoint[fn](r(bad_nets[0]), r(ode_ok), 6, 2, None))   # grad_params missing
        refused(2, "ff_cnf_adjoint: n*d > 64", fn, *adjoint[fn](r(net_ok), r(ode_ok), 33, 2))
    # n beyond the fused kernels (n <= 24, n d <= 60)
    for fn in ("ff_cnf_generate", "ff_cnf_delta_logp"):
        for nn, d in ((25, 2), (21, 3), (6, 4)):
            refused(2, "fused CNF kernels serve n <= 24 particles with n*d <= 60 in d = 2, 3", fn, *flow[fn](r(net_ok), r(ode_ok), nn, d))
    # --- entry points that only ask for a complete net (any width)
    refused(1, "ff_radial_table_build: null pointer", "ff_radial_table_build", None, p8)
    refused(1, "ff_radial_table_build: null pointer", "ff_radial_table_build", r(net_ok), None)
    for net in bad_nets:
        refused(1, "ff_radial_table_build: bad net", "ff_radial_table_build", r(net), p8)
        refused(1, "ff_backflow_vjp: bad net", "ff_backflow_vjp", B, 6, 2, r(net), p8, p8, p8, p8)
        refused(1, "ff_backflow_v_div: bad net", "ff_backflow_v_div", B, 6, 2, r(net), p8, p8, p8)
        refused(1, "ff_backflow_v_div_f32: bad net", "ff_backflow_v_div_f32", B, 6, 2, r(net), p8, p8, p8)
    refused(1, "ff_backflow_vjp: bad argument", "ff_backflow_vjp", B, 6, 2, None, p8, p8, p8, p8)
    refused(2, "ff_backflow_vjp: n > 24 or d > 3", "ff_backflow_vjp", B, 25, 2, r(net_ok), p8, p8, p8, p8)
    refused(1, "ff_backflow_v_div: bad argument", "ff_backflow_v_div", B, 6, 2, None, p8, p8, p8)
    refused(2, "ff_backflow_v_div: n > 24 or d > 3", "ff_backflow_v_div", B, 6, 4, r(net_ok), p8, p8, p8)
    refused(1, "ff_backflow_v_div_f32: bad argument", "ff_backflow_v_div_f32", B, 6, 2, None, p8, p8, p8)
    refused(2, "ff_backflow_v_div_f32: n > 24 or d > 3", "ff_backflow_v_div_f32", B, 25, 2, r(net_ok), p8, p8, p8)
    # --- (nup, ndn, tab_up, tab_dn): a spin species that has particles needs its orbital table (1); a determinant holds at most 12 (2)
    spins = {      # arguments behind (stream, B, nup, ndn, tab_up, tab_dn)
        "ff_eloc_nd": (("ff_eloc",) * 2, lambda: (None, r(net_ok), r(ode_ok), f64(2.0), 1) + (p8,) * 10 + (None,), (2,)),
        "ff_eloc": (("ff_eloc",) * 2, lambda: (None, r(net_ok), r(ode_ok), f64(2.0), 1) + (p8,) * 10 + (None,), ()),
        "ff_eloc_finish": (("ff_eloc_finish",) * 2, lambda: (None, f64(2.0), 1) + (p8,) * 10, ()),
        "ff_eloc_finish3d": (("ff_eloc_finish3d: null orbital table", "ff_eloc_finish3d: walker too large"), lambda: (None, f64(2.0), 1) + (p8,) * 10, ()),
        "ff_logprob": (("ff_logprob",) * 2, lambda: (None, p8, p8, p8, p8), ()),
        "ff_logprob3d": (("ff_logprob3d: null pointer", "ff_logprob3d"), lambda: (None, p8, p8, p8, p8), ()),
        "ff_mcmc_sample_noise3d": (("ff_mcmc_sample_noise3d",) * 2, lambda: (None, 10, f64(0.1), p8, p8, p8, p8, p8, p8), ()),
        "ff_mcmc_sample3d": (("ff_mcmc_sample3d",) * 2, lambda: (None, 10, f64(0.1), C.c_uint64(1), i64(0), p8, p8, p8), ()),
        "ff_mcmc_sample_noise": (("ff_mcmc: null pointer", "ff_mcmc"), lambda: (None, 10, f64(0.1), p8, p8, p8, p8, p8, p8), ()),
        "ff_mcmc_sample": (("ff_mcmc: null pointer", "ff_mcmc"), lambda: (None, 10, f64(0.1), C.c_uint64(1), i64(0), p8, p8, p8), ()),
        "ff_mcmc_continue": (("ff_mcmc: null pointer", "ff_mcmc"), lambda: (None, 10, f64(0.1), C.c_uint64(1), i64(0), p8, p8, p8, p8), ()),
    }
    for fn, ((null_tab, too_large), rest, dim) in spins.items():
        null_tab = null_tab if ":" in null_tab else null_tab + ": null orbital table"
        too_large = too_large if ":" in too_large else too_large + ": determinant larger than FF_MAX_NS"
        for nup, ndn, tu, td in ((3, 3, None, p8), (3, 3, p8, None), (3, 0, None, None), (0, 3, p8, None)):
            refused(1, null_tab, fn, B, nup, ndn, *dim, tu, td, *rest())
        for nup, ndn in ((13, 3), (3, 13), (13, 0)):
            refused(2, too_large, fn, B, nup, ndn, *dim, p8, p8, *rest())
        assert getattr(lib, fn)(None, i64(0), 3, 0, *dim, p8, None, *rest()) == 0      # a species without particles needs no table
    # where both are wrong: the sampler looks at the size first, everybody else at the tables
    refused(2, "ff_mcmc: determinant larger than FF_MAX_NS", "ff_mcmc_sample", B, 13, 3, None, p8, *spins["ff_mcmc_sample"][1]())
    refused(1, "ff_logprob: null orbital table", "ff_logprob", B, 13, 3, None, p8, *spins["ff_logprob"][1]())
    refused(1, "ff_eloc: null orbital table", "ff_eloc", B, 13, 3, None, p8, *spins["ff_eloc"][1]())
    refused(1, "ff_eloc: bad particle numbers or dimension", "ff_eloc_nd", B, 3, 3, 4, p8, p8, *spins["ff_eloc_nd"][1]())
    refused(2, "ff_eloc_finish3d: walker too large", "ff_eloc_finish3d", B, 11, 11, p8, p8, *spins["ff_eloc_finish3d"][1]())      # 3 n > 64


# What tests/common.py kernel_families returned before it read ff_kernel_plan -- a Python restatement of the dispatch of csrc/, checked
# against the C++ shape by shape when it was retired -- for all six calls at every supported shape: data, not a second implementation.
PLAN_TABLE = {      # (call, n, d): (family, walkers per group, walkers per round at 2 CUs, at 256 CUs)
    ('flow', 1, 2): ('flow_table', 16, None, None),
    ('flow', 2, 2): ('flow_table', 16, None, None),
    ('flow', 3, 2): ('flow_table', 10, None, None),
    ('flow', 4, 2): ('flow_table', 8, None, None),
    ('flow', 5, 2): ('flow_table', 6, None, None),
    ('flow', 6, 2): ('flow_table', 5, None, None),
    ('flow', 7, 2): ('flow_table', 4, None, None),
    ('flow', 8, 2): ('flow_table', 4, None, None),
    ('flow', 9, 2): ('flow_table', 3, None, None),
    ('flow', 10, 2): ('flow_table', 3, None, None),
    ('flow', 11, 2): ('flow_table', 2, None, None),
    ('flow', 12, 2): ('flow_table', 2, None, None),
    ('flow', 13, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 14, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 15, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 16, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 17, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 18, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 19, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 20, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 21, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 22, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 23, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 24, 2): ('flow_wide', 1, 128, 16384),
    ('flow', 1, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 2, 3): ('flow_table', 10, None, None),
    ('flow', 3, 3): ('flow_table', 7, None, None),
    ('flow', 4, 3): ('flow_table', 5, None, None),
    ('flow', 5, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 6, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 7, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 8, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 9, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 10, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 11, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 12, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 13, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 14, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 15, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 16, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 17, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 18, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 19, 3): ('flow_wide', 1, 128, 16384),
    ('flow', 20, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 1, 2): ('flow_direct_fb', 16, 32768, 32768),
    ('flow_fb', 2, 2): ('flow_direct_fb', 16, 32768, 32768),
    ('flow_fb', 3, 2): ('flow_direct_fb', 10, 20480, 20480),
    ('flow_fb', 4, 2): ('flow_direct_fb', 8, 16384, 16384),
    ('flow_fb', 5, 2): ('flow_direct_fb', 6, 12288, 12288),
    ('flow_fb', 6, 2): ('flow_direct_fb', 5, 10240, 10240),
    ('flow_fb', 7, 2): ('flow_direct_fb', 4, 8192, 8192),
    ('flow_fb', 8, 2): ('flow_direct_fb', 4, 8192, 8192),
    ('flow_fb', 9, 2): ('flow_direct_fb', 3, 6144, 6144),
    ('flow_fb', 10, 2): ('flow_direct_fb', 3, 6144, 6144),
    ('flow_fb', 11, 2): ('flow_direct_fb', 2, 4096, 4096),
    ('flow_fb', 12, 2): ('flow_direct_fb', 2, 4096, 4096),
    ('flow_fb', 13, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 14, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 15, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 16, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 17, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 18, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 19, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 20, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 21, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 22, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 23, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 24, 2): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 1, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 2, 3): ('flow_direct_fb', 10, 20480, 20480),
    ('flow_fb', 3, 3): ('flow_direct_fb', 7, 14336, 14336),
    ('flow_fb', 4, 3): ('flow_direct_fb', 5, 10240, 10240),
    ('flow_fb', 5, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 6, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 7, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 8, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 9, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 10, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 11, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 12, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 13, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 14, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 15, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 16, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 17, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 18, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 19, 3): ('flow_wide', 1, 128, 16384),
    ('flow_fb', 20, 3): ('flow_wide', 1, 128, 16384),
    ('eloc', 1, 2): ('eloc_rows', 16, 128, 16384),
    ('eloc', 2, 2): ('eloc_columns', 16, 128, 16384),
    ('eloc', 3, 2): ('eloc_columns', 10, 80, 10240),
    ('eloc', 4, 2): ('eloc_mfma', 4, 64, 8192),
    ('eloc', 5, 2): ('eloc_mfma', 4, 64, 8192),
    ('eloc', 6, 2): ('eloc_mfma', 4, 64, 8192),
    ('eloc', 7, 2): ('eloc_rows', 2, 16, 2048),
    ('eloc', 8, 2): ('eloc_split', 2, 16, 2048),
    ('eloc', 9, 2): ('eloc_rows', 1, 8, 1024),
    ('eloc', 10, 2): ('eloc_rows', 1, 8, 1024),
    ('eloc', 11, 2): ('eloc_wide', 1, 4, 512),
    ('eloc', 12, 2): ('eloc_wide', 1, 4, 512),
    ('eloc', 13, 2): ('eloc_wide', 1, 4, 512),
    ('eloc', 14, 2): ('eloc_wide', 1, 4, 512),
    ('eloc', 15, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 16, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 17, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 18, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 19, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 20, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 21, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 22, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 23, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 24, 2): ('eloc_wide', 1, 2, 256),
    ('eloc', 1, 3): ('eloc_wide', 1, 8, 1024),
    ('eloc', 2, 3): ('eloc_rows', 10, 80, 10240),
    ('eloc', 3, 3): ('eloc_rows', 7, 56, 7168),
    ('eloc', 4, 3): ('eloc_rows', 5, 40, 5120),
    ('eloc', 5, 3): ('eloc_wide', 1, 4, 512),
    ('eloc', 6, 3): ('eloc_wide', 1, 4, 512),
    ('eloc', 7, 3): ('eloc_wide', 1, 4, 512),
    ('eloc', 8, 3): ('eloc_wide', 1, 4, 512),
    ('eloc', 9, 3): ('eloc_wide', 1, 4, 512),
    ('eloc', 10, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 11, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 12, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 13, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 14, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 15, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 16, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 17, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 18, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 19, 3): ('eloc_wide', 1, 2, 256),
    ('eloc', 20, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 1, 2): ('eloc_rows', 16, 128, 16384),
    ('eloc_fb', 2, 2): ('eloc_columns', 16, 128, 16384),
    ('eloc_fb', 3, 2): ('eloc_columns', 10, 80, 10240),
    ('eloc_fb', 4, 2): ('eloc_mfma', 4, 32, 4096),
    ('eloc_fb', 5, 2): ('eloc_mfma', 4, 32, 4096),
    ('eloc_fb', 6, 2): ('eloc_mfma', 4, 32, 4096),
    ('eloc_fb', 7, 2): ('eloc_rows', 2, 16, 2048),
    ('eloc_fb', 8, 2): ('eloc_split', 2, 16, 2048),
    ('eloc_fb', 9, 2): ('eloc_rows', 1, 8, 1024),
    ('eloc_fb', 10, 2): ('eloc_rows', 1, 8, 1024),
    ('eloc_fb', 11, 2): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 12, 2): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 13, 2): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 14, 2): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 15, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 16, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 17, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 18, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 19, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 20, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 21, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 22, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 23, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 24, 2): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 1, 3): ('eloc_wide', 1, 8, 1024),
    ('eloc_fb', 2, 3): ('eloc_rows', 10, 80, 10240),
    ('eloc_fb', 3, 3): ('eloc_rows', 7, 56, 7168),
    ('eloc_fb', 4, 3): ('eloc_rows', 5, 40, 5120),
    ('eloc_fb', 5, 3): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 6, 3): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 7, 3): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 8, 3): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 9, 3): ('eloc_wide', 1, 4, 512),
    ('eloc_fb', 10, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 11, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 12, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 13, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 14, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 15, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 16, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 17, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 18, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 19, 3): ('eloc_wide', 1, 2, 256),
    ('eloc_fb', 20, 3): ('eloc_wide', 1, 2, 256),
    ('adjoint', 1, 2): ('adj_tab', 16, 256, 32768),
    ('adjoint', 2, 2): ('adj_tab', 16, 256, 32768),
    ('adjoint', 3, 2): ('adj_tab', 10, 160, 20480),
    ('adjoint', 4, 2): ('adj_tab', 6, 96, 12288),
    ('adjoint', 5, 2): ('adj_tab', 4, 64, 8192),
    ('adjoint', 6, 2): ('adj_tab', 3, 48, 6144),
    ('adjoint', 7, 2): ('adj_tab', 2, 32, 4096),
    ('adjoint', 8, 2): ('adj_tab', 4, 64, 8192),
    ('adjoint', 9, 2): ('adj_tab', 1, 16, 2048),
    ('adjoint', 10, 2): ('adj_tab', 1, 16, 2048),
    ('adjoint', 11, 2): ('adj_tab', 1, 16, 2048),
    ('adjoint', 12, 2): ('adj_tab', 2, 32, 4096),
    ('adjoint', 13, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 14, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 15, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 16, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 17, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 18, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 19, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 20, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 21, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 22, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 23, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 24, 2): ('adj_wide', 1, 8, 1024),
    ('adjoint', 1, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 2, 3): ('adj_tab', 10, 160, 20480),
    ('adjoint', 3, 3): ('adj_tab', 7, 112, 14336),
    ('adjoint', 4, 3): ('adj_tab', 3, 48, 6144),
    ('adjoint', 5, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 6, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 7, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 8, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 9, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 10, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 11, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 12, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 13, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 14, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 15, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 16, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 17, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 18, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 19, 3): ('adj_wide', 1, 8, 1024),
    ('adjoint', 20, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 1, 2): ('adj_direct', 16, 128, 16384),
    ('adj_fb', 2, 2): ('adj_direct', 16, 128, 16384),
    ('adj_fb', 3, 2): ('adj_direct', 10, 80, 10240),
    ('adj_fb', 4, 2): ('adj_direct', 8, 64, 8192),
    ('adj_fb', 5, 2): ('adj_direct', 6, 48, 6144),
    ('adj_fb', 6, 2): ('adj_direct', 5, 40, 5120),
    ('adj_fb', 7, 2): ('adj_direct', 4, 32, 4096),
    ('adj_fb', 8, 2): ('adj_direct', 4, 32, 4096),
    ('adj_fb', 9, 2): ('adj_direct', 3, 24, 3072),
    ('adj_fb', 10, 2): ('adj_direct', 3, 24, 3072),
    ('adj_fb', 11, 2): ('adj_direct', 2, 16, 2048),
    ('adj_fb', 12, 2): ('adj_direct', 2, 16, 2048),
    ('adj_fb', 13, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 14, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 15, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 16, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 17, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 18, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 19, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 20, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 21, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 22, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 23, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 24, 2): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 1, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 2, 3): ('adj_direct', 10, 80, 10240),
    ('adj_fb', 3, 3): ('adj_direct', 7, 56, 7168),
    ('adj_fb', 4, 3): ('adj_direct', 5, 40, 5120),
    ('adj_fb', 5, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 6, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 7, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 8, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 9, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 10, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 11, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 12, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 13, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 14, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 15, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 16, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 17, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 18, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 19, 3): ('adj_wide', 1, 8, 1024),
    ('adj_fb', 20, 3): ('adj_wide', 1, 8, 1024),
}
PLAN_TABLE_SIM = {**PLAN_TABLE,      # the host simulator's build (FF_MFMA_FROM=99): no matrix-core kernel
    ('eloc', 4, 2): ('eloc_columns', 8, 64, 8192),
    ('eloc', 5, 2): ('eloc_columns', 6, 48, 6144),
    ('eloc', 6, 2): ('eloc_columns', 5, 40, 5120),
    ('eloc_fb', 4, 2): ('eloc_columns', 8, 64, 8192),
    ('eloc_fb', 5, 2): ('eloc_columns', 6, 48, 6144),
    ('eloc_fb', 6, 2): ('eloc_columns', 5, 40, 5120),
}
# walkers the sweep's shrink threshold was computed for before VMC._init_sweep read the plan: n = 1..24 in d = 2, n = 1..20 in d = 3
H_SHRINK_G = {2: [16, 16, 10, 4, 4, 4, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
              3: [21, 10, 7, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]}


def test_kernel_plan_reproduces_the_recorded_routing():
    """ff_kernel_plan (csrc/ff_plan.h: what the dispatch switches on) of the GPU build and of the simulator's build gives, at every
    supported shape and for every call, the family, group size and round the recorded table holds, at 2 and at 256 compute units;
    shapes beyond the kernels are refused.  The sweep's shrink threshold follows the plan's lockstep count: unchanged at every shape
    but one particle in d = 3, which the one-walker-per-workgroup kernel serves (0.25; the retired formula took it for 21 walkers)."""
    from fermiflow_amd import native
    from fermiflow_amd.VMC import _Sweep
    from tests.common import kernel_families
    shapes = [(n, 2) for n in range(1, 25)] + [(n, 3) for n in range(1, 21)]
    assert set(PLAN_TABLE) == set(PLAN_TABLE_SIM) == {(c, n, d) for c in native.PLAN_CALLS for n, d in shapes}
    for hostsim, table in ((False, PLAN_TABLE), (True, PLAN_TABLE_SIM)):
        for (call, n, d), (family, group, r2, r256) in table.items():
            for cus, rnd in ((2, r2), (256, r256)):
                assert kernel_families(call, n, d, cus, hostsim=hostsim) == {family: (group, rnd)}, (hostsim, call, n, d, cus)
    for call in native.PLAN_CALLS:
        for n, d in ((0, 2), (25, 2), (21, 3), (6, 4), (6, 1)):
            with pytest.raises(NotImplementedError):
                native.kernel_plan(call, n, d)
    with pytest.raises(ValueError):
        native.kernel_plan("eloc", 6, 2, cus=0)
    for n, d in shapes:
        s = _Sweep()
        s._init_sweep(n, d)
        G = H_SHRINK_G[d][n - 1]
        want = 0.25 if (n, d) == (1, 3) else min(0.25, max(0.06, 1.0 - 0.65 ** (1.0 / G)))
        assert s._h_shrink_at == want, (n, d, s._h_shrink_at, want)
        assert G == PLAN_TABLE[("eloc", n, d)][1] or (n, d) == (1, 3)


def test_std_of_a_negative_sum_of_squares_is_zero_and_nan_stays_nan():
    """VMC._std clamps like the kernels: all-reduced sums restored from an older checkpoint may carry a rounding-sized negative centred
    sum of squares (sqrt of it was a NaN E_std / F_std); a NaN sum stays NaN"""
    import math
    from fermiflow_amd.VMC import _Sweep
    sw = _Sweep.__new__(_Sweep)
    sw._n_global = 1000
    sw._dev = {"E_ss": torch.tensor(-1.98e-9, dtype=torch.float64), "F_ss": torch.tensor(float("nan"), dtype=torch.float64),
               "S_ss": torch.tensor(999.0, dtype=torch.float64)}
    assert sw._std("E") == 0.0 and math.isnan(sw._std("F")) and sw._std("S") == 1.0
