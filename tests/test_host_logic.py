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
    assert lib.ff_cnf_adjoint_energy(None, C.c_int64(4), 6, 2, C.byref(net), C.byref(ode), p8, p8, None, p8, C.c_double(0.25),
                                     None, p8, p8, None) == 1                       # eloc missing
    assert lib.ff_cnf_adjoint(None, C.c_int64(4), 6, 2, C.byref(net), C.byref(ode), p8, p8, None, None, p8, p8, None) == 1   # a_d missing


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
