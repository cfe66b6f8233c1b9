"""Helpers shared by the oracle, hostsim and GPU parity tests."""
import hashlib
import math
import os

import numpy as np
import torch


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def mcmc_noise_from_seed(G, name, dim=2):
    """Regenerate the torch-CPU noise stream of a g1 (dim = 2) or g7 (dim = 3) case in the reference's draw order
    (src/base_dist.py:62,65,68) and check it against the committed SHA-256 (detects RNG drift)."""
    nup, ndn, B, seed, steps = (int(v) for v in G[name + "_cfg"])
    torch.manual_seed(seed)
    n = nup + ndn
    g0 = torch.randn(B, n, dim, dtype=torch.float64)
    gs, us = [], []
    for _ in range(steps):
        gs.append(torch.randn(B, n, dim, dtype=torch.float64))
        us.append(torch.rand(B, dtype=torch.float64))
    g0, g, u = g0.numpy(), torch.stack(gs).numpy(), torch.stack(us).numpy()
    if sha(g0) + sha(g) + sha(u) != str(G[name + "_noise_sha"]):
        raise RuntimeError("torch CPU RNG stream differs from the one the golden vectors were made with")
    accept = np.unpackbits(G[name + "_accept"])[:steps * B].reshape(steps, B)
    return nup, ndn, g0, g, u, accept


def net_arrays(G, prefix, use_mu=True):
    eta = (G[prefix + "eta_w1"], G[prefix + "eta_b1"], G[prefix + "eta_w2"])
    mu = (G[prefix + "mu_w1"], G[prefix + "mu_b1"], G[prefix + "mu_w2"]) if use_mu else None
    return eta, mu


def cnf_param_grads(G, tag):
    names = [str(s) for s in G[tag + "_pnames"]]
    return np.concatenate([G[f"{tag}_g_{nm}"] for nm in names])


GSVMC_PG = ["cnf.v_wrapper.v.eta.fc1.weight", "cnf.v_wrapper.v.eta.fc1.bias", "cnf.v_wrapper.v.eta.fc2.weight",
            "cnf.v_wrapper.v.mu.fc1.weight", "cnf.v_wrapper.v.mu.fc1.bias", "cnf.v_wrapper.v.mu.fc2.weight"]


def gsvmc_param_grads(G, name, use_mu=True):
    keys = GSVMC_PG if use_mu else GSVMC_PG[:3]
    return np.concatenate([G[f"{name}_pg_{k}"] for k in keys])



# ---- sampler edge cases: tests/golden/g8_sampler_edges.npz (make_golden.py edges) -------------------------------------------
# (loaded here, not in conftest.py's `golden` fixture: the edge tests bring their own module-level fixture)
EDGE_SHAPES = [(2, 1), (3, 3), (6, 0), (6, 6), (4, 3), (10, 0)]     # log p probes, d = 2
EDGE_SHAPES3D = [(4, 3), (10, 10)]                                  # d = 3
EDGE_CHAINS = ["c3_3", "c6_0", "c2_1"]                              # crafted chains, d = 2 ("c3d4_3": d = 3)
_G8 = {}


def sampler_edges():
    if not _G8:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_sampler_edges.npz")) as z:
            _G8.update({k: z[k] for k in z.files})
    return _G8


def edge_chain(G, name):
    """nup, ndn, g0, g, u, accept (steps, B), and the reference's final x, log p and initial log p of a g8 chain"""
    nup, ndn, dim, B, steps = (int(v) for v in G[name + "_cfg"])
    accept = np.unpackbits(G[name + "_accept"])[:steps * B].reshape(steps, B)
    return (nup, ndn, G[name + "_g0"], G[name + "_g"].astype(np.float64), G[name + "_u"].astype(np.float64), accept,
            G[name + "_x"], G[name + "_logp"], G[name + "_logp0"])


def assert_edge_logp(lp, ref, rtol=1e-12):
    """-inf exactly where the reference has -inf (a zero column), NaN where it has NaN, the rest to rtol"""
    lp, ref = np.asarray(lp), np.asarray(ref)
    assert (np.isneginf(lp) == np.isneginf(ref)).all(), (lp, ref)
    assert (np.isnan(lp) == np.isnan(ref)).all(), (lp, ref)
    f = np.isfinite(ref)
    np.testing.assert_allclose(lp[f], ref[f], rtol=rtol, atol=0)


def bits_equal(a, b):
    """bit-identical float64 arrays (NaNs included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


def coincident_chains(nup, ndn, B, steps, dim=2, seed=0):
    """Walkers with identical rows in a Slater matrix, and crafted noise (g0, g, u):
      0: particles 0 and 1 (spin up) coincident, their proposals identical at every step -> the pair stays together;
      1: the same pair, ordinary proposals -> the first one separates it;
      2, 3: particles 0, 1, 2 coincident (nup >= 3; else another pair), kept together / separated;
      4: a coincident pair in the down species (ndn >= 2; else in the up species), kept together;
      the rest: ordinary walkers.
    The determinant of a matrix with two equal rows is 0: log p = -inf in exact arithmetic, and the kernels and the oracle
    compute it so (the reference returns a finite value that depends on LAPACK's rounding).  A chain whose pair stays
    together never accepts (p = exp(-inf - -inf) = NaN); one whose first proposal separates it accepts step 1 (p = +inf)."""
    rng = np.random.default_rng(seed)
    n = nup + ndn
    g0 = rng.standard_normal((B, n, dim)); g = rng.standard_normal((steps, B, n, dim)); u = rng.random((steps, B))
    trip = [0, 1, 2] if nup >= 3 else [0, 1]
    groups = {0: [0, 1], 1: [0, 1], 2: trip, 3: trip, 4: [nup, nup + 1] if ndn >= 2 else [nup - 2, nup - 1]}
    for b, idx in groups.items():
        g0[b, idx] = g0[b, idx[0]]
        if b in (0, 2, 4):
            g[:, b, idx] = g[:, b, idx[0]][:, None]
    kept, separated = np.array([0, 2, 4]), np.array([1, 3])
    return g0, g, u, kept, separated


def special_starts(nup, ndn, B, positions, dim=2, seed=0):
    """Ordinary normal walkers (B, n, dim) with special ones at `positions`, cycling through: all particles at the origin,
    all on the first axis, all on the second axis, a spiral at radius 16, 22 or 30, one NaN coordinate, a coincident
    pair (particles 0 and 1).  Returns the walkers and the same walkers with the special ones replaced by ordinary ones."""
    rng = np.random.default_rng(seed)
    n = nup + ndn
    x = rng.standard_normal((B, n, dim))
    plain = x.copy()
    k = np.arange(n)
    for i, b in enumerate(positions):
        kind = i % 8
        if kind == 0:
            x[b] = 0.0
        elif kind in (1, 2):
            x[b] = 0.0; x[b, :, kind - 1] = np.linspace(-1.3, 1.7, n)
        elif kind in (3, 4, 5):
            r = (16.0, 22.0, 30.0)[kind - 3] * (1 + 0.1 * k / n)      # (distinct radii: see make_golden.edge_probes)
            t = 2 * np.pi * (k + 0.37) / n
            x[b] = 0.0; x[b, :, 0] = r * np.cos(t); x[b, :, 1] = r * np.sin(t)
        elif kind == 6:
            x[b, n - 1, 0] = np.nan
        else:
            x[b, 1] = x[b, 0]
    return x, plain


# ---- GPU-side helpers (fermiflow_amd is imported lazily: the CPU suite imports this module too)
def T(a, dev, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def N(t):
    return t.detach().cpu().numpy()


# ---- stiff weight sets: every regime of the radial table's header (fermiflow_amd/csrc/ff_radial.h)
def stiff_net(target, seed=1, H=50, amp=0.05, stiff="eta"):
    """Seeded (eta, mu) weights (w1, b1, w2) with max|w1| over both nets exactly `target`, carried by the `stiff` net (the other
    one's |w1| stays at or below target / 2).  The sigmoid centres c = -b1 / w1 are spread over 0.3 .. 9 (across r = 8, where the
    adjoint's deposit table leaves LDS), so that the sharp switches sit at radii the walkers take; w2 ~ amp / max(target, 2) keeps
    the flow's first derivative bounded while the higher ones grow with the target."""
    rng = np.random.RandomState(seed)

    def one(wmax, a):
        w1 = rng.uniform(0.25, 1.0, H) * wmax * rng.choice([-1.0, 1.0], H)
        w1[rng.randint(H)] = wmax * (1.0 if rng.rand() < 0.5 else -1.0)
        c = rng.uniform(0.3, 9.0, H)
        return w1, -w1 * c, rng.standard_normal(H) * a / max(float(target), 2.0)
    # (mu multiplies x_i itself, a growth rate summed over H units: at eta's amplitude it carries walkers off the table)
    if stiff == "eta":
        return one(float(target), amp), one(0.5 * float(target), 0.2 * amp)
    return one(0.5 * float(target), amp), one(float(target), 0.2 * amp)


def radial_header(w):
    """Slots 0..5 of the radial table's header for max|w1| = w: the rule of ff_radial.h restated.
    (1/h, h, nodes, table refused, deposit grid refused, coefficients per deposit row)"""
    lg = 6
    while lg < 9 and w * 2.0 ** -lg > 0.06:
        lg += 1
    bad = not (w * 2.0 ** -lg <= 0.06)
    xd = 1.5 * w / 16.0
    nrow = next((n for n in (6, 8, 10) if xd ** n / math.factorial(n) <= 4.5e-12), 12)
    return [2.0 ** lg, 2.0 ** -lg, float(32 * 2 ** lg + 1), float(bad), 0.0 if w / 16.0 <= 0.4 else 1.0, float(nrow)]


FF_TAB_HDR, FF_TAB_ROW, FF_TAB_NMAX = 16, 10, 32 * 512 + 1       # ff_radial.h: the table tensor's layout

# the regimes of tests/test_gpu_stiff_weights.py: name -> (max|w1|, the net that carries it)
STIFF_REGIMES = {"w0.4": (0.4, "eta"), "w1": (1.0, "eta"), "w2.5": (2.5, "eta"), "w3.7": (3.7, "eta"), "w5": (5.0, "eta"),
                 "w5mu": (5.0, "mu"), "w7": (7.0, "eta"), "w12": (12.0, "eta"), "w25": (25.0, "eta"), "w40": (40.0, "eta")}
STIFF_NARROW_REGIMES = ["w0.4", "w1", "w2.5", "w3.7", "w5", "w7", "w12", "w25", "w40"]       # every regime of the table
STIFF_BROAD_REGIMES = ["w3.7", "w5", "w7", "w25", "w40"]       # 12 rows, h = 1/128, deposit refused, h = 1/512, table refused


def radial_nodes_ref(w, h, nodes):
    """f^(0..8)(j h), j < nodes, of one scalar MLP f(r) = sum w2 sigma(w1 r + b1) in long double: (nodes, 9).  The derivatives of
    sigma come from the recursion P_{n+1}(s) = P_n'(s) s (1 - s) on polynomials in s = sigma, built here independently of the
    kernels' coefficient table."""
    P = [np.polynomial.Polynomial([0.0, 1.0])]
    s1 = np.polynomial.Polynomial([0.0, 1.0, -1.0])
    for _ in range(8):
        P.append(P[-1].deriv() * s1)
    w1, b1, w2 = (np.asarray(a, dtype=np.longdouble) for a in w)
    r = np.arange(nodes, dtype=np.longdouble) * np.longdouble(h)
    out = np.zeros((nodes, 9), dtype=np.longdouble)
    for k in range(len(w1)):
        s = 1 / (1 + np.exp(-(w1[k] * r + b1[k])))
        wp = w2[k]
        for n in range(9):
            c = P[n].coef.astype(np.longdouble)
            v = np.zeros_like(s)
            for ck in c[::-1]:
                v = v * s + ck
            out[:, n] += wp * v
            wp = wp * w1[k]
    return out


def make_mlp(w, dev):
    import fermiflow_amd as ff
    m = ff.MLP(1, len(w[1]))
    with torch.no_grad():
        m.fc1.weight.copy_(torch.as_tensor(w[0]).reshape(-1, 1))
        m.fc1.bias.copy_(torch.as_tensor(w[1]))
        m.fc2.weight.copy_(torch.as_tensor(w[2]).reshape(1, -1))
    return m.to(dev)


def make_flow(eta, mu, dev):
    import fermiflow_amd as ff
    v = ff.Backflow(make_mlp(eta, dev), mu=make_mlp(mu, dev) if mu is not None else None)
    return ff.CNF(v, (0.0, 1.0))


# ---- launch geometry of the persistent grids, for the tests that must reach a second walker group per workgroup: read from the
# library's own plan (ff_kernel_plan, fermiflow_amd/csrc/ff_plan.h -- what the dispatch itself switches on).  Each family maps to
# (walkers per group, walkers per round of the grid); a round of None means one workgroup per group: that grid never loops.
def cu_count(hostsim=False):
    """Compute units the grid caps are sized by: the device's, or the host simulator's 2 (tests/hostsim/hip_shim.h:85)."""
    return 2 if hostsim else torch.cuda.get_device_properties(0).multi_processor_count


_FAMILY_NAMES = {"flow": {"narrow": "flow_table", "wide": "flow_wide"}, "flow_fb": {"narrow": "flow_direct_fb", "wide": "flow_wide"},
                 "adjoint": {"tabulated": "adj_tab", "wide": "adj_wide"}, "adj_fb": {"direct": "adj_direct", "wide": "adj_wide"}}


def kernel_families(call, n, d, cus, hostsim=False):
    """{family: (walkers per group, walkers per round or None)} of the kernels that do the work of one stand-alone native call
    with a radial-table net and every radius on the table: call = "flow" (cnf_generate / cnf_delta_logp), "eloc" (ff_eloc_nd,
    queue mode), "adjoint"; "flow_fb", "eloc_fb", "adj_fb" = the direct kernels that redo the call when a radius is off the table.
    hostsim: the plan of the host simulator's build (FF_MFMA_FROM=99, tests/hostsim/Makefile: no matrix-core kernel there)."""
    from fermiflow_amd import native
    if hostsim:
        from tests.hostsim import simlib
        fam, g, r = simlib.kernel_plan(native.PLAN_CALLS.index(call), n, d, cus)
        fam = native.PLAN_FAMILIES[fam]
    else:
        fam, g, r = native.kernel_plan(call, n, d, cus)
    return {"eloc_" + fam if call in ("eloc", "eloc_fb") else _FAMILY_NAMES[call][fam]: (g, r or None)}


def looping_batch(fams, rounds=2):
    """Smallest B that makes every capped family start more than `rounds` rounds, with a ragged last group wherever a group holds
    more than one walker (and a ragged last round everywhere)."""
    caps = [r for _, r in fams.values() if r]
    B = rounds * max(caps) + 1 if caps else 64
    while any((g > 1 and B % g == 0) or (r and B % r == 0) for g, r in fams.values()):
        B += 1
    return B


def assert_loops(fams, B, rounds=2):
    for name, (g, r) in fams.items():
        assert g == 1 or B % g != 0, (name, B, g)       # ragged last group (every family, looping or not)
        if r:
            assert B > rounds * r, (name, B, r)
            assert B % r != 0, (name, B, r)


def probe_set(B, fams, seed=0, nrand=16, edge_rounds=3):
    """Walkers where a state carried from one group to the next would show: 0 and B - 1, the first and last walker of the first and
    last `edge_rounds` rounds of every family's grid, every walker of each family's ragged last group, and a seeded random sample.
    (Queue-ordered calls are compared with the unordered call over the whole batch instead.)"""
    s = {0, B - 1}
    for g, r in fams.values():
        if r:
            nr = (B + r - 1) // r
            for k in sorted(set(range(min(edge_rounds, nr))) | set(range(max(0, nr - edge_rounds), nr))):
                s.update((k * r, min(B, (k + 1) * r) - 1))
        last = ((B - 1) // g) * g
        s.update(range(last, B))
    rng = np.random.RandomState(seed)
    s.update(int(v) for v in rng.choice(B, size=min(nrand, B), replace=False))
    return np.array(sorted(s), dtype=np.int64)
