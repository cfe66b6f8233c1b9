"""Shared by tests/test_sr_hostsim.py and tests/test_gpu_sr.py: shapes, walkers, ctypes calls into the host simulator's library and
the references of the stochastic-reconfiguration tests (ff_cnf_adjoint_scores, ff_sr_moments, ff_sr_finish)."""
import ctypes as C

import numpy as np

from tests.frames_ref import walkers      # noqa: F401  (the walkers of these tests are those of the frames tests)

# (n, d, B): G = 16 with a nearly empty second group; ...; d = 3
SHAPES = [(2, 2, 17), (3, 2, 11), (6, 2, 7), (7, 2, 5), (12, 2, 3), (3, 3, 8)]
IDS = [f"{n}x{d}_B{B}" for n, d, B in SHAPES]
WIDE_NET_SHAPE = (3, 2, 4)      # He = Hm = 100 at 6 coordinates: 66 units per unit0 chunk, that loop runs twice
Z = 2.0
T0, T1 = 0.0, 1.0
LOOSE = dict(rtol=1e-6, atol=1e-8)
TIGHT = dict(rtol=1e-10, atol=1e-12)

# Bar of the scores against oracle.cnf_adjoint walker by walker at TIGHT (error of a row relative to its largest |entry|):
# 4 x the largest such error of the EXISTING direct ff_cnf_adjoint (B = 1 calls, radial_table = NULL) against the same oracle calls on
# the same walkers, over SHAPES with and without mu.  Under the host simulator (tests/test_sr_hostsim.py measures both again):
YARDSTICK_HOSTSIM = 6.402e-11   # existing direct adjoint, as measured (2 x 2, B = 17, no mu; 2.9e-11 .. 6.4e-11 over the shapes)
SCORES_HOSTSIM = 6.402e-11      # the scores: the same number, shape by shape -- the rows are bit-identical to the one-walker calls

SR_CHUNK = 2048                 # FF_SR_CHUNK (fermiflow_amd/csrc/ff_sr.h): walkers per chunk of ff_sr_moments
MOMENT_CASES = [(1, 24), (5, 36), (4099, 300), (0, 300)]
EPS = 2.0 ** -52


def spins(n):
    return (n + 1) // 2, n // 2


def wide_net_arrays(H=100, seed=5):
    rng = np.random.default_rng(seed)
    one = lambda a: (rng.standard_normal(H) * 0.8, rng.standard_normal(H), rng.standard_normal(H) * a / H)
    return one(1.5), one(0.4)


def row_rel_err(got, ref):
    """largest over the rows of max|got - ref| / max|ref|"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    return float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


# ---- host simulator: ctypes calls (S = tests.hostsim.simlib)
def sim_flow_end(S, x, net, tol):
    """z(t0), Delta and glogp0 of the walkers x from the simulator's own local-energy pass"""
    n, d = x.shape[1], x.shape[2]
    nup, ndn = spins(n)
    r = (S.eloc3d if d == 3 else S.eloc)(x, nup, ndn, net, Z, t0=T0, t1=T1, **tol)
    return r["z"], r["dlogp"], r["glogp0"]


def sim_scores(S, z, glogp0, net, tol, order=None, check=True, scores=None, null_scores=False):
    """ff_cnf_adjoint_scores of the simulator's library: (status, scores, stats)"""
    z = np.ascontiguousarray(z, dtype=np.float64); g0 = np.ascontiguousarray(glogp0, dtype=np.float64)
    B, n, d = z.shape
    if scores is None:
        scores = np.full((B, net.nparams), 7.0)
    stats = np.zeros(4, dtype=np.int32)
    ode = S._ode(T0, T1, tol["rtol"], tol["atol"], None, order)
    st = S.lib().ff_cnf_adjoint_scores(None, B, n, d, C.byref(net.c), C.byref(ode), S._p(z), S._p(g0), None if null_scores else S._p(scores), None, S._p(stats))
    if check:
        assert st == 0, S.lib().ff_last_error()
    return st, scores, stats


def sim_adjoint_one(S, z, glogp0, net, tol, b):
    """the existing ff_cnf_adjoint on walker b alone, seeds glogp0[b] and -1, direct evaluation: (grad_params, stats)"""
    assert net.c.radial_table is None
    _, gp, st = S.cnf_adjoint(z[b:b + 1], glogp0[b:b + 1], np.array([-1.0]), net, t0=T0, t1=T1, **tol)
    return gp, st


def sr_sums_len(P):
    return P * P + 2 * P + 2


def sim_moments(S, O, e, emean, check=True):
    """ff_sr_moments of the simulator's library: (status, sums)"""
    lib = S.lib()
    O = np.ascontiguousarray(O, dtype=np.float64); e = np.ascontiguousarray(e, dtype=np.float64)
    B, P = O.shape
    ws = np.full(max(1, lib.ff_sr_moments_workspace_bytes(B, P) // 8), np.nan)
    sums = np.full(sr_sums_len(max(P, 1)), np.nan)
    em = np.array([emean], dtype=np.float64)
    st = lib.ff_sr_moments(None, B, P, S._p(O), S._p(e), S._p(em), S._p(sums), S._p(ws))
    if check:
        assert st == 0, lib.ff_last_error()
    return st, sums


def sim_finish(S, sums, P):
    f, ob, g = np.full((P, P), np.nan), np.full(P, np.nan), np.full(P, np.nan)
    st = S.lib().ff_sr_finish(None, P, S._p(np.ascontiguousarray(sums)), S._p(f), S._p(ob), S._p(g))
    assert st == 0, S.lib().ff_last_error()
    return f, ob, g


# ---- moments: data, long-double reference and bounds
def moment_data(B, P, seed=0):
    """seeded O with mean about 1 (centring matters), local energies around 3"""
    rng = np.random.default_rng(100 * P + B + seed)
    O = 1.0 + 0.5 * rng.standard_normal((B, P))
    e = 3.0 + rng.standard_normal(B)
    return O, e, 2.9


def moment_ref(O, e, emean):
    """long-double sums and the bounds of the RAW sums: each entry of S_raw within B eps sqrt(S_ii S_jj) -- the dot-product bound
    gamma_B |x| |y| of any summation order with a factor 2 of room; o_sum (y = 1) and g_sum (y = e - E) likewise; sum(e - E)
    within B eps sum|e - E|"""
    L = np.longdouble
    O = O.astype(L); de = e.astype(L) - L(emean)
    B = O.shape[0]
    S = O.T @ O
    o = O.sum(axis=0); g = O.T @ de; se = de.sum()
    dg = np.sqrt(np.diag(S))
    r = dict(S=S, o=o, g=g, se=se, B=B)
    r["bS"] = B * EPS * np.outer(dg, dg)
    r["bo"] = B * EPS * dg * np.sqrt(L(B))
    r["bg"] = B * EPS * dg * np.sqrt((de * de).sum())
    r["bse"] = B * EPS * np.abs(de).sum()
    return r


def split_sums(sums, P):
    return sums[:P * P].reshape(P, P), sums[P * P:P * P + P], sums[P * P + P:P * P + 2 * P], sums[P * P + 2 * P], sums[P * P + 2 * P + 1]


def check_raw_sums(sums, ref, P):
    S, o, g, se, cnt = split_sums(sums, P)
    assert cnt == ref["B"]
    assert (S == S.T).all()
    assert (np.abs(S - ref["S"]) <= ref["bS"]).all(), float((np.abs(S - ref["S"]) / ref["bS"]).max())
    assert (np.abs(o - ref["o"]) <= ref["bo"]).all()
    assert (np.abs(g - ref["g"]) <= ref["bg"]).all()
    assert abs(se - ref["se"]) <= ref["bse"]


def finished_ref(ref):
    """fisher, obar, grad in long double and their bounds, propagated from the raw sums' (factor `scale` on all of them):
    fisher_ij = S_ij / B - o_i o_j / B^2: bS / B + (bo_i |o_j| + |o_i| bo_j) / B^2 + three roundings of the finish (the quotients and
    the product: 3 eps |o_i o_j| / B^2, eps |S_ij| / B, and eps on the difference); grad alike."""
    L = np.longdouble
    B = L(ref["B"])
    S, o, g, se = ref["S"], ref["o"], ref["g"], ref["se"]
    ob = o / B
    F = S / B - np.outer(ob, ob)
    G = g / B - ob * (se / B)
    ao = np.abs(ob)
    bF = ref["bS"] / B + (np.outer(ref["bo"], ao) + np.outer(ao, ref["bo"])) / B + EPS * (np.abs(S) / B + 4 * np.outer(ao, ao) + np.abs(F))
    bob = ref["bo"] / B + EPS * ao
    bG = ref["bg"] / B + (ref["bo"] * abs(se) + np.abs(o) * ref["bse"]) / (B * B) + EPS * (np.abs(g) / B + 4 * ao * abs(se / B) + np.abs(G))
    return dict(F=F, ob=ob, G=G, bF=bF, bob=bob, bG=bG)


def check_finished(f, ob, g, fr, scale=1.0):
    assert (f == f.T).all()
    assert (np.abs(f - fr["F"]) <= scale * fr["bF"]).all(), float((np.abs(f - fr["F"]) / fr["bF"]).max())
    assert (np.abs(ob - fr["ob"]) <= scale * fr["bob"]).all()
    assert (np.abs(g - fr["G"]) <= scale * fr["bG"]).all(), float((np.abs(g - fr["G"]) / fr["bG"]).max())


def sr_residual_bound(A, delta):
    """bar of ||A delta - g|| for a direct solve of the P x P system: P^2 eps ||A||_F ||delta||"""
    P = A.shape[0]
    return P * P * EPS * np.linalg.norm(A) * np.linalg.norm(delta)
