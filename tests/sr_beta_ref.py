"""Shared by tests/test_sr_beta_hostsim.py and tests/test_gpu_sr_beta.py: cases, data, ctypes calls into the host simulator's library and
the long-double references of the per-state moments (ff_sr_state_moments / ff_sr_state_finish)."""

import numpy as np

from tests.sr_ref import EPS

# name -> (B, P, walkers per state)
CASES = {
    "a": (1, 24, [1]),                                          # one walker, one state
    "b": (37, 36, [1, 0, 20, 15, 1]),                           # singletons and an empty state
    "c": (4099, 300, [100, 1900, 100, 1990, 0, 8, 1]),          # states straddle both chunk boundaries, 2048 and 4096; one is empty
    "d": (300, 24, [1] * 300),                                  # every state a singleton: fisher is zero within its bound
    "e": (0, 300, [0, 0, 0]),                                   # empty batch
}
IDS = list(CASES)


def sums_len(P, ns):
    return P * P + ns * P + P + ns


def split_sums(sums, P, ns):
    """S_raw (P, P), o_state (ns, P), g_sum (P), c_state (ns)"""
    a, b, c = P * P, P * P + ns * P, P * P + ns * P + P
    return sums[:a].reshape(P, P), sums[a:b].reshape(ns, P), sums[b:c], sums[c:c + ns]


def state_data(name, seed=0):
    """seeded O with mean about 1 (centring matters; the states' means differ), local energies around 3, the sorted state list and a
    per-state baseline near the states' mean energies: (O, e, walker_state int32, mean_e)"""
    B, P, counts = CASES[name]
    assert sum(counts) == B
    ns = len(counts)
    rng = np.random.default_rng(1000 * P + B + seed)
    ws = np.repeat(np.arange(ns, dtype=np.int32), counts)
    O = 1.0 + 0.5 * rng.standard_normal((B, P)) + 0.2 * np.cos(ws)[:, None]
    e = 3.0 + rng.standard_normal(B) + 0.1 * ws
    mean_e = 2.9 + 0.1 * np.arange(ns) + 0.05 * rng.standard_normal(ns)
    return O, e, ws, mean_e


def raw_ref(O, e, ws, mean_e):
    """long-double raw sums and their bounds, built as sr_ref.moment_ref builds its own: an entry that is a dot product of m terms
    lies within m eps |x| |y| of the exact one (gamma_m |x| |y| of any summation order, with a factor 2 of room) -- S_raw over the
    batch, o_state[n] (y = 1) over the walkers of state n, g_sum (y = e - mean_e[state]) over the batch; the counts are exact"""
    L = np.longdouble
    ns = len(mean_e)
    O = O.astype(L)
    de = e.astype(L) - mean_e.astype(L)[ws] if len(e) else np.zeros(0, dtype=L)
    B, P = O.shape
    S = O.T @ O
    dg = np.sqrt(np.diag(S))
    c = np.bincount(ws, minlength=ns).astype(np.int64)
    o = np.zeros((ns, P), dtype=L)
    bo = np.zeros((ns, P), dtype=L)
    for n in range(ns):
        rows = O[ws == n]
        o[n] = rows.sum(axis=0)
        bo[n] = c[n] * EPS * np.sqrt((rows * rows).sum(axis=0)) * np.sqrt(L(c[n]))
    g = O.T @ de
    return dict(S=S, o=o, g=g, c=c, B=B, P=P, ns=ns,
                bS=B * EPS * np.outer(dg, dg), bo=bo, bg=B * EPS * dg * np.sqrt((de * de).sum()))


def check_raw_sums(sums, ref):
    S, o, g, c = split_sums(sums, ref["P"], ref["ns"])
    assert (c == ref["c"]).all()      # exact
    assert (S == S.T).all()
    assert (np.abs(S - ref["S"]) <= ref["bS"]).all(), float((np.abs(S - ref["S"]) / ref["bS"]).max())
    assert (np.abs(o - ref["o"]) <= ref["bo"]).all()
    assert (np.abs(g - ref["g"]) <= ref["bg"]).all()


def finished_ref(ref):
    """fisher = (S - G) / B with G = sum_{n: c_n > 0} o_n o_n^T / c_n, obar_state = o_n / c_n, grad = g / B in long double, and their
    bounds propagated from the raw sums':
      G_ij is a sum over the states of products r_ni r_nj, r_n = o_n / sqrt(c_n): the inputs' bounds give
      sum_n (bo_ni |o_nj| + |o_ni| bo_nj) / c_n; each r carries two roundings (the square root, the quotient: 2 eps with the factor 2 of
      room), hence 4 eps per product; the dot product over ns states ns eps more: (ns + 4) eps sum_n |o_ni o_nj| / c_n;
      fisher: (bS + bG) / B and two roundings (the difference, the quotient): 2 eps |F|;   obar, grad: one quotient."""
    L = np.longdouble
    B = L(ref["B"])
    P, ns = ref["P"], ref["ns"]
    o, c = ref["o"], ref["c"]
    G, aG, bG = (np.zeros((P, P), dtype=L) for _ in range(3))
    ob, bob = np.zeros((ns, P), dtype=L), np.zeros((ns, P), dtype=L)
    for n in range(ns):
        if c[n] == 0:
            continue
        cn, ao = L(c[n]), np.abs(o[n])
        G += np.outer(o[n], o[n]) / cn
        aG += np.outer(ao, ao) / cn
        bG += (np.outer(ref["bo"][n], ao) + np.outer(ao, ref["bo"][n])) / cn
        ob[n] = o[n] / cn
        bob[n] = ref["bo"][n] / cn + EPS * np.abs(ob[n])
    bG += (ns + 4) * EPS * aG
    F = (ref["S"] - G) / B
    bF = (ref["bS"] + bG) / B + 2 * EPS * np.abs(F)
    Gr = ref["g"] / B
    return dict(F=F, ob=ob, G=Gr, bF=bF, bob=bob, bG=ref["bg"] / B + EPS * np.abs(Gr), c=c)


def check_finished(f, ob, g, fr, scale=1.0):
    assert (f == f.T).all()
    assert (np.abs(f - fr["F"]) <= scale * fr["bF"]).all(), float((np.abs(f - fr["F"]) / fr["bF"]).max())
    assert (np.abs(ob - fr["ob"]) <= scale * fr["bob"]).all()
    assert (ob[fr["c"] == 0] == 0.0).all()
    assert (np.abs(g - fr["G"]) <= scale * fr["bG"]).all(), float((np.abs(g - fr["G"]) / fr["bG"]).max())


# ---- host simulator: ctypes calls (S = tests.hostsim.simlib)
def _ws(lib, B, P, ns):
    return np.full(max(1, lib.ff_sr_state_moments_workspace_bytes(B, P, ns) // 8), np.nan)


def sim_state_moments(S, O, e, ws, mean_e, check=True, ns=None):
    """ff_sr_state_moments of the simulator's library: (status, sums)"""
    lib = S.lib()
    O = np.ascontiguousarray(O, dtype=np.float64); e = np.ascontiguousarray(e, dtype=np.float64)
    ws = np.ascontiguousarray(ws, dtype=np.int32); mean_e = np.ascontiguousarray(mean_e, dtype=np.float64)
    B, P = O.shape
    ns = len(mean_e) if ns is None else ns
    work = _ws(lib, B, P, ns)
    sums = np.full(sums_len(max(P, 1), max(ns, 1)), np.nan)
    st = lib.ff_sr_state_moments(None, B, P, ns, S._p(O), S._p(e), S._p(ws), S._p(mean_e), S._p(sums), S._p(work))
    if check:
        assert st == 0, lib.ff_last_error()
    return st, sums


def sim_state_finish(S, sums, P, ns):
    lib = S.lib()
    f, ob, g = np.full((P, P), np.nan), np.full((ns, P), np.nan), np.full(P, np.nan)
    work = _ws(lib, 0, P, ns)
    st = lib.ff_sr_state_finish(None, P, ns, S._p(np.ascontiguousarray(sums)), S._p(f), S._p(ob), S._p(g), S._p(work))
    assert st == 0, lib.ff_last_error()
    return f, ob, g
