"""TEST-ONLY: a numpy restatement of the energy components of ff_energy_parts_accumulate, written from the definitions in
include/fermiflow_energy.h and not from the kernel, in numpy.longdouble; the rounding bounds of a correct fp64 implementation; a parser of
the accumulator; ctypes access to the host-simulated kernels; seeded input makers.  The product package never imports this.

Rounding bounds.  u = 2^-53 is the largest relative error of one fp64 operation (a fused multiply-add counts as one).  The error of a
number that is a sum of terms is at most (roundings on the path of a term) x u x (sum of the magnitudes of the terms), to first order in
u; the second-order terms are kept where they are cheap (e (1 + ...)) so that no constant has to absorb them.  The counts:
  |grad|^2, sum x^2   a term is squared (1) and passes at most M - 1 additions, M = n d: M roundings; the factor 1/8 or 1/2 is exact
  T_G                 R = M
  T_L                 one more, the fused -lap / 4 - T_G: R = M + 1, over the magnitudes |lap| / 4 + |grad|^2 / 8
  V_trap              R = M
  a pair term Z / r   the differences (each 1; squared, so 2 in r^2), d more for the squares and their sum: (d + 2) u on r^2, half of it
                      on r; the square root 1, the reciprocal 1, the factor Z 1, and the sum over the partners of a particle and then
                      over the particles, at most 2 n additions: R = (d + 2) / 2 + 3 + 2 n <= d + 4 + 2 n
  d_k = c_k - centre  one more on |d_k|
  a chunk's sums      32 walkers of a segment in order (32), the 8 segments (7), the chunks in order (ceil(B / 256)) and the addition to
                      the accumulator (1): DEPTH(B) = 40 + ceil(B / 256) additions on the path of a walker's term; a second moment
                      d_k d_l enters by a fused multiply-add, so its own rounding is one of these
  a state's sums      at most count + 10 additions on a path, whatever the size of the workgroup (its threads' strided sums, the tree,
                      the addition to the accumulator)
"""
import ctypes as C

import numpy as np

K = 6
CHUNK = 256
PARTIAL = 28
HEAD = 4
FIXED = 52
MAX_STATES = 65536
U = 2.0 ** -53
NAMES = ("T_L", "T_G", "V_trap", "V_uu", "V_ud", "V_dd")
LD = np.longdouble
# the derived quantities as linear combinations of the six components
DERIVED = {"V_ee": (0, 0, 0, 1, 1, 1), "E": (1, 0, 1, 1, 1, 1), "virial": (2, 0, -2, 1, 1, 1), "dT": (1, -1, 0, 0, 0, 0)}
E_PARTS = (0, 2, 3, 4, 5)


def depth(B):
    return 40 + (B + CHUNK - 1) // CHUNK


def parts(x, grad, lap, nup, Z, ft=LD):
    """(c (B, 6), mag (B, 6)): the components in `ft` and the sum of the magnitudes of the terms of each"""
    x, grad, lap = np.asarray(x, dtype=ft), np.asarray(grad, dtype=ft), np.asarray(lap, dtype=ft)
    B, n, d = x.shape
    c, mag = np.zeros((B, K), dtype=ft), np.zeros((B, K), dtype=ft)
    with np.errstate(all="ignore"):
        gg = (grad * grad).sum((1, 2))
        c[:, 1] = gg / ft(8)
        c[:, 0] = -lap / ft(4) - gg / ft(8)
        mag[:, 1], mag[:, 0] = gg / ft(8), np.abs(lap) / ft(4) + gg / ft(8)
        c[:, 2] = (x * x).sum((1, 2)) / ft(2)
        mag[:, 2] = c[:, 2]
        if Z != 0:
            for i in range(n):
                for j in range(i + 1, n):
                    r = np.sqrt(((x[:, i] - x[:, j]) ** 2).sum(-1))
                    k = 3 if j < nup else (4 if i < nup else 5)
                    c[:, k] += ft(Z) / r
                    mag[:, k] += abs(ft(Z)) / r
    return c, mag


def roundings(n, d):
    M = n * d
    return np.array([M + 1, M, M] + [d + 4 + 2 * n] * 3, dtype=np.float64)


def valid(x, grad, lap, nup, Z, wstate=None, nstates=0):
    """validity is decided in fp64, as the kernel computes it: all six components finite, and the state in range"""
    c, _ = parts(x, grad, lap, nup, Z, ft=np.float64)
    ok = np.isfinite(c).all(1)
    if nstates > 0:
        ws = np.asarray(wstate)
        ok &= (ws >= 0) & (ws < nstates)
    return ok


def reference(x, grad, lap, nup, Z, wstate=None, nstates=0, centre=None):
    """Every accumulator field of ONE call on a zeroed buffer, in longdouble, with the rounding bound of each double entry (`b_` + name)
    and the per-walker components and their bounds."""
    x = np.asarray(x, dtype=np.float64)
    B, n, d = x.shape
    ctr = np.zeros(K, dtype=LD) if centre is None else np.asarray(centre, dtype=LD)
    c, mag = parts(x, grad, lap, nup, Z)
    ok = valid(x, grad, lap, nup, Z, wstate, nstates)
    R = roundings(n, d).astype(LD)
    u = LD(U)
    c0, mag0 = np.where(ok[:, None], c, LD(0)), np.where(ok[:, None], mag, LD(0))
    e_c = R * u * mag0                                                  # (B, 6) error of a component
    dk = np.where(ok[:, None], c0 - ctr, LD(0))
    e_d = np.where(ok[:, None], e_c + u * np.abs(dk), LD(0))            # ... of a centred component
    D = LD(depth(B))
    out = dict(calls=1, walkers=int(ok.sum()), invalid=int(B - ok.sum()), valid=ok, parts=c, b_parts=e_c, centre=ctr)
    out["sum"] = dk.sum(0)
    out["b_sum"] = e_d.sum(0) + D * u * (np.abs(dk) + e_d).sum(0)
    prod = dk[:, :, None] * dk[:, None, :]
    e_p = np.abs(dk)[:, :, None] * e_d[:, None, :] + e_d[:, :, None] * np.abs(dk)[:, None, :] + e_d[:, :, None] * e_d[:, None, :]
    out["sum2"] = prod.sum(0)
    out["b_sum2"] = e_p.sum(0) + D * u * (np.abs(prod) + e_p).sum(0)
    S, b = out["sum"], out["b_sum"]
    out["blocksq"] = S * S
    out["b_blocksq"] = (2 * np.abs(S) * b + b * b) * (1 + 2 * u) + 2 * u * S * S      # the square (1) and its addition to the accumulator (1)
    if nstates > 0:
        ws = np.asarray(wstate)
        cnt, ssum, b_ssum = np.zeros(nstates, dtype=np.int64), np.zeros((nstates, K), dtype=LD), np.zeros((nstates, K), dtype=LD)
        sE2, b_sE2 = np.zeros(nstates, dtype=LD), np.zeros(nstates, dtype=LD)
        de = dk[:, E_PARTS].sum(1)
        e_de = e_d[:, E_PARTS].sum(1) + 4 * u * np.abs(dk[:, E_PARTS]).sum(1)      # four additions
        t2, e_t2 = de * de, 2 * np.abs(de) * e_de + e_de * e_de
        for s in range(nstates):
            m = ok & (ws == s)
            cnt[s] = int(m.sum())
            Ds = LD(cnt[s] + 10)
            ssum[s] = dk[m].sum(0)
            b_ssum[s] = e_d[m].sum(0) + Ds * u * (np.abs(dk[m]) + e_d[m]).sum(0)
            sE2[s] = t2[m].sum()
            b_sE2[s] = e_t2[m].sum() + Ds * u * (t2[m] + e_t2[m]).sum()
        out.update(count=cnt, ssum=ssum, b_ssum=b_ssum, sumE2=sE2, b_sumE2=b_sE2)
    return out


def statistics(ref):
    """means and walker-level standard errors of the six components and the derived quantities from a reference's moments (longdouble)"""
    N = LD(ref["walkers"])
    m = ref["sum"] / N
    cov = ref["sum2"] / N - np.outer(m, m)
    mean, err = {}, {}
    combos = {name: np.eye(K)[k] for k, name in enumerate(NAMES)}
    combos.update({k: np.array(v, dtype=np.float64) for k, v in DERIVED.items()})
    for name, a in combos.items():
        a = a.astype(LD)
        mean[name] = float(a @ (ref["centre"] + m))
        err[name] = float(np.sqrt(max(a @ cov @ a, LD(0)) / (N - 1)))
    return mean, err


# ---- the accumulator as the C ABI lays it out
def new_buffer(lib, nstates=0):
    nbytes = lib.ff_energy_parts_buffer_bytes(int(nstates))
    assert nbytes == 8 * (FIXED + 8 * nstates)
    return np.zeros(nbytes // 8, dtype=np.uint64)


def split(acc, nstates=0):
    a = np.ascontiguousarray(acc).view(np.uint64)
    f = a.view(np.float64)
    out = dict(calls=int(a[0]), walkers=int(a[1]), invalid=int(a[2]), ticket=int(a[3]), sum=f[4:10].copy(), sum2=f[10:46].reshape(K, K).copy(),
               blocksq=f[46:52].copy())
    if nstates > 0:
        S = nstates
        assert len(a) == FIXED + 8 * S
        out.update(count=a[FIXED:FIXED + S].astype(np.int64), ssum=f[FIXED + S:FIXED + 7 * S].reshape(S, K).copy(), sumE2=f[FIXED + 7 * S:].copy())
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def accumulate(lib, x, grad, lap, nup, ndn, Z, acc, wstate=None, nstates=0, centre=None, parts_out=None, B=None, d=None, null=(), ws=None):
    """ff_energy_parts_accumulate through ctypes; null: names of pointer arguments passed as NULL; returns the status"""
    a = dict(x=np.ascontiguousarray(x, dtype=np.float64), grad=np.ascontiguousarray(grad, dtype=np.float64), lap=np.ascontiguousarray(lap, dtype=np.float64))
    B = a["x"].shape[0] if B is None else B
    d = a["x"].shape[2] if d is None else d
    st = None if wstate is None else np.ascontiguousarray(wstate, dtype=np.int32)
    ctr = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    if ws is None:
        ws = np.full(max(1, lib.ff_energy_parts_workspace_bytes(max(B, 0), max(int(nstates), 0)) // 8), np.nan)      # (scratch: need not be zero)
    ptr = {k: (None if k in null else _p(v)) for k, v in a.items()}
    return lib.ff_energy_parts_accumulate(None, B, int(nup), int(ndn), int(d), float(Z), ptr["x"], ptr["grad"], ptr["lap"], _p(st), int(nstates),
                                          _p(ctr), _p(parts_out), None if "acc" in null else _p(acc), None if "workspace" in null else _p(ws))


def compare(got, ref, nstates=0, calls=1):
    """the parsed accumulator `got` after `calls` identical calls against the reference of one: the integers exactly, every double within
    its bound; returns the largest error-to-bound ratio"""
    assert (got["calls"], got["walkers"], got["invalid"], got["ticket"]) == (calls, calls * ref["walkers"], calls * ref["invalid"], 0)
    worst = 0.0
    names = ("sum", "sum2", "blocksq") + (("ssum", "sumE2") if nstates > 0 else ())
    for name in names:
        err = np.abs(got[name].astype(LD) - calls * ref[name])
        bound = calls * ref["b_" + name] + (calls - 1) * LD(U) * np.abs(calls * ref[name])      # (the later calls' additions to the accumulator)
        assert np.isfinite(got[name]).all(), name
        assert (err <= bound).all(), (name, float(err.max()), float(bound.max()))
        with np.errstate(all="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
        worst = max(worst, float(ratio.max()))
    if nstates > 0:
        assert np.array_equal(got["count"], calls * ref["count"])
    assert np.array_equal(got["sum2"], got["sum2"].T)                  # symmetric bit for bit
    return worst


def compare_parts(parts_out, ref):
    """(B, 6) of the kernel against the reference: valid walkers within the component's bound; an invalid walker that has all six finite
    was left out for its state.  Returns the largest error-to-bound ratio."""
    ok = ref["valid"]
    err = np.abs(parts_out[ok].astype(LD) - ref["parts"][ok])
    bound = ref["b_parts"][ok]
    assert (err <= bound).all(), float((err - bound).max())
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
    return float(ratio.max()) if ratio.size else 0.0


# ---- seeded inputs
def inputs(seed, B, nup, ndn, d):
    """walkers, gradients and Laplacians of no particular wave function: every term of every component at its natural size"""
    rng = np.random.default_rng(seed)
    n = nup + ndn
    return dict(x=rng.standard_normal((B, n, d)) * 1.2, grad=rng.standard_normal((B, n, d)) * 2.0, lap=-2.0 * n * d + 3.0 * rng.standard_normal(B))


def states(seed, B, nstates, empty=()):
    """a sorted state list over [0, nstates) that leaves the states `empty` out"""
    rng = np.random.default_rng(seed)
    live = [s for s in range(nstates) if s not in empty]
    return np.sort(rng.choice(live, size=B)).astype(np.int32)


GAUSS_SEED = 20240611


def gaussian_inputs(B, d, seed=GAUSS_SEED):
    """One particle in the ground state of the trap, psi = exp(-|x|^2 / 2): x ~ |psi|^2 = N(0, I / 2), grad log p = -2 x, laplacian = -2 d.
    E = d / 2 for every walker; <T_L> = <T_G> = <V_trap> = d / 4; virial and dT vanish on average."""
    rng = np.random.default_rng(seed + d)
    x = rng.standard_normal((B, 1, d)) * np.sqrt(0.5)
    return dict(x=x, grad=-2.0 * x, lap=np.full(B, -2.0 * d))
