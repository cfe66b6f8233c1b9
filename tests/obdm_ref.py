"""TEST-ONLY: a numpy restatement of the one-body density matrix estimator of ff_obdm_accumulate and of ff_slater_sign, written from
the definitions in include/fermiflow_obdm.h and not from the kernels, and ctypes access to the accumulator of the host-simulated
kernels.  Every function takes `ft`, the floating-point type it computes in: numpy.float64 restates the kernel, numpy.longdouble
measures the reference's own rounding.  The product package never imports this."""
import ctypes as C

import numpy as np

CHUNK = 256
HEAD = 5
EPS = 2.0 ** -52


def nbasis(nshells):
    return nshells * (nshells + 1) // 2


def degrees(count=36):
    """(nx, ny) of the first `count` orbitals in the HO2D list order"""
    return [(nx, N - nx) for N in range(8) for nx in range(N + 1)][:count]


def hermite(t, ft=np.float64):
    """h_0 .. h_7 at t by the three-term recurrence"""
    t = np.asarray(t, dtype=ft)
    h = [np.ones_like(t), np.sqrt(ft(2.0)) * t]
    for m in range(1, 7):
        h.append(np.sqrt(ft(2.0) / ft(m + 1)) * t * h[m] - np.sqrt(ft(m) / ft(m + 1)) * h[m - 1])
    return h


def orbitals(idx, x, y, ft=np.float64):
    """phi_k(x, y) for the orbital indices idx: (*shape, len(idx)); 0 where the Gaussian factor is 0 as computed"""
    x, y = np.asarray(x, dtype=ft), np.asarray(y, dtype=ft)
    deg = degrees()
    with np.errstate(all="ignore"):
        G = np.exp(-(x * x + y * y) / ft(2.0)) / np.sqrt(ft(np.pi))
        live = G > 0
        xs, ys = np.where(live, x, ft(0.0)), np.where(live, y, ft(0.0))
        hx, hy = hermite(xs, ft), hermite(ys, ft)
        return np.stack([np.where(live, G * hx[deg[k][0]] * hy[deg[k][1]], ft(0.0)) for k in idx], axis=-1)


def _tab(ns, tab):
    t = np.arange(ns) if tab is None else np.asarray(tab)
    return t.reshape(-1, ns)


def slater_sign(z, nup, ndn, tab_up=None, tab_dn=None, wstate=None):
    """(sign (B,), margin (B,)): the sign of det Phi_up det Phi_dn through numpy.linalg.slogdet of the orbital matrices (NaN for a
    walker with a non-finite coordinate), and the smallest |det| / prod(row norms) over the species -- how far from singular."""
    z = np.asarray(z, dtype=np.float64)
    B = z.shape[0]
    st = np.zeros(B, dtype=np.int64) if wstate is None else np.asarray(wstate, dtype=np.int64)
    sign, margin = np.ones(B), np.full(B, np.inf)
    for ns, off, tab in ((nup, 0, tab_up), (ndn, nup, tab_dn)):
        if not ns:
            continue
        t = _tab(ns, tab)
        for b in range(B):
            p = z[b, off:off + ns]
            if not np.isfinite(z[b]).all():
                sign[b] = np.nan
                continue
            Phi = orbitals(t[st[b]], p[:, 0], p[:, 1])          # [particle, orbital]
            s, _ = np.linalg.slogdet(Phi)
            sign[b] *= s
            with np.errstate(all="ignore"):
                margin[b] = min(margin[b], abs(np.linalg.det(Phi / np.linalg.norm(Phi, axis=1, keepdims=True))))
    return sign, margin


MARGIN = 1e-6


def good_walkers(seed, B, nup, ndn, tab_up=None, tab_dn=None, wstate=None):
    """B seeded walkers whose determinants are not within MARGIN of zero relative to the product of their row norms -- chosen with the
    reference alone: candidates are drawn in order and the near-singular ones are passed over."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, nup + ndn, 2)) * 1.5
    for _ in range(20):
        _, margin = slater_sign(z, nup, ndn, tab_up, tab_dn, wstate)
        bad = np.flatnonzero(~(margin > MARGIN))
        if not len(bad):
            return z
        z[bad] = rng.standard_normal((len(bad), nup + ndn, 2)) * 1.5
    raise AssertionError("no well-conditioned walkers found")


def condition(z, nup, ndn, tab_up=None, tab_dn=None, state=0):
    """cond_2 of the orbital matrix of each species of ONE walker z (n, 2): (cond_up, cond_dn), 1 for an empty species"""
    out = []
    for ns, off, tab in ((nup, 0, tab_up), (ndn, nup, tab_dn)):
        out.append(float(np.linalg.cond(orbitals(_tab(ns, tab)[state], z[off:off + ns, 0], z[off:off + ns, 1]))) if ns else 1.0)
    return tuple(out)


def ratios(sign, sign_moved, logp, logp_moved, ft=np.float64):
    with np.errstate(all="ignore"):
        return (np.asarray(sign, ft)[:, None] * np.asarray(sign_moved, ft)) * np.exp((np.asarray(logp_moved, ft) - np.asarray(logp, ft)[:, None]) / ft(2.0))


def weights(rp, sigma, nshells, ft=np.float64):
    """C (B, nb) of one species' points rp (B, 2): phi_c(r') / g(r')"""
    rp = np.asarray(rp, dtype=ft)
    s2 = ft(sigma) * ft(sigma)
    pi = ft(np.pi)          # (the double nearest pi in either precision: the kernels' constant)
    with np.errstate(all="ignore"):
        g = np.exp(-(rp[:, 0] * rp[:, 0] + rp[:, 1] * rp[:, 1]) / (ft(2.0) * s2)) / (ft(2.0) * pi * s2)
        return orbitals(range(nbasis(nshells)), rp[:, 0], rp[:, 1], ft) / g[:, None]


def estimate(x, rprime, logp, sign, logp_moved, sign_moved, sigma, nshells, nup, ft=np.float64, block=64):
    """One call of the estimator.  Returns dict(T (2, nb, nb), invalid (2,), abs (2, nb, nb): sum |terms| per entry, nterms (2,): terms
    per entry of the species).  A term is phi_a(x_i) q_i C_c / 2 or its transpose C_a phi_c(x_i) q_i / 2 of one valid sample."""
    x, rprime = np.asarray(x, dtype=np.float64), np.asarray(rprime, dtype=np.float64)
    B, n, _ = x.shape
    nb = nbasis(nshells)
    q64 = ratios(sign, sign_moved, logp, logp_moved)
    fin = np.isfinite(x).all(-1) & np.isfinite(q64)                         # validity is decided in fp64, as the kernel computes it
    T, S = np.zeros((2, nb, nb), dtype=ft), np.zeros((2, nb, nb), dtype=ft)
    invalid, nterms = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    q = ratios(sign, sign_moved, logp, logp_moved, ft)
    for s, (lo, hi) in enumerate(((0, nup), (nup, n))):
        if hi == lo:
            continue
        ok = fin[:, lo:hi] & np.isfinite(rprime[:, s]).all(-1)[:, None]      # (B, ns)
        invalid[s] = int((~ok).sum())
        nterms[s] = 2 * int(ok.sum())
        for b0 in range(0, B, block):
            sl = slice(b0, b0 + block)
            okb = ok[sl]
            Cw = np.where(okb.any(1)[:, None], weights(np.where(okb.any(1)[:, None], rprime[sl, s], 0.0), sigma, nshells, ft), ft(0.0))
            xs = np.where(okb[..., None], x[sl, lo:hi], 0.0)
            phi = orbitals(range(nb), xs[..., 0], xs[..., 1], ft)            # (b, i, a)
            w = phi * np.where(okb, q[sl, lo:hi], ft(0.0))[..., None]
            term = ft(0.5) * w[:, :, :, None] * Cw[:, None, None, :]         # (b, i, a, c)
            T[s] += term.sum((0, 1)) + term.sum((0, 1)).T
            S[s] += np.abs(term).sum((0, 1)) + np.abs(term).sum((0, 1)).T
    return dict(T=T, invalid=invalid, abs=S, nterms=nterms)


def term_delta(x, rprime, logp, sign, logp_moved, sign_moved, sigma, nshells, nup, block=64):
    """delta: the largest |term in fp64 - term in longdouble| over the terms of these inputs (the reference's own rounding)"""
    x, rprime = np.asarray(x, dtype=np.float64), np.asarray(rprime, dtype=np.float64)
    B, n, _ = x.shape
    nb = nbasis(nshells)
    fin = np.isfinite(x).all(-1) & np.isfinite(ratios(sign, sign_moved, logp, logp_moved))
    delta = 0.0
    for s, (lo, hi) in enumerate(((0, nup), (nup, n))):
        if hi == lo:
            continue
        ok = fin[:, lo:hi] & np.isfinite(rprime[:, s]).all(-1)[:, None]
        for b0 in range(0, B, block):
            sl = slice(b0, b0 + block)
            okb = ok[sl]
            t = []
            for ft in (np.float64, np.longdouble):
                q = ratios(sign[sl], sign_moved[sl], logp[sl], logp_moved[sl], ft)
                Cw = np.where(okb.any(1)[:, None], weights(np.where(okb.any(1)[:, None], rprime[sl, s], 0.0), sigma, nshells, ft), ft(0.0))
                xs = np.where(okb[..., None], x[sl, lo:hi], 0.0)
                phi = orbitals(range(nb), xs[..., 0], xs[..., 1], ft)
                w = phi * np.where(okb, q[:, lo:hi], ft(0.0))[..., None]
                t.append(ft(0.5) * w[:, :, :, None] * Cw[:, None, None, :])
            if t[0].size:
                delta = max(delta, float(np.abs(t[0].astype(np.longdouble) - t[1]).max()))
    return delta


def bound(ref, delta):
    """per entry: N 2^-52 sum |terms| (any summation order) + 4 N delta (the kernel's differently ordered, equally rounded terms)"""
    N = ref["nterms"][:, None, None].astype(np.float64)
    return N * EPS * ref["abs"].astype(np.float64) + 4.0 * N * delta


# ---- the accumulator as the C ABI lays it out
def new_buffer(lib, nshells):
    nbytes = lib.ff_obdm_buffer_bytes(int(nshells))
    assert nbytes == 8 * (HEAD + 4 * nbasis(nshells) ** 2)
    return np.zeros(nbytes // 8, dtype=np.uint64)


def split(acc, nshells):
    a = np.asarray(acc)
    nb = nbasis(nshells)
    E = 2 * nb * nb
    f = a[HEAD:].view(np.float64)
    return dict(calls=int(a[0]), walkers=int(a[1]), invalid=a[2:4].astype(np.int64), ticket=int(a[4]),
                sum=f[:E].reshape(2, nb, nb).copy(), sumsq=f[E:].reshape(2, nb, nb).copy())


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def accumulate(lib, x, rprime, logp, sign, logp_moved, sign_moved, sigma, nshells, nup, ndn, acc, B=None, null=(), ws=None):
    """ff_obdm_accumulate through ctypes; null: names of pointer arguments passed as NULL; returns the status"""
    a = dict(x=np.ascontiguousarray(x, dtype=np.float64), rprime=np.ascontiguousarray(rprime, dtype=np.float64),
             logp=np.ascontiguousarray(logp, dtype=np.float64), sign=np.ascontiguousarray(sign, dtype=np.float64),
             logp_moved=np.ascontiguousarray(logp_moved, dtype=np.float64), sign_moved=np.ascontiguousarray(sign_moved, dtype=np.float64))
    B = a["x"].shape[0] if B is None else B
    if ws is None:
        ws = np.full(max(1, lib.ff_obdm_workspace_bytes(max(B, 0), int(nshells)) // 8), np.nan)       # (scratch: need not be zero)
    ptr = {k: (None if k in null else _p(v)) for k, v in a.items()}
    return lib.ff_obdm_accumulate(None, B, int(nup), int(ndn), ptr["x"], ptr["rprime"], ptr["logp"], ptr["sign"], ptr["logp_moved"],
                                  ptr["sign_moved"], float(sigma), int(nshells), None if "acc" in null else _p(acc),
                                  None if "workspace" in null else _p(ws))


def sign_call(lib, z, nup, ndn, tab_up=None, tab_dn=None, wstate=None):
    z = np.ascontiguousarray(z, dtype=np.float64)
    out = np.full(z.shape[0], 7.0)
    tu = np.ascontiguousarray(_tab(nup, tab_up), dtype=np.int32) if nup else None
    td = np.ascontiguousarray(_tab(ndn, tab_dn), dtype=np.int32) if ndn else None
    ws = None if wstate is None else np.ascontiguousarray(wstate, dtype=np.int32)
    st = lib.ff_slater_sign(None, z.shape[0], int(nup), int(ndn), _p(tu), _p(td), _p(ws), _p(z), _p(out))
    assert st == 0, lib.ff_last_error()
    return out


def inputs(seed, B, nup, ndn, sigma=1.0):
    """seeded synthetic inputs of ff_obdm_accumulate: walkers, r', log-densities and signs (a few exact zeros among sign_moved)"""
    rng = np.random.default_rng(seed)
    n = nup + ndn
    x = rng.standard_normal((B, n, 2)) * 1.2
    rp = rng.standard_normal((B, 2, 2)) * sigma
    logp = -8.0 + 2.0 * rng.standard_normal(B)
    lpm = logp[:, None] + 1.5 * rng.standard_normal((B, n))
    sign = rng.choice([-1.0, 1.0], size=B)
    sgm = rng.choice([-1.0, 1.0, 0.0], size=(B, n), p=[0.48, 0.48, 0.04])
    return dict(x=x, rprime=rp, logp=logp, sign=sign, logp_moved=lpm, sign_moved=sgm)
