"""TEST-ONLY: a numpy restatement of the density-map definitions of ff_maps_accumulate (include/fermiflow_maps.h), written from the
definitions and not from the kernel, and ctypes access to the accumulator of the host-simulated kernel.  The product package never
imports this."""
import ctypes as C

import numpy as np

PLANES = ("up", "down", "uu", "ud", "du", "dd")


def species(nup, n):
    return [np.arange(0, nup), np.arange(nup, n)]


def samples(x, nup):
    """The six planes' samples of walkers x (B, n, 2): a list of six (p, q, ok, rho2) tuples of flat arrays.  ok: every coordinate
    that enters the sample (and the reference particle's rho) is finite; rho2: x_i^2 + y_i^2 of the reference particle (lab: 1)."""
    x = np.asarray(x, dtype=np.float64)
    B, n, d = x.shape
    assert d == 2
    sp = species(nup, n)
    fin = np.isfinite(x).all(-1)                              # (B, n)
    out = []
    for s in (0, 1):
        i = sp[s]
        out.append((x[:, i, 0].reshape(-1), x[:, i, 1].reshape(-1), fin[:, i].reshape(-1), np.ones(B * len(i))))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rho2 = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]
        rho = np.sqrt(rho2)
        zero = rho == 0.0
        c = np.where(zero, 1.0, x[..., 0] / np.where(zero, 1.0, rho))
        s_ = np.where(zero, 0.0, x[..., 1] / np.where(zero, 1.0, rho))
        okr = fin & np.isfinite(rho)
        for si in (0, 1):
            for sj in (0, 1):
                ii, jj = np.meshgrid(sp[si], sp[sj], indexing="ij")
                keep = ii != jj
                ii, jj = ii[keep], jj[keep]                   # every ordered pair, i != j
                p = c[:, ii] * x[:, jj, 0] + s_[:, ii] * x[:, jj, 1]
                q = c[:, ii] * x[:, jj, 1] - s_[:, ii] * x[:, jj, 0]
                ok = okr[:, ii] & fin[:, jj]
                out.append((p.reshape(-1), q.reshape(-1), ok.reshape(-1), rho2[:, ii].reshape(-1)))
    return out


def slots(p, q, ok, extent, nbins):
    scale = nbins / (2.0 * extent)
    s = np.full(p.shape, nbins * nbins + 1, dtype=np.int64)   # invalid
    with np.errstate(invalid="ignore", over="ignore"):
        good = ok & np.isfinite(p) & np.isfinite(q)
        a, b = (p + extent) * scale, (q + extent) * scale
        inside = good & (a >= 0.0) & (a < nbins) & (b >= 0.0) & (b < nbins)
    s[good & ~inside] = nbins * nbins                         # overflow
    s[inside] = a[inside].astype(np.int64) * nbins + b[inside].astype(np.int64)
    return s


def histogram(x, nup, extent, nbins):
    """(6, nbins^2 + 2) int64 counts of one call."""
    P = nbins * nbins + 2
    return np.stack([np.bincount(slots(p, q, ok, extent, nbins), minlength=P) for p, q, ok, _ in samples(x, nup)]).astype(np.int64)


def edge_samples(x, nup, extent, nbins, tol=1e-9):
    """Samples whose a or b lies within `tol` of an integer, plus the pairs whose rho^2 is 0 or subnormal.  Device code is compiled
    with FMA contraction: the rotation's rounding moves a or b by at most a few tens of eps 2L scale (under 1e-12 at 128 bins), so
    only such samples may change slot (each one moves two slots by one)."""
    scale, k = nbins / (2.0 * extent), 0
    tiny = np.finfo(np.float64).tiny
    for plane, (p, q, ok, rho2) in enumerate(samples(x, nup)):
        with np.errstate(invalid="ignore", over="ignore"):
            good = ok & np.isfinite(p) & np.isfinite(q)
            a, b = (p[good] + extent) * scale, (q[good] + extent) * scale
            near = lambda v: (np.abs(v - np.rint(v)) < tol) & (v > -1.0) & (v < nbins + 1.0)
            k += int((near(a) | near(b)).sum())
            if plane >= 2:
                k += int((ok & (rho2 < tiny)).sum())
    return k


def samples_per_walker(nup, ndn):
    return np.array([nup, ndn, nup * (nup - 1), nup * ndn, ndn * nup, ndn * (ndn - 1)], dtype=np.int64)


# ---- the accumulator as the C ABI lays it out: uint64 words [calls, walkers | sum[6][P]]
def new_buffer(lib, nbins):
    nb = lib.ff_maps_buffer_bytes(int(nbins))
    assert nb == 8 * (2 + 6 * (nbins * nbins + 2))
    return np.zeros(nb // 8, dtype=np.uint64)


def split(acc, nbins):
    a = np.asarray(acc).astype(np.int64)
    return dict(calls=int(a[0]), walkers=int(a[1]), sum=a[2:].reshape(6, nbins * nbins + 2))


def accumulate(lib, x, nup, ndn, extent, nbins, acc, B=None, x_null=False, acc_null=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    B = x.shape[0] if B is None else B
    return lib.ff_maps_accumulate(None, B, int(nup), int(ndn), None if x_null else x.ctypes.data_as(C.c_void_p), float(extent), int(nbins),
                                  None if acc_null else acc.ctypes.data_as(C.c_void_p))
