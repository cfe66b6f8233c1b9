"""TEST-ONLY: a numpy restatement of the histogram definitions of ff_observe_accumulate (include/fermiflow.h), and ctypes access to
the accumulator of the host-simulated kernel.  The product package never imports this."""
import ctypes as C

import numpy as np

CLASSES = ("up", "down", "uu", "ud", "dd")


def distances(delta):
    """r = sqrt(sum_k delta_k^2) in fp64; finite components whose squares overflow are summed again scaled by 2^-512 (exact)."""
    delta = np.asarray(delta, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.sqrt((delta ** 2).sum(-1))
        fix = ~np.isfinite(r) & np.isfinite(delta).all(-1)
        if fix.any():
            r[fix] = np.sqrt(((delta[fix] * 2.0 ** -512) ** 2).sum(-1)) * 2.0 ** 512
    return r


def samples(x, nup):
    """The five classes' samples of walkers x (B, n, d): a list of five flat arrays of distances."""
    x = np.asarray(x, dtype=np.float64)
    B, n, d = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        rad = distances(x)                                    # (B, n)
        out = [rad[:, :nup].reshape(-1), rad[:, nup:].reshape(-1)]
        i, j = np.triu_indices(n, 1)
        pr = distances(x[:, i, :] - x[:, j, :])               # (B, npairs)
    cls = np.where(j < nup, 0, np.where(i < nup, 1, 2))
    for c in range(3):
        out.append(pr[:, cls == c].reshape(-1))
    return out


def slots(r, rmax, nbins):
    r = np.asarray(r, dtype=np.float64)
    s = np.full(r.shape, nbins + 1, dtype=np.int64)           # invalid
    fin = np.isfinite(r)
    s[fin & (r >= rmax)] = nbins                              # overflow
    ok = fin & (r < rmax)
    s[ok] = np.minimum((r[ok] * (nbins / rmax)).astype(np.int64), nbins - 1)
    return s


def histogram(x, nup, rmax, nbins):
    """(5, nbins + 2) int64 counts of one call."""
    return np.stack([np.bincount(slots(r, rmax, nbins), minlength=nbins + 2) for r in samples(x, nup)]).astype(np.int64)


def edge_samples(x, nup, rmax, nbins, tol=1e-9):
    """Samples whose r * nbins / rmax lies within `tol` of an integer: device code is compiled with FMA contraction, so such a sample
    may land in either neighbouring bin (each one moves two slots by one)."""
    k = 0
    for r in samples(x, nup):
        r = r[np.isfinite(r)]
        q = r[r < rmax * (1.0 + 1e-12)] * (nbins / rmax)
        k += int((np.abs(q - np.rint(q)) < tol).sum())
    return k


def pair_counts(nup, ndn):
    """samples per walker of the five classes"""
    return np.array([nup, ndn, nup * (nup - 1) // 2, nup * ndn, ndn * (ndn - 1) // 2], dtype=np.int64)


# ---- the accumulator as the C ABI lays it out: uint64 words [calls, walkers | sum | sumsq | scratch (S words + ticket)]
def new_buffer(lib, nbins):
    nb = lib.ff_observe_buffer_bytes(int(nbins))
    assert nb == 8 * (3 + 15 * (nbins + 2))
    return np.zeros(nb // 8, dtype=np.uint64)


def split(acc, nbins):
    S = 5 * (nbins + 2)
    a = np.asarray(acc).astype(np.int64)
    return dict(calls=int(a[0]), walkers=int(a[1]), sum=a[2:2 + S].reshape(5, nbins + 2), sumsq=a[2 + S:2 + 2 * S].reshape(5, nbins + 2),
                scratch=a[2 + 2 * S:])


def accumulate(lib, x, nup, ndn, rmax, nbins, acc, B=None, d=None, x_null=False, acc_null=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    B = x.shape[0] if B is None else B
    d = x.shape[2] if d is None else d
    return lib.ff_observe_accumulate(None, B, int(nup), int(ndn), int(d), None if x_null else x.ctypes.data_as(C.c_void_p),
                                     rmax, int(nbins), None if acc_null else acc.ctypes.data_as(C.c_void_p))
