"""Observables of the physical walkers, accumulated on the device: the radial density of each spin species and the
pair-distance distribution of each pair of species, averaged over many sweeps.

    obs = Observables(nup, ndown, dim=2, rmax=6.0, nbins=240)
    model.observables = obs              # GSVMC / BetaVMC: every sweep feeds it with one launch, right after the flow pass
    ...
    r, n_up, n_dn, err_up, err_dn = obs.radial_density()

`accumulate(x)` is one enqueue of ff_observe_accumulate (csrc/ff_observe.h) on torch's current stream: integer histograms in a
device buffer, no host read.  The host reads the buffer only in counts() / radial_density() / pair_distribution() /
state_dict() / all_reduce_().  Counts are integers, so a result is bit-identical from run to run and does not depend on how
the walkers are spread over launches' grids or over ranks.

Slots per class: nbins bins of width rmax / nbins, then "overflow" (finite r >= rmax) and "invalid" (r not finite: walkers
whose integration failed carry NaN).  Normalisation, on the host in fp64: value_k = sum_k / (walkers V_k) with V_k the volume
of shell k (pi (r_{k+1}^2 - r_k^2) in d = 2, 4 pi / 3 (r_{k+1}^3 - r_k^3) in d = 3), so sum_k n_s(r_k) V_k is the particle number
of species s minus its overflow and invalid share, and the same sum of a pair distribution is the number of pairs of the class.
Errors are block standard errors with one block per call (per rank and call after all_reduce_()); NaN below two calls.
"""
import math

import numpy as np
import torch

from . import _lib
from . import dist as D

CLASSES = ("up", "down", "uu", "ud", "dd")
MAX_BINS = 1024
_EXACT = float(2 ** 53)


class Observables:
    def __init__(self, nup, ndown, dim=2, rmax=6.0, nbins=240, device=None):
        nup, ndown, dim, nbins, rmax = int(nup), int(ndown), int(dim), int(nbins), float(rmax)
        if nup < 0 or ndown < 0 or nup + ndown < 1:
            raise ValueError("Observables: nup, ndown >= 0 and at least one particle")
        if dim not in (2, 3):
            raise ValueError("Observables: dim must be 2 or 3")
        if not 1 <= nbins <= MAX_BINS:
            raise ValueError(f"Observables: 1 <= nbins <= {MAX_BINS}")
        if not (rmax > 0.0 and math.isfinite(rmax)):
            raise ValueError("Observables: rmax must be positive and finite")
        if nup + ndown > 24 or (nup + ndown) * dim > 60:
            raise NotImplementedError("Observables: n <= 24 and n * dim <= 60")
        self.nup, self.ndown, self.dim, self.rmax, self.nbins = nup, ndown, dim, rmax, nbins
        self._S = len(CLASSES) * (nbins + 2)
        self._words = 3 + 3 * self._S          # include/fermiflow.h: [calls, walkers | sum | sumsq | scratch, ticket]
        self._B = None                         # walkers per call (every call the same: equal blocks)
        self._buf = None
        if device is not None:
            self._buf = torch.zeros(self._words, dtype=torch.int64, device=torch.device(device))

    # ---- device side -------------------------------------------------------------------------------------------------------
    def accumulate(self, x):
        """Add the walkers x (B, n, dim), fp64 on the device, to the histograms: one launch on the current stream, no host read."""
        x = _lib.dev(x, name="x")
        if x.dim() != 3 or x.shape[1] != self.nup + self.ndown or x.shape[2] != self.dim:
            raise ValueError(f"Observables.accumulate: x must be (B, {self.nup + self.ndown}, {self.dim}), got {tuple(x.shape)}")
        B = int(x.shape[0])
        if self._B is not None and B != self._B:
            raise ValueError(f"Observables.accumulate: {B} walkers, the earlier calls had {self._B} (the block errors need equal blocks)")
        if self._buf is None or self._buf.device != x.device:
            self._buf = torch.zeros(self._words, dtype=torch.int64, device=x.device) if self._buf is None else self._buf.to(x.device)
        lib = _lib.lib()
        if self._B is None and lib.ff_observe_buffer_bytes(self.nbins) != 8 * self._words:
            raise RuntimeError("Observables: the library lays the accumulator out differently (include/fermiflow.h)")
        _lib.check(lib.ff_observe_accumulate(_lib.stream(), B, self.nup, self.ndown, self.dim, _lib.ptr(x), self.rmax,
                                             self.nbins, _lib.ptr(self._buf)), "ff_observe_accumulate")
        if B > 0:
            self._B = B                        # (only a call that counted fixes the block size)

    def reset(self):
        if self._buf is not None:
            self._buf.zero_()
        self._B = None

    def all_reduce_(self):
        """Sum the counts over the ranks of torch.distributed (sum, sumsq, calls, walkers), as doubles through dist.all_reduce_sum_:
        exact below 2^53, and it raises if a count is not.  Call it once, when the run is over: the object then holds the totals of
        all ranks, with one block per rank and call."""
        if self._buf is None:
            self._buf = torch.zeros(self._words, dtype=torch.int64)
        n = 2 + 2 * self._S
        t = self._buf[:n].to(torch.float64)
        D.all_reduce_sum_(t)
        if bool((t >= _EXACT).any()):
            raise OverflowError("Observables.all_reduce_: a count reached 2^53, the sum over ranks as doubles would not be exact")
        self._buf[:n] = t.to(torch.int64)
        return self

    # ---- host side ---------------------------------------------------------------------------------------------------------
    def _host(self):
        n = 2 + 2 * self._S
        a = np.zeros(n, dtype=np.int64) if self._buf is None else self._buf[:n].cpu().numpy().astype(np.int64)
        S, nb = self._S, self.nbins + 2
        return int(a[0]), int(a[1]), a[2:2 + S].reshape(len(CLASSES), nb), a[2 + S:2 + 2 * S].reshape(len(CLASSES), nb)

    def counts(self):
        """Raw counts on the host: {"up", "down", "uu", "ud", "dd": int64 (nbins + 2,) -- the bins, overflow, invalid --, "calls", "walkers"}."""
        calls, walkers, s, _ = self._host()
        out = {name: s[c].copy() for c, name in enumerate(CLASSES)}
        out["calls"], out["walkers"] = calls, walkers
        return out

    def shell_volumes(self):
        e = np.linspace(0.0, self.rmax, self.nbins + 1)
        e[-1] = self.rmax
        return (math.pi * (e[1:] ** 2 - e[:-1] ** 2)) if self.dim == 2 else (4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3))

    def r_mid(self):
        return (np.arange(self.nbins) + 0.5) * (self.rmax / self.nbins)

    def _normalised(self):
        calls, walkers, s, q = self._host()
        V = self.shell_volumes()
        s = s[:, :self.nbins].astype(np.float64)
        q = q[:, :self.nbins].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = s / (float(walkers) * V)
            if calls >= 2:
                m = float(calls)
                var = np.maximum(q / m - (s / m) ** 2, 0.0) * (m / (m - 1.0))
                err = np.sqrt(var / m) / ((float(walkers) / m) * V)
            else:
                err = np.full_like(val, np.nan)
        return val, err

    def radial_density(self):
        """r_mid, n_up, n_dn, err_up, err_dn -- particles of the species per unit volume at radius r."""
        v, e = self._normalised()
        return self.r_mid(), v[0], v[1], e[0], e[1]

    def pair_distribution(self):
        """r_mid, uu, ud, dd, err_uu, err_ud, err_dd -- pairs of the class per unit volume at distance r."""
        v, e = self._normalised()
        return self.r_mid(), v[2], v[3], v[4], e[2], e[3], e[4]

    def state_dict(self):
        n = 2 + 2 * self._S
        acc = torch.zeros(n, dtype=torch.int64) if self._buf is None else self._buf[:n].cpu().clone()
        return {"nup": self.nup, "ndown": self.ndown, "dim": self.dim, "rmax": self.rmax, "nbins": self.nbins, "acc": acc}

    def load_state_dict(self, st):
        for k in ("nup", "ndown", "dim", "rmax", "nbins"):
            if st[k] != getattr(self, k):
                raise ValueError(f"Observables.load_state_dict: {k} = {st[k]!r}, this object has {getattr(self, k)!r}")
        acc = torch.as_tensor(st["acc"]).to(torch.int64).reshape(-1)
        n = 2 + 2 * self._S
        if acc.numel() != n:
            raise ValueError(f"Observables.load_state_dict: {acc.numel()} words, expected {n}")
        if self._buf is None:
            self._buf = torch.zeros(self._words, dtype=torch.int64)
        self._buf.zero_()
        self._buf[:n] = acc.to(self._buf.device)
        calls, walkers = int(acc[0]), int(acc[1])
        self._B = walkers // calls if calls > 0 else None

    def save_npz(self, path):
        """r_mid, densities, pair distributions, their errors and the raw counts in one .npz (what the drivers' --observe_out writes)."""
        r, n_up, n_dn, e_up, e_dn = self.radial_density()
        _, uu, ud, dd, e_uu, e_ud, e_dd = self.pair_distribution()
        c = self.counts()
        np.savez(path, r_mid=r, n_up=n_up, n_dn=n_dn, err_up=e_up, err_dn=e_dn, g_uu=uu, g_ud=ud, g_dd=dd, err_uu=e_uu, err_ud=e_ud,
                 err_dd=e_dd, shell_volumes=self.shell_volumes(), calls=c["calls"], walkers=c["walkers"],
                 nup=self.nup, ndown=self.ndown, dim=self.dim, rmax=self.rmax, nbins=self.nbins,
                 **{"counts_" + name: c[name] for name in CLASSES})
