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

DensityMaps (below) is the two-dimensional counterpart: the lab-frame density rho(x, y) of each species and the pair densities in the
frame rotating with the reference particle, through ff_maps_accumulate (csrc/ff_maps.h, include/fermiflow_maps.h).
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


# ---- two-dimensional density maps (include/fermiflow_maps.h, csrc/ff_maps.h) ---------------------------------------------------
PLANES = ("up", "down", "uu", "ud", "du", "dd")
MAPS_MAX_BINS = 128


class DensityMaps:
    """Two-dimensional density maps of the physical walkers (d = 2), accumulated on the device as integer histograms over the window
    [-extent, extent)^2 cut into nbins x nbins cells:

      up, down          the lab-frame density rho(x, y) of each spin species;
      uu, ud, du, dd    the pair density of every ORDERED pair (i, j), i != j, in the frame that rotates with the reference particle i
                        (first letter: its species), in which i sits on the positive first axis at (|x_i|, 0): the partner j (second
                        letter) is binned at (p, q) = (c x_j + s y_j, c y_j - s x_j), (c, s) = x_i / |x_i| (the identity at the origin).
                        In a rotationally symmetric trap this is where angular order (a Wigner molecule) shows; the reference particle
                        itself is not binned, its law in that frame is the radial density of Observables.

        maps = DensityMaps(nup, ndown, extent=6.0, nbins=128)
        model.density_maps = maps            # GSVMC / BetaVMC: every sweep feeds it with one launch, right after the flow pass
        ...
        x_mid, y_mid = maps.xy_mid(); rho = maps.density(); g = maps.pair_density()["ud"]      # [ix, iy]

    With nframes = K the object holds K such accumulators, one per frame of CNF.generate(z, nframes=K) (accumulate_frames).
    `accumulate(x, frame)` is one enqueue of ff_maps_accumulate on torch's current stream, no host read; the host reads the buffer only
    in counts() / density() / pair_density() / state_dict() / all_reduce_() / save_npz().  Counts only: the cells of a map are Poisson
    counts, the standard error of a cell is sqrt(count) (in the units of density(): sqrt(count) / (walkers cell_area)) -- no block
    errors are kept.  Every word is an integer: a result is bit-identical from run to run and additive over launches' grids and ranks.
    Slots per plane: the nbins^2 cells, then "overflow" (a finite sample outside the window) and "invalid" (a non-finite coordinate
    entered the sample).  Normalisation, on the host in fp64: value = count / (walkers cell_area), so the sum of value x cell_area over
    a plane is its samples per walker (nup, ndown; nup (nup - 1), nup ndown, ndown nup, ndown (ndown - 1)) minus its lost share."""

    def __init__(self, nup, ndown, extent=6.0, nbins=128, nframes=1, device=None):
        nup, ndown, nbins, nframes, extent = int(nup), int(ndown), int(nbins), int(nframes), float(extent)
        if nup < 0 or ndown < 0 or nup + ndown < 1:
            raise ValueError("DensityMaps: nup, ndown >= 0 and at least one particle")
        if not 1 <= nbins <= MAPS_MAX_BINS:
            raise ValueError(f"DensityMaps: 1 <= nbins <= {MAPS_MAX_BINS}")
        if not (extent > 0.0 and math.isfinite(extent)):
            raise ValueError("DensityMaps: extent must be positive and finite")
        if nframes < 1:
            raise ValueError("DensityMaps: nframes must be at least 1")
        if nup + ndown > 24:
            raise NotImplementedError("DensityMaps: n <= 24")
        self.nup, self.ndown, self.extent, self.nbins, self.nframes = nup, ndown, extent, nbins, nframes
        self._P = nbins * nbins + 2
        self._words = 2 + len(PLANES) * self._P          # include/fermiflow_maps.h: [calls, walkers | sum[6][P]]
        self._B = [None] * nframes                       # walkers per call of every frame (every call the same, as Observables)
        self._buf = None
        self._checked = False
        if device is not None:
            self._buf = torch.zeros(nframes, self._words, dtype=torch.int64, device=torch.device(device))

    @property
    def cell_area(self):
        return (2.0 * self.extent / self.nbins) ** 2

    def samples_per_walker(self):
        u, d = self.nup, self.ndown
        return dict(zip(PLANES, (u, d, u * (u - 1), u * d, d * u, d * (d - 1))))

    def _frame(self, frame):
        k = int(frame)
        if not 0 <= k < self.nframes:
            raise IndexError(f"DensityMaps: frame {frame} of {self.nframes}")
        return k

    # ---- device side -------------------------------------------------------------------------------------------------------
    def _check_x(self, x, who, lead=()):
        n = self.nup + self.ndown
        want = "(" + ", ".join([str(v) for v in lead] + ["B", str(n), "2"]) + ")"
        if x.dim() == len(lead) + 3 and x.shape[-1] == 3:
            raise ValueError(f"DensityMaps.{who}: maps are two-dimensional, x must be {want}, got {tuple(x.shape)}")
        if x.dim() != len(lead) + 3 or tuple(x.shape[:len(lead)]) != tuple(lead) or x.shape[-2] != n or x.shape[-1] != 2:
            raise ValueError(f"DensityMaps.{who}: x must be {want}, got {tuple(x.shape)}")

    def _launch(self, x, k):
        B = int(x.shape[0])
        if self._B[k] is not None and B != self._B[k]:
            raise ValueError(f"DensityMaps.accumulate: {B} walkers, the earlier calls of frame {k} had {self._B[k]}")
        if self._buf is None or self._buf.device != x.device:
            self._buf = torch.zeros(self.nframes, self._words, dtype=torch.int64, device=x.device) if self._buf is None else self._buf.to(x.device)
        lib = _lib.lib()
        if not self._checked:
            if lib.ff_maps_buffer_bytes(self.nbins) != 8 * self._words:
                raise RuntimeError("DensityMaps: the library lays the accumulator out differently (include/fermiflow_maps.h)")
            self._checked = True
        _lib.check(lib.ff_maps_accumulate(_lib.stream(), B, self.nup, self.ndown, _lib.ptr(x), self.extent, self.nbins,
                                          _lib.ptr(self._buf[k])), "ff_maps_accumulate")
        if B > 0:
            self._B[k] = B

    def accumulate(self, x, frame=0):
        """Add the walkers x (B, n, 2), fp64 on the device, to the maps of `frame`: one launch on the current stream, no host read."""
        k = self._frame(frame)
        x = _lib.dev(x, name="x")
        self._check_x(x, "accumulate")
        self._launch(x, k)

    def accumulate_frames(self, frames):
        """Add the trajectory frames (K, B, n, 2) of CNF.generate(z, nframes=K), K == nframes, frame k to the maps of frame k: K launches
        on the current stream, nothing is copied."""
        frames = _lib.dev(frames, name="frames")
        self._check_x(frames, "accumulate_frames", lead=(self.nframes,))
        for k in range(self.nframes):
            self._launch(frames[k], k)

    def reset(self):
        if self._buf is not None:
            self._buf.zero_()
        self._B = [None] * self.nframes

    def all_reduce_(self):
        """Sum the counts over the ranks of torch.distributed, as doubles through dist.all_reduce_sum_: exact below 2^53, and it raises
        if a count is not.  Call it once, when the run is over: the object then holds the totals of all ranks."""
        if self._buf is None:
            self._buf = torch.zeros(self.nframes, self._words, dtype=torch.int64)
        t = self._buf.to(torch.float64)
        D.all_reduce_sum_(t)
        if bool((t >= _EXACT).any()):
            raise OverflowError("DensityMaps.all_reduce_: a count reached 2^53, the sum over ranks as doubles would not be exact")
        self._buf.copy_(t.to(torch.int64))
        return self

    # ---- host side ---------------------------------------------------------------------------------------------------------
    def _host(self, k):
        a = np.zeros(self._words, dtype=np.int64) if self._buf is None else self._buf[k].cpu().numpy().astype(np.int64)
        return int(a[0]), int(a[1]), a[2:].reshape(len(PLANES), self._P)

    def counts(self, frame=0):
        """Raw counts on the host: {"up", ..., "dd": int64 (nbins, nbins) indexed [ix, iy]; "lost_up", ..., "lost_dd": (overflow,
        invalid); "calls", "walkers"}."""
        calls, walkers, s = self._host(self._frame(frame))
        nb = self.nbins
        out = {}
        for c, name in enumerate(PLANES):
            out[name] = s[c, :nb * nb].reshape(nb, nb).copy()
            out["lost_" + name] = (int(s[c, nb * nb]), int(s[c, nb * nb + 1]))
        out["calls"], out["walkers"] = calls, walkers
        return out

    def xy_mid(self):
        """(x_mid, y_mid): the cell centres along the two axes (first and second index of a plane)."""
        mid = -self.extent + (np.arange(self.nbins) + 0.5) * (2.0 * self.extent / self.nbins)
        return mid, mid.copy()

    def _normalised(self, frame, names):
        c = self.counts(frame)
        with np.errstate(divide="ignore", invalid="ignore"):
            return {name: c[name].astype(np.float64) / (float(c["walkers"]) * self.cell_area) for name in names}

    def density(self, frame=0):
        """{"up", "down"}: particles of the species per unit area at (x_mid[ix], y_mid[iy]); the Poisson error of a cell is
        sqrt(count) / (walkers cell_area)."""
        return self._normalised(frame, PLANES[:2])

    def pair_density(self, frame=0):
        """{"uu", "ud", "du", "dd"}: partners of the second species per unit area at (p, q) in the frame rotating with a reference
        particle of the first, summed over the reference particles."""
        return self._normalised(frame, PLANES[2:])

    def state_dict(self):
        acc = torch.zeros(self.nframes, self._words, dtype=torch.int64) if self._buf is None else self._buf.cpu().clone()
        return {"nup": self.nup, "ndown": self.ndown, "extent": self.extent, "nbins": self.nbins, "nframes": self.nframes, "acc": acc}

    def load_state_dict(self, st):
        for k in ("nup", "ndown", "extent", "nbins", "nframes"):
            if st[k] != getattr(self, k):
                raise ValueError(f"DensityMaps.load_state_dict: {k} = {st[k]!r}, this object has {getattr(self, k)!r}")
        acc = torch.as_tensor(st["acc"]).to(torch.int64)
        if tuple(acc.shape) != (self.nframes, self._words):
            raise ValueError(f"DensityMaps.load_state_dict: acc of shape {tuple(acc.shape)}, expected {(self.nframes, self._words)}")
        if self._buf is None:
            self._buf = torch.zeros(self.nframes, self._words, dtype=torch.int64)
        self._buf.copy_(acc.to(self._buf.device))
        self._B = [int(w) // int(c) if int(c) > 0 else None for c, w in zip(acc[:, 0], acc[:, 1])]

    def save_npz(self, path):
        """One .npz (what the drivers' --maps_out / --frames_maps_out write): x_mid, y_mid, the six normalised planes (nframes, nbins,
        nbins), counts_<plane>, lost_<plane> (nframes, 2), calls and walkers (nframes), cell_area and the settings."""
        x_mid, y_mid = self.xy_mid()
        cs = [self.counts(k) for k in range(self.nframes)]
        out = dict(x_mid=x_mid, y_mid=y_mid, cell_area=self.cell_area, calls=np.array([c["calls"] for c in cs], dtype=np.int64),
                   walkers=np.array([c["walkers"] for c in cs], dtype=np.int64), nup=self.nup, ndown=self.ndown, extent=self.extent,
                   nbins=self.nbins, nframes=self.nframes)
        for name in PLANES:
            cnt = np.stack([c[name] for c in cs])
            with np.errstate(divide="ignore", invalid="ignore"):
                out[("rho_" if name in PLANES[:2] else "g_") + name] = cnt.astype(np.float64) / (out["walkers"][:, None, None].astype(np.float64) * self.cell_area)
            out["counts_" + name] = cnt
            out["lost_" + name] = np.array([c["lost_" + name] for c in cs], dtype=np.int64)
        np.savez(path, **out)
