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

OneBodyDensityMatrix (at the end) is the off-diagonal one: the one-body reduced density matrix in the oscillator basis from
wave-function ratios with one particle moved -- natural occupations, n(k) -- through ff_slater_sign and ff_obdm_accumulate
(csrc/ff_obdm.h, include/fermiflow_obdm.h).

EnergyParts (last) splits the energy: kinetic energy by two estimators, trap energy and the Coulomb repulsion by spin pair, their
covariance, the virial residual and the energy of every many-body state, through ff_energy_parts_accumulate (csrc/ff_energy_parts.h,
include/fermiflow_energy.h).
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


# ---- one-body density matrix in the oscillator basis (include/fermiflow_obdm.h, csrc/ff_obdm.h) ----------------------------------
OBDM_MAX_SHELLS = 8
_OBDM_HEAD = 5                 # FF_OBDM_HEAD: calls, walkers, invalid[2], ticket
OBDM_MAX_MOVED = 2 ** 22       # walkers of the moved batch of one measure()


def ho2d_degrees(nshells):
    """(nx, ny) of the first nshells (nshells + 1) / 2 orbitals in the HO2D list order."""
    return [(nx, N - nx) for N in range(int(nshells)) for nx in range(N + 1)]


def ho2d_basis(nshells, x, y):
    """phi_k(x, y) = pi^-1/2 exp(-r^2 / 2) h_nx(x) h_ny(y) of the basis orbitals on the host: (nb, *shape) for broadcastable x, y."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))

    def herm(t):
        h = [np.ones_like(t), math.sqrt(2.0) * t]
        for m in range(1, 7):
            h.append(math.sqrt(2.0 / (m + 1)) * t * h[m] - math.sqrt(m / (m + 1.0)) * h[m - 1])
        return h
    hx, hy = herm(x), herm(y)
    g = np.exp(-0.5 * (x * x + y * y)) / math.sqrt(math.pi)
    return np.stack([g * hx[nx] * hy[ny] for nx, ny in ho2d_degrees(nshells)])


class OneBodyDensityMatrix:
    """The one-body reduced density matrix rho_1(r, r') of each spin species (d = 2) in the basis of the first
    nb = nshells (nshells + 1) / 2 harmonic-oscillator orbitals, rho^s_ac = <phi_a| rho_1^s |phi_c>, accumulated on the device.  From it:
    the natural occupation numbers (occupations()), the momentum distribution n(k) (momentum_distribution()) and the density
    (density()).  tr rho^s -> N_s as the basis grows.

        obdm = OneBodyDensityMatrix(nup, ndown, nshells=4)
        model.obdm = obdm                    # GSVMC / BetaVMC: every `every`-th sweep measures, right after the local-energy pass
        ...
        occ, coeff = obdm.occupations()["up"]; n_k = obdm.momentum_distribution(kx, ky)["up"]

    Estimator (include/fermiflow_obdm.h): for every walker x and species s ONE point r' is drawn from N(0, sigma^2 I); with x^(i) = x
    with particle i of s moved to r' and q_i = psi(x^(i)) / psi(x), the walker adds (A C^T + C A^T) / 2, A_a = sum_i phi_a(x_i) q_i,
    C_c = phi_c(r') / g(r').  The ratios need the flow integrated backwards for the n moved copies of every walker and the sign of the
    Slater determinants (ff_slater_sign): measure() costs about n local backward flows per walker it takes, so `stride` thins the
    walkers (0, stride, 2 stride, ...: a sorted walker_state stays sorted and keeps its proportions) and `every` the sweeps.

    measure() and accumulate_raw() enqueue on torch's current stream and read nothing on the host; r' comes from a private
    torch.Generator on the walkers' device, seeded with `seed` -- torch's CPU generator is never touched.  The host reads the buffer
    only in counts() / matrix() / ... / state_dict() / all_reduce_() / save_npz().  Every call must bring the same number of walkers:
    one call is one block of the block standard error (matrix_err(); NaN below two calls).  A result is bit-identical from run to run
    on one device.  all_reduce_() adds the sums of the ranks as doubles, once, when the run is over: one block per rank and call,
    and the sum is NOT bit-identical across rank counts (the counts are exact)."""

    def __init__(self, nup, ndown, nshells=4, sigma=1.0, every=1, stride=1, seed=0, device=None):
        nup, ndown, nshells, sigma, every, stride, seed = int(nup), int(ndown), int(nshells), float(sigma), int(every), int(stride), int(seed)
        if nup < 0 or ndown < 0 or nup + ndown < 1:
            raise ValueError("OneBodyDensityMatrix: nup, ndown >= 0 and at least one particle")
        if not 1 <= nshells <= OBDM_MAX_SHELLS:
            raise ValueError(f"OneBodyDensityMatrix: 1 <= nshells <= {OBDM_MAX_SHELLS}")
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError("OneBodyDensityMatrix: sigma must be positive and finite")
        if every < 1 or stride < 1:
            raise ValueError("OneBodyDensityMatrix: every and stride must be at least 1")
        if nup + ndown > 24 or nup > 12 or ndown > 12:
            raise NotImplementedError("OneBodyDensityMatrix: n <= 24 and at most 12 particles per species")
        self.nup, self.ndown, self.nshells, self.sigma, self.every, self.stride, self.seed = nup, ndown, nshells, sigma, every, stride, seed
        self.nb = nshells * (nshells + 1) // 2
        self._E = 2 * self.nb * self.nb
        self._words = _OBDM_HEAD + 2 * self._E      # include/fermiflow_obdm.h: [calls, walkers, invalid[2], ticket | sum | sumsq]
        self._B = None
        self._buf = None
        self._ws = None
        self._gen = None
        self._cols = None
        self._sweeps = 0
        self._checked = False
        self.last = None
        if device is not None:
            self._buf = torch.zeros(self._words, dtype=torch.int64, device=torch.device(device))

    # ---- device side -------------------------------------------------------------------------------------------------------
    def accumulate_raw(self, x, rprime, logp, sign, logp_moved, sign_moved):
        """One ff_obdm_accumulate on the current stream: x (B, n, 2), rprime (B, 2, 2), logp (B), sign (B), logp_moved (B, n),
        sign_moved (B, n), fp64 on the device.  One call is one block."""
        from . import native
        x = _lib.dev(x, name="x")
        B = int(x.shape[0])
        if self._B is not None and B != self._B:
            raise ValueError(f"OneBodyDensityMatrix: {B} walkers, the earlier calls had {self._B} (the block errors need equal blocks)")
        if self._buf is None or self._buf.device != x.device:
            self._buf = torch.zeros(self._words, dtype=torch.int64, device=x.device) if self._buf is None else self._buf.to(x.device)
        lib = _lib.lib()
        if not self._checked:
            if lib.ff_obdm_buffer_bytes(self.nshells) != 8 * self._words:
                raise RuntimeError("OneBodyDensityMatrix: the library lays the accumulator out differently (include/fermiflow_obdm.h)")
            self._checked = True
        need = max(1, lib.ff_obdm_workspace_bytes(B, self.nshells) // 8)
        if self._ws is None or self._ws.device != x.device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float64, device=x.device)
        native.obdm_accumulate(self.nup, self.ndown, x, rprime, logp, sign, logp_moved, sign_moved, self.sigma, self.nshells, self._buf, self._ws)
        if B > 0:
            self._B = B

    def measure(self, net, tab_up, tab_dn, x, z, logp, t_span, rtol, atol, walker_state=None):
        """The whole pipeline for the walkers x (B, n, 2) of a sweep, z = z(t0) their base walkers and logp = log p(x): take every
        `stride`-th walker, draw r', build the moved batch (B' n, n, 2), integrate it backwards (native.cnf_delta_logp), evaluate
        log-density and sign of the moved and the unmoved base walkers, accumulate.  Nothing is read on the host.  `last` keeps
        {rprime, logp_moved, sign_moved, sign, logp} of this call (the walkers it took) on the device."""
        from . import native
        n = self.nup + self.ndown
        x = _lib.dev(x, name="x")
        if x.dim() != 3 or x.shape[1] != n or x.shape[2] != 2:
            raise ValueError(f"OneBodyDensityMatrix.measure: x must be (B, {n}, 2), got {tuple(x.shape)}")
        s = self.stride
        xs, zs, lps = x[::s].contiguous(), z[::s].contiguous(), logp[::s].contiguous()
        ws = None if walker_state is None else walker_state[::s].contiguous()
        B, dev = int(xs.shape[0]), x.device
        if B * n > OBDM_MAX_MOVED:
            raise ValueError(f"OneBodyDensityMatrix.measure: a moved batch of {B * n} walkers (more than 2^22): raise `stride` (now {s})")
        if self._gen is None or self._gen.device != dev:
            self._gen = torch.Generator(device=dev)
            self._gen.manual_seed(self.seed)
            ar = torch.arange(n, device=dev)
            self._cols = (ar, (ar >= self.nup).to(torch.int64))          # particle -> its row, its species
        rp = torch.randn(B, 2, 2, generator=self._gen, device=dev, dtype=torch.float64) * self.sigma
        ar, species = self._cols
        xm = xs[:, None].expand(B, n, n, 2).clone()                      # [walker, moved particle, row, coordinate]
        xm[:, ar, ar] = rp[:, species]
        xm = xm.view(B * n, n, 2)
        wsm = None if ws is None else ws[:, None].expand(B, n).reshape(-1)      # walker-major: a sorted state list stays sorted
        zm, dl = native.cnf_delta_logp(net, xm, float(t_span[0]), float(t_span[1]), rtol, atol)
        lpm = (native.logprob(tab_up, tab_dn, self.nup, self.ndown, zm, wsm) - dl).view(B, n)
        sgm = native.slater_sign(tab_up, tab_dn, self.nup, self.ndown, zm, wsm).view(B, n)
        sg = native.slater_sign(tab_up, tab_dn, self.nup, self.ndown, zs, ws)
        self.accumulate_raw(xs, rp, lps, sg, lpm, sgm)
        self.last = {"rprime": rp, "logp_moved": lpm, "sign_moved": sgm, "sign": sg, "logp": lps}

    def on_sweep(self, net, tab_up, tab_dn, x, z, logp, t_span, rtol, atol, walker_state=None):
        """The sweeps' hook: measure() on every `every`-th call."""
        k, self._sweeps = self._sweeps, self._sweeps + 1
        if k % self.every == 0:
            self.measure(net, tab_up, tab_dn, x, z, logp, t_span, rtol, atol, walker_state)

    def reset(self):
        if self._buf is not None:
            self._buf.zero_()
        self._B, self._sweeps = None, 0

    def all_reduce_(self):
        """Sum calls, walkers, invalid (exact below 2^53, it raises otherwise) and sum, sumsq (doubles) over the ranks of
        torch.distributed through dist.all_reduce_sum_.  Call it once, when the run is over."""
        if self._buf is None:
            self._buf = torch.zeros(self._words, dtype=torch.int64)
        t = torch.cat([self._buf[:4].to(torch.float64), self._buf[_OBDM_HEAD:].view(torch.float64)])
        D.all_reduce_sum_(t)
        if bool((t[:4] >= _EXACT).any()):
            raise OverflowError("OneBodyDensityMatrix.all_reduce_: a count reached 2^53, the sum over ranks as doubles would not be exact")
        self._buf[:4] = t[:4].to(torch.int64)
        self._buf[_OBDM_HEAD:] = t[4:].view(torch.int64)
        return self

    # ---- host side ---------------------------------------------------------------------------------------------------------
    def _host(self):
        a = np.zeros(self._words, dtype=np.int64) if self._buf is None else self._buf.cpu().numpy().astype(np.int64)
        f = a[_OBDM_HEAD:].view(np.float64)
        nb, E = self.nb, self._E
        return int(a[0]), int(a[1]), (int(a[2]), int(a[3])), f[:E].reshape(2, nb, nb).copy(), f[E:].reshape(2, nb, nb).copy()

    def counts(self):
        """{"calls", "walkers", "invalid_up", "invalid_down": samples (walker, particle) that were left out, "samples_up",
        "samples_down": walkers x particles of the species}."""
        calls, walkers, inv, _, _ = self._host()
        return {"calls": calls, "walkers": walkers, "invalid_up": inv[0], "invalid_down": inv[1],
                "samples_up": walkers * self.nup, "samples_down": walkers * self.ndown}

    def matrix(self):
        """{"up", "down"}: rho^s (nb, nb), symmetric."""
        _, walkers, _, s, _ = self._host()
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"up": s[0] / float(walkers), "down": s[1] / float(walkers)}

    def matrix_err(self):
        """{"up", "down"}: the block standard error of every entry, one block per call (NaN below two calls)."""
        calls, walkers, _, s, q = self._host()
        with np.errstate(divide="ignore", invalid="ignore"):
            if calls >= 2:
                m = float(calls)
                var = np.maximum(q / m - (s / m) ** 2, 0.0) * (m / (m - 1.0))
                err = np.sqrt(var / m) / (float(walkers) / m)
            else:
                err = np.full_like(s, np.nan)
        return {"up": err[0], "down": err[1]}

    def occupations(self):
        """{"up", "down"}: (occ (nb,) the natural occupation numbers in descending order, coeff (nb, nb): column k holds the
        coefficients of natural orbital k in the basis) -- numpy.linalg.eigh of rho^s."""
        out = {}
        for name, rho in self.matrix().items():
            w, v = np.linalg.eigh(rho)
            out[name] = (w[::-1].copy(), v[:, ::-1].copy())
        return out

    def degrees(self):
        return ho2d_degrees(self.nshells)

    def momentum_distribution(self, kx, ky):
        """{"up", "down"}: n_s(k) = sum_ac rho_ac cos(pi (N_c - N_a) / 2) phi_a(k) phi_c(k), N = nx + ny (an oscillator
        eigenfunction is its own Fourier transform up to (-i)^N); its integral over the plane is tr rho^s."""
        phi = ho2d_basis(self.nshells, kx, ky)
        N = np.array([nx + ny for nx, ny in self.degrees()])
        ph = np.cos(0.5 * math.pi * (N[None, :] - N[:, None]))
        return {name: np.einsum("ac,a...,c...->...", rho * ph, phi, phi) for name, rho in self.matrix().items()}

    def density(self, x, y):
        """{"up", "down"}: rho_s(r) = sum_ac rho_ac phi_a(r) phi_c(r), the density as the basis resolves it."""
        phi = ho2d_basis(self.nshells, x, y)
        return {name: np.einsum("ac,a...,c...->...", rho, phi, phi) for name, rho in self.matrix().items()}

    def state_dict(self):
        acc = torch.zeros(self._words, dtype=torch.int64) if self._buf is None else self._buf.cpu().clone()
        return {"nup": self.nup, "ndown": self.ndown, "nshells": self.nshells, "sigma": self.sigma, "acc": acc}

    def load_state_dict(self, st):
        for k in ("nup", "ndown", "nshells", "sigma"):
            if st[k] != getattr(self, k):
                raise ValueError(f"OneBodyDensityMatrix.load_state_dict: {k} = {st[k]!r}, this object has {getattr(self, k)!r}")
        acc = torch.as_tensor(st["acc"]).to(torch.int64).reshape(-1)
        if acc.numel() != self._words:
            raise ValueError(f"OneBodyDensityMatrix.load_state_dict: {acc.numel()} words, expected {self._words}")
        if self._buf is None:
            self._buf = torch.zeros(self._words, dtype=torch.int64)
        self._buf.copy_(acc.to(self._buf.device))
        calls, walkers = int(acc[0]), int(acc[1])
        self._B = walkers // calls if calls > 0 else None

    def save_npz(self, path):
        """One .npz (what the drivers' --obdm_out writes): rho_<s>, err_<s>, occ_<s>, natorb_<s>, the raw sums, the counts, the
        degrees (nx, ny) of the basis and the settings."""
        calls, walkers, inv, s, q = self._host()
        rho, err, occ = self.matrix(), self.matrix_err(), self.occupations()
        out = dict(calls=calls, walkers=walkers, invalid=np.array(inv, dtype=np.int64), sum=s, sumsq=q, degrees=np.array(self.degrees(), dtype=np.int64),
                   nup=self.nup, ndown=self.ndown, nshells=self.nshells, sigma=self.sigma, every=self.every, stride=self.stride, seed=self.seed)
        for name in ("up", "down"):
            out["rho_" + name], out["err_" + name] = rho[name], err[name]
            out["occ_" + name], out["natorb_" + name] = occ[name]
        np.savez(path, **out)


# ---- energy components (include/fermiflow_energy.h, csrc/ff_energy_parts.h) -----------------------------------------------------
ENERGY_NAMES = ("T_L", "T_G", "V_trap", "V_uu", "V_ud", "V_dd")
# the derived quantities: linear in the six components, so their means and errors follow from the accumulated moments
ENERGY_DERIVED = {"V_ee": (0, 0, 0, 1, 1, 1), "E": (1, 0, 1, 1, 1, 1), "virial": (2, 0, -2, 1, 1, 1), "dT": (1, -1, 0, 0, 0, 0)}
ENERGY_MAX_STATES = 65536
_EN_K, _EN_HEAD, _EN_FIXED = 6, 4, 52          # FF_ENERGY_PARTS, FF_ENERGY_HEAD, FF_ENERGY_FIXED


class EnergyCounts(tuple):
    """(calls, walkers, invalid) of an EnergyParts: blocks, valid walkers, walkers left out"""
    __slots__ = ()
    calls, walkers, invalid = (property(lambda self, i=i: self[i]) for i in range(3))


class EnergyParts:
    """How the energy of the walkers splits: the kinetic energy by two estimators (T_L = -1/2 laplacian psi / psi, T_G = 1/2 |grad ln psi|^2),
    the trap energy V_trap and the Coulomb repulsion by spin pair (V_uu, V_ud, V_dd), their means, their covariance and, with nstates > 0,
    the energy of every many-body state -- accumulated on the device from what the local-energy pass leaves (x, grad, lap).

        parts = EnergyParts(nup, ndown, Z)                          # BetaVMC: nstates=len(model.Es_original)
        model.energy_parts = parts           # GSVMC / BetaVMC: every sweep feeds it with one launch (two with states), right after the local-energy pass
        ...
        m, e = parts.means(), parts.errors(); m["virial"], e["virial"]; parts.dE_dZ(); parts.per_state()["E"]

    Keys of means() / errors() / block_errors(): the six components and V_ee = V_uu + V_ud + V_dd, E = T_L + V_trap + V_ee, the virial
    2 T_L - 2 V_trap + V_ee (zero on average in an eigenstate of the harmonic trap with Coulomb repulsion) and dT = T_L - T_G (zero on
    average for any normalisable wave function).  errors() are walker-level standard errors -- the walkers of a sweep are independent
    draws -- and those of the derived quantities come from the covariance of the components; block_errors() are block standard errors
    with one block per call (NaN below two calls), for the six components only: the accumulator keeps no cross moments of the blocks, the
    derived entries are NaN there.  Every variance is clamped at zero before its root, as E_std's: no NaN from rounding.

    A walker with a component that is not finite (a failed integration, a coincident pair) is left out and counted.  `centre`: six
    numbers near the expected means, about which the moments are taken (None: zeros); it is part of the object's identity, as Z is.
    accumulate_raw() enqueues on torch's current stream and reads nothing on the host; the host reads the buffer only in counts() /
    means() / ... / state_dict() / all_reduce_() / save_npz().  Every call must bring the same number of walkers.  A result is
    bit-identical from run to run on one device.  all_reduce_() adds the sums of the ranks as doubles, once, when the run is over (the
    counts are exact)."""

    def __init__(self, nup, ndown, Z, dim=2, nstates=0, centre=None, device=None):
        nup, ndown, Z, dim, nstates = int(nup), int(ndown), float(Z), int(dim), int(nstates)
        if nup < 0 or ndown < 0 or nup + ndown < 1:
            raise ValueError("EnergyParts: nup, ndown >= 0 and at least one particle")
        if dim not in (2, 3):
            raise ValueError("EnergyParts: dim must be 2 or 3")
        if not math.isfinite(Z):
            raise ValueError("EnergyParts: Z must be finite")
        if nstates < 0:
            raise ValueError("EnergyParts: nstates must not be negative")
        if nup + ndown > 24 or (nup + ndown) * dim > 60:
            raise NotImplementedError("EnergyParts: n <= 24 and n * dim <= 60")
        if nstates > ENERGY_MAX_STATES:
            raise NotImplementedError(f"EnergyParts: nstates <= {ENERGY_MAX_STATES}")
        if centre is None:
            ctr = (0.0,) * _EN_K
        else:
            ctr = tuple(float(v) for v in np.asarray(centre, dtype=np.float64).reshape(-1))
            if len(ctr) != _EN_K or not all(math.isfinite(v) for v in ctr):
                raise ValueError("EnergyParts: centre must be six finite numbers (T_L, T_G, V_trap, V_uu, V_ud, V_dd)")
        self.nup, self.ndown, self.Z, self.dim, self.nstates, self.centre = nup, ndown, Z, dim, nstates, ctr
        self._words = _EN_FIXED + 8 * nstates          # include/fermiflow_energy.h
        self._B = None
        self._buf = None
        self._ws = None
        self._ctr = None
        self._checked = False
        self.last = None
        if device is not None:
            self._buf = torch.zeros(self._words, dtype=torch.int64, device=torch.device(device))

    # ---- device side -------------------------------------------------------------------------------------------------------
    def accumulate_raw(self, x, grad, lap, walker_state=None):
        """One ff_energy_parts_accumulate on the current stream: x (B, n, dim), grad (B, n, dim), lap (B), fp64 on the device, as native.eloc
        leaves them; walker_state (B) int32, sorted, with nstates > 0.  One call is one block.  `last` keeps the (B, 6) components."""
        from . import native
        x = _lib.dev(x, name="x")
        n = self.nup + self.ndown
        if x.dim() != 3 or x.shape[1] != n or x.shape[2] != self.dim:
            raise ValueError(f"EnergyParts.accumulate_raw: x must be (B, {n}, {self.dim}), got {tuple(x.shape)}")
        if (walker_state is None) != (self.nstates == 0):
            raise ValueError("EnergyParts.accumulate_raw: walker_state goes with nstates > 0, and only with it")
        B = int(x.shape[0])
        if self._B is not None and B != self._B:
            raise ValueError(f"EnergyParts: {B} walkers, the earlier calls had {self._B} (the block errors need equal blocks)")
        if self._buf is None or self._buf.device != x.device:
            self._buf = torch.zeros(self._words, dtype=torch.int64, device=x.device) if self._buf is None else self._buf.to(x.device)
        lib = _lib.lib()
        if not self._checked:
            if lib.ff_energy_parts_buffer_bytes(self.nstates) != 8 * self._words:
                raise RuntimeError("EnergyParts: the library lays the accumulator out differently (include/fermiflow_energy.h)")
            self._checked = True
        need = max(1, lib.ff_energy_parts_workspace_bytes(B, self.nstates) // 8)
        if self._ws is None or self._ws.device != x.device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float64, device=x.device)
        if any(self.centre) and (self._ctr is None or self._ctr.device != x.device):
            self._ctr = torch.tensor(self.centre, dtype=torch.float64, device=x.device)
        last = torch.empty(B, _EN_K, dtype=torch.float64, device=x.device)
        native.energy_parts_accumulate(self.nup, self.ndown, self.Z, x, grad, lap, walker_state, self.nstates, self._ctr, last, self._buf, self._ws)
        self.last = last
        if B > 0:
            self._B = B

    def check_hamiltonian(self, Z, use_ho, extra, nup, ndown, dim, nstates=None):
        """The sweeps' guard: the components are those of the stock Hamiltonian -- harmonic trap and Coulomb repulsion of this object's Z --
        for this object's particle numbers and dimension.  Nothing is decomposed under another one.  nstates: the sweep's state count
        (None: a sweep without states); an object with per-state sums must have exactly that many."""
        if self.nstates > 0 and nstates != self.nstates:
            raise ValueError(f"energy_parts: the EnergyParts object has nstates = {self.nstates}, the sweep has {nstates or 'no'} states")
        if extra or not use_ho:
            raise ValueError("energy_parts: the components are those of HO() and CoulombPairPotential(Z); this model has other potentials")
        if float(Z) != self.Z:
            raise ValueError(f"energy_parts: the model's pair potential has Z = {Z}, the EnergyParts object Z = {self.Z}")
        if (int(nup), int(ndown), int(dim)) != (self.nup, self.ndown, self.dim):
            raise ValueError(f"energy_parts: the model has (nup, ndown, dim) = {(int(nup), int(ndown), int(dim))}, the EnergyParts object "
                             f"{(self.nup, self.ndown, self.dim)}")

    def reset(self):
        if self._buf is not None:
            self._buf.zero_()
        self._B, self.last = None, None

    def _int_words(self):
        idx = list(range(3)) + list(range(_EN_FIXED, _EN_FIXED + self.nstates))
        return torch.tensor(idx, dtype=torch.int64)

    def all_reduce_(self):
        """Sum calls, walkers, invalid and the states' counts (exact below 2^53, it raises otherwise) and every sum (doubles) over the ranks
        of torch.distributed through dist.all_reduce_sum_.  Call it once, when the run is over: one block per rank and call."""
        if self._buf is None:
            self._buf = torch.zeros(self._words, dtype=torch.int64)
        ii = self._int_words().to(self._buf.device)
        isint = torch.zeros(self._words, dtype=torch.bool, device=self._buf.device)
        isint[ii] = True
        isint[3] = True                                  # (the ticket: zero between calls, not reduced)
        fi = torch.nonzero(~isint).reshape(-1)
        t = torch.cat([self._buf[ii].to(torch.float64), self._buf.view(torch.float64)[fi]])
        D.all_reduce_sum_(t)
        if bool((t[:ii.numel()] >= _EXACT).any()):
            raise OverflowError("EnergyParts.all_reduce_: a count reached 2^53, the sum over ranks as doubles would not be exact")
        self._buf[ii] = t[:ii.numel()].to(torch.int64)
        self._buf.view(torch.float64)[fi] = t[ii.numel():]
        return self

    # ---- host side ---------------------------------------------------------------------------------------------------------
    def _host(self):
        a = np.zeros(self._words, dtype=np.int64) if self._buf is None else self._buf.cpu().numpy().astype(np.int64)
        f = a.view(np.float64)
        K, S = _EN_K, self.nstates
        out = dict(calls=int(a[0]), walkers=int(a[1]), invalid=int(a[2]), sum=f[4:10].copy(), sum2=f[10:46].reshape(K, K).copy(), blocksq=f[46:52].copy())
        if S > 0:
            out.update(count=a[_EN_FIXED:_EN_FIXED + S].copy(), ssum=f[_EN_FIXED + S:_EN_FIXED + 7 * S].reshape(S, K).copy(),
                       sumE2=f[_EN_FIXED + 7 * S:_EN_FIXED + 8 * S].copy())
        return out

    def counts(self):
        """(calls, walkers, invalid): blocks, valid walkers, walkers that were left out"""
        h = self._host()
        return EnergyCounts((h["calls"], h["walkers"], h["invalid"]))

    @staticmethod
    def _combos():
        c = {name: np.eye(_EN_K)[k] for k, name in enumerate(ENERGY_NAMES)}
        c.update({name: np.array(a, dtype=np.float64) for name, a in ENERGY_DERIVED.items()})
        return c

    def _moments(self):
        h = self._host()
        N = float(h["walkers"])
        with np.errstate(divide="ignore", invalid="ignore"):
            m = h["sum"] / N
            cov = h["sum2"] / N - np.outer(m, m)
        return h, N, m, cov

    def means(self):
        """{name: mean over the valid walkers}"""
        _, _, m, _ = self._moments()
        c = np.asarray(self.centre) + m
        return {name: float(a @ c) for name, a in self._combos().items()}

    def cov(self):
        """(6, 6): the covariance of the six components over the valid walkers (sum2 / N - mean mean^T about the centre), symmetric"""
        return self._moments()[3]

    def errors(self):
        """{name: walker-level standard error sqrt(max(a^T cov a, 0) / (N - 1))}; NaN below two walkers"""
        _, N, _, cov = self._moments()
        out = {}
        for name, a in self._combos().items():
            with np.errstate(invalid="ignore"):
                out[name] = float(np.sqrt(max(float(a @ cov @ a), 0.0) / (N - 1.0))) if N > 1 else float("nan")
        return out

    def block_errors(self):
        """{name: block standard error, one block per call}: the six components from blocksq, NaN below two calls; NaN for the derived
        entries (no cross moments of the blocks are kept)"""
        h = self._host()
        out = dict.fromkeys(list(ENERGY_NAMES) + list(ENERGY_DERIVED), float("nan"))
        if h["calls"] >= 2:
            m = float(h["calls"])
            var = np.maximum(h["blocksq"] / m - (h["sum"] / m) ** 2, 0.0) * (m / (m - 1.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.sqrt(var / m) / (float(h["walkers"]) / m)
            out.update({name: float(err[k]) for k, name in enumerate(ENERGY_NAMES)})
        return out

    def dE_dZ(self):
        """(value, error) of the Hellmann-Feynman derivative dE/dZ = <V_ee> / Z; NaN at Z = 0"""
        if self.Z == 0.0:
            return float("nan"), float("nan")
        return self.means()["V_ee"] / self.Z, self.errors()["V_ee"] / abs(self.Z)

    def per_state(self):
        """{"count" (S,), the six names (S,): means over the state's valid walkers, "E" (S,), "E_err" (S,): its walker-level standard
        error (NaN below two walkers)}; NaN where a state drew no walker"""
        if self.nstates == 0:
            raise ValueError("EnergyParts.per_state: this object has nstates = 0")
        h = self._host()
        cnt = h["count"].astype(np.float64)
        ctr = np.asarray(self.centre)
        e_idx = [k for k, a in enumerate(ENERGY_DERIVED["E"]) if a]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = h["ssum"] / cnt[:, None]
            out = {"count": h["count"].copy()}
            out.update({name: ctr[k] + d[:, k] for k, name in enumerate(ENERGY_NAMES)})
            dE = d[:, e_idx].sum(1)
            out["E"] = ctr[e_idx].sum() + dE
            var = np.maximum(h["sumE2"] / cnt - dE * dE, 0.0)
            out["E_err"] = np.where(cnt > 1, np.sqrt(var / np.where(cnt > 1, cnt - 1.0, 1.0)), np.nan)
        return out

    def state_dict(self):
        acc = torch.zeros(self._words, dtype=torch.int64) if self._buf is None else self._buf.cpu().clone()
        return {"nup": self.nup, "ndown": self.ndown, "Z": self.Z, "dim": self.dim, "nstates": self.nstates, "centre": self.centre, "acc": acc}

    def load_state_dict(self, st):
        for k in ("nup", "ndown", "Z", "dim", "nstates"):
            if st[k] != getattr(self, k):
                raise ValueError(f"EnergyParts.load_state_dict: {k} = {st[k]!r}, this object has {getattr(self, k)!r}")
        if tuple(float(v) for v in st["centre"]) != self.centre:
            raise ValueError(f"EnergyParts.load_state_dict: centre = {tuple(st['centre'])!r}, this object has {self.centre!r}")
        acc = torch.as_tensor(st["acc"]).to(torch.int64).reshape(-1)
        if acc.numel() != self._words:
            raise ValueError(f"EnergyParts.load_state_dict: {acc.numel()} words, expected {self._words}")
        if self._buf is None:
            self._buf = torch.zeros(self._words, dtype=torch.int64)
        self._buf.copy_(acc.to(self._buf.device))
        calls, total = int(acc[0]), int(acc[1]) + int(acc[2])
        self._B = total // calls if calls > 0 else None

    def save_npz(self, path):
        """One .npz (what the drivers' --energy_out writes): names, mean, err, block_err (one entry per name, the six components and the
        four derived quantities), cov, dE_dZ, the raw moments, the counts, the per-state table with nstates > 0 and the settings."""
        h = self._host()
        names = list(ENERGY_NAMES) + list(ENERGY_DERIVED)
        m, e, b = self.means(), self.errors(), self.block_errors()
        out = dict(names=np.array(names), mean=np.array([m[k] for k in names]), err=np.array([e[k] for k in names]),
                   block_err=np.array([b[k] for k in names]), cov=self.cov(), dE_dZ=np.array(self.dE_dZ()), sum=h["sum"], sum2=h["sum2"],
                   blocksq=h["blocksq"], calls=h["calls"], walkers=h["walkers"], invalid=h["invalid"], centre=np.asarray(self.centre),
                   nup=self.nup, ndown=self.ndown, Z=self.Z, dim=self.dim, nstates=self.nstates)
        if self.nstates > 0:
            ps = self.per_state()
            out.update(state_count=ps["count"], state_E=ps["E"], state_E_err=ps["E_err"], state_mean=np.stack([ps[k] for k in ENERGY_NAMES], axis=1),
                       state_sum=h["ssum"], state_sumE2=h["sumE2"])
        np.savez(path, **out)
