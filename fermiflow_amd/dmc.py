"""Fixed-node diffusion Monte Carlo with the trained flow as guiding function (not in the reference): fermiflow_amd.DMC.

A step is one native local-energy pass at the proposals plus a few small launches (include/fermiflow_dmc.h, csrc/ff_dmc.h):
drift-diffusion proposals, the sign of psi at z(t0), the Green's-function accept step with the weights and the step's record, and a comb
that keeps the population at B walkers of weight 1.  The host reads the device trace once per block.  DESIGN.md 3af has the contract
and what is left out (several ranks, BetaVMC, d = 3, an effective time step, walker ages, weighted observables)."""
import math

import numpy as np
import torch

from . import dist as D
from . import native

RESULT_KEYS = ("E", "E_err", "E_vmc", "acceptance", "crossing", "invalid", "esf", "distinct", "blocks", "tau", "steps_per_block", "batch")


class DMC:
    """DMC(model, tau, steps_per_block, drift_limit, ecut, seed): `model` a GSVMC in two dimensions on one rank.

    start(batch) draws the population with model.sample and sets E_T = E_ref = E_VMC of it, c = ecut sqrt(n / tau) (the local energies
    enter the weights clipped to E_ref +- c).  run(nblocks, equilibrate) advances blocks of steps_per_block steps; after every block
    E_ref = E_T = (sum sum w e) / (sum sum w) over the measured steps so far (over the block itself while equilibrating).  result()
    gives E (the ratio of the summed records of the measured blocks), E_err (the standard error of the block ratios), E_vmc, the
    acceptance, the node-crossing rate, the invalid count, the mean effective sample fraction (sum w)^2 / (B sum w^2), the mean number
    of distinct sources per comb and the block energies.  observables / density_maps: an Observables / DensityMaps that receives the
    walkers after the comb every `observe_every` measured steps (mixed estimators; the weights are 1 there).  comb = False leaves the walkers
    where the accept step put them and lets the weights run (a plain drift-diffusion Metropolis chain in |psi|^2)."""

    def __init__(self, model, tau=0.01, steps_per_block=50, drift_limit=1.0, ecut=0.2, seed=0, observe_every=1):
        from .VMC import GSVMC, BetaVMC
        if isinstance(model, BetaVMC):
            raise ValueError("DMC: BetaVMC (an ensemble of states) has no single guiding function; pass a GSVMC")
        if not isinstance(model, GSVMC):
            raise ValueError(f"DMC: model must be a GSVMC, not {type(model).__name__}")
        if model.__dict__.get("_sweep_dim", 2) != 2:
            raise ValueError("DMC: two dimensions only (the sign of the determinants is computed for d = 2)")
        if D.world()[1] > 1:
            raise ValueError("DMC: one rank only (the comb resamples one population)")
        tau, drift_limit, ecut = float(tau), float(drift_limit), float(ecut)
        if not (tau > 0.0 and math.isfinite(tau)):
            raise ValueError("DMC: tau must be positive and finite")
        if not (drift_limit >= 0.0 and math.isfinite(drift_limit)):
            raise ValueError("DMC: drift_limit must be finite and >= 0")
        if not (ecut > 0.0 and math.isfinite(ecut)):
            raise ValueError("DMC: ecut must be positive and finite")
        if int(steps_per_block) < 1 or int(observe_every) < 1:
            raise ValueError("DMC: steps_per_block and observe_every must be at least 1")
        self.model, self.tau, self.drift_limit, self.ecut = model, tau, drift_limit, ecut
        self.steps_per_block, self.observe_every, self.seed = int(steps_per_block), int(observe_every), int(seed) & (2 ** 64 - 1)
        self.nup, self.ndown = model.nup, model.ndown
        self.observables = None
        self.density_maps = None
        self.comb = True
        self.trace_blocks = 64      # how many blocks' records `trace` keeps (the oldest go first)
        self._state, self._tabs = None, None

    # ---- the population --------------------------------------------------------------------------------------------------
    def _guide(self, x):
        """logp, grad, eloc and the sign of psi at x: one local-energy pass and the sign kernel at its z(t0)"""
        r = self.model.local_energy(x)
        if self._tabs is None or self._tabs[0] != x.device:
            self._tabs = (x.device,) + tuple(self.model._tables(x.device))
        sign = native.slater_sign(self._tabs[1], self._tabs[2], self.nup, self.ndown, r["z"])
        return dict(x=x, logp=r["logp"], grad=r["grad"], eloc=r["eloc"], sign=sign)

    def start(self, batch, x=None):
        """Draw `batch` walkers with model.sample (or take x (batch, n, 2)) and set the energies from them.  Returns E_VMC."""
        batch = int(batch)
        if batch < 1:
            raise ValueError("DMC.start: batch must be at least 1")
        with torch.no_grad():
            if x is None:
                _, x = self.model.sample((batch,))
            x = x.detach().contiguous().clone()
            if tuple(x.shape) != (batch, self.nup + self.ndown, 2):
                raise ValueError(f"DMC.start: x must be ({batch}, {self.nup + self.ndown}, 2), got {tuple(x.shape)}")
            st = self._guide(x)
            e = st["eloc"]
            ok = torch.isfinite(e)
            e_vmc = float(torch.where(ok, e, torch.zeros_like(e)).sum() / ok.sum())
        dev = x.device
        self._state = {k: v.contiguous() for k, v in st.items()}
        self._spare = {k: torch.empty_like(v) for k, v in self._state.items()}
        self._w = torch.ones(batch, dtype=torch.float64, device=dev)
        self._src = torch.zeros(batch, dtype=torch.int32, device=dev)
        self._ws_accept, self._ws_comb = native.dmc_workspaces(batch, dev)
        self.batch, self.E_vmc = batch, e_vmc
        self.E_T = self.E_ref = e_vmc
        self.cut = self.ecut * math.sqrt((self.nup + self.ndown) / self.tau)
        self._ctrl = torch.tensor([e_vmc, e_vmc, self.cut], dtype=torch.float64, device=dev)
        self._step_no, self._measured = 0, 0
        self._blocks, self._tot = [], np.zeros(2)
        self._diag = dict(acc=0, crossed=0, invalid=0, esf=0.0, distinct=0.0, steps=0, combs=0)
        self.trace = []      # per block, the last `trace_blocks` of them: (six sums (steps, 6), three counts (steps, 3), the comb's info words (steps, 4))
        return e_vmc

    @property
    def walkers(self):
        return self._state["x"]

    @property
    def weights(self):
        return self._w

    def _step(self, rec, slot, info, measure):
        st = self._state
        x1, _ = native.dmc_propose(self.nup, self.ndown, st["x"], st["grad"], self.tau, self.drift_limit, seed=self.seed, step=self._step_no)
        prop = self._guide(x1)
        native.dmc_accept(self.nup, self.ndown, dict(st, w=self._w), prop, self.tau, self.drift_limit, self._ctrl, rec, slot, self._ws_accept,
                          seed=self.seed, step=self._step_no)
        if self.comb:
            native.dmc_comb(self.nup, self.ndown, dict(st, w=self._w), self._spare, self._src, info, self._ws_comb, seed=self.seed,
                            step=self._step_no)
            self._state, self._spare = self._spare, self._state
        self._step_no += 1
        if not measure:
            return
        self._measured += 1
        if self._measured % self.observe_every == 0:
            if self.observables is not None:
                self.observables.accumulate(self._state["x"])
            if self.density_maps is not None:
                self.density_maps.accumulate(self._state["x"])

    def run(self, nblocks, equilibrate=0):
        """`equilibrate` blocks that are not measured, then `nblocks` that are.  One host read per block.  Returns result()."""
        if self._state is None:
            raise RuntimeError("DMC.run: call start(batch) first")
        spb, dev = self.steps_per_block, self._w.device
        for blk in range(int(equilibrate) + int(nblocks)):
            rec = torch.zeros(spb * native.DMC_REC, dtype=torch.int64, device=dev)
            info = torch.zeros(spb, 4, dtype=torch.int32, device=dev)
            with torch.no_grad():
                for s in range(spb):
                    self._step(rec, s, info[s], blk >= int(equilibrate))
            words = rec.cpu().numpy().reshape(spb, native.DMC_REC)       # the block's one host read
            info_h = info.cpu().numpy()
            f, cnt = words[:, :6].copy().view(np.float64), words[:, 6:]
            self.trace.append((f, cnt.copy(), info_h))
            del self.trace[:max(0, len(self.trace) - int(self.trace_blocks))]
            if info_h[:, 2].any() or not np.isfinite(f).all() or not (f[:, 0] > 0).all():
                raise FloatingPointError("DMC: the population's total weight became zero or not finite (step "
                                         f"{self._step_no - spb + int(np.argmax(info_h[:, 2] != 0))} of this run's block)")
            bsum = np.array([f[:, 0].sum(), f[:, 1].sum()])
            if blk >= int(equilibrate):
                self._blocks.append(bsum[1] / bsum[0])
                self._tot += bsum
                d = self._diag
                d["acc"] += int(cnt[:, 0].sum()); d["crossed"] += int(cnt[:, 1].sum()); d["invalid"] += int(cnt[:, 2].sum())
                d["esf"] += float((f[:, 0] ** 2 / (self.batch * f[:, 3])).sum()); d["steps"] += spb
                if self.comb:
                    d["distinct"] += float(info_h[:, 0].sum()); d["combs"] += spb
                self.E_T = self.E_ref = float(self._tot[1] / self._tot[0])
            else:
                self.E_T = self.E_ref = float(bsum[1] / bsum[0])
            self._ctrl.copy_(torch.tensor([self.E_T, self.E_ref, self.cut], dtype=torch.float64))
        return self.result()

    def result(self):
        b, d = np.array(self._blocks), self._diag
        ns = max(d["steps"], 1)
        return dict(E=float(self._tot[1] / self._tot[0]) if len(b) else float("nan"),
                    E_err=float(b.std(ddof=1) / math.sqrt(len(b))) if len(b) > 1 else float("nan"), E_vmc=self.E_vmc,
                    acceptance=d["acc"] / (ns * self.batch), crossing=d["crossed"] / (ns * self.batch), invalid=d["invalid"],
                    esf=d["esf"] / ns, distinct=d["distinct"] / max(d["combs"], 1), blocks=b, tau=self.tau,
                    steps_per_block=self.steps_per_block, batch=self.batch)

    def save_npz(self, path):
        """result() in one .npz (what the driver's --dmc_out writes): the keys of RESULT_KEYS"""
        np.savez(path, **{k: np.asarray(v) for k, v in self.result().items()})
