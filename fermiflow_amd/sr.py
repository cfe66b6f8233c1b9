"""Stochastic reconfiguration (natural gradient) for GSVMC (SR) and BetaVMC (BetaSR, below).

    model.sr = optimizer = SR(model.parameters(), lr=0.05, shift=1e-3)
    gradE = model(batch); optimizer.zero_grad(); gradE.backward(); optimizer.step()

With `model.sr` set, every sweep also computes the per-walker log-derivatives O_b = d log p(x_b) / d theta
(ff_cnf_adjoint_scores), their moments on the matrix cores (ff_sr_moments, all-reduced over the ranks) and leaves
`fisher` = <O O^T> - <O><O>^T, `obar` = <O>, `grad` = <O (E_loc - E)> and `scores` on this object as device tensors.
step() solves (fisher + shift I) delta = g on the device and updates theta <- theta - lr delta, where g is the parameters'
.grad -- the gradient the sweep's own (tabulated) adjoint delivers, exactly what Adam would get.  Nothing waits for the host: the
Cholesky factorisation's status flag is never read back (a matrix that is not positive definite gives NaN parameters, as a NaN
gradient does with Adam).

Convention.  `fisher` is the Fisher matrix of p = |psi|^2.  In terms of the log-derivatives of psi (O^psi = O / 2, the usual
statement of stochastic reconfiguration) the matrix is fisher / 4 and the force g / 2, so the solution there is twice the one here:
the same direction with the step doubled at equal lr.  lr = 0.05 and shift = 1e-3 here are lr = 0.025 and shift = 2.5e-4 there.
"""
import torch


class SR:
    kind = "sr"

    def __init__(self, params, lr=0.05, shift=1e-3, rescale=True):
        self.params = [p for p in params]
        self.lr, self.shift = float(lr), float(shift)
        # rescale: the system is solved in the variables D delta with D = sqrt(diag(fisher) + shift) (a symmetric diagonal
        # equilibration in front of the factorisation: the same solution, a better conditioned matrix)
        self.rescale = bool(rescale)
        self.fisher = self.obar = self.grad = self.scores = None      # set by the sweep (GSVMC._sweep)
        self.delta = None                                             # the last step's solution

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def flat_grad(self):
        return torch.cat([p.grad.reshape(-1) for p in self.params])

    def solve(self, fisher, g, shift=None):
        """delta of (fisher + shift I) delta = g by a Cholesky factorisation on the tensors' device (shift: default self.shift)"""
        A = fisher + (self.shift if shift is None else shift) * torch.eye(fisher.shape[0], dtype=fisher.dtype, device=fisher.device)
        if self.rescale:
            dinv = A.diagonal().rsqrt()
            A = A * dinv[:, None] * dinv[None, :]
            g = g * dinv
        Lc, _ = torch.linalg.cholesky_ex(A)
        x = torch.cholesky_solve(g[:, None], Lc)[:, 0]
        return x * dinv if self.rescale else x

    @torch.no_grad()
    def step(self):
        if self.fisher is None:
            raise RuntimeError("SR.step: no Fisher matrix -- set model.sr to this optimizer before the sweep")
        self.delta = self.solve(self.fisher, self.flat_grad().to(self.fisher.dtype))
        off = 0
        for p in self.params:
            n = p.numel()
            p.sub_(self.lr * self.delta[off:off + n].view_as(p).to(p.dtype))
            off += n

    # a checkpoint stores the kind and the two numbers: there is no other state
    def state_dict(self):
        return {"kind": self.kind, "lr": self.lr, "shift": self.shift, "rescale": self.rescale}

    def load_state_dict(self, sd):      # (checkpoint.load has checked the kind)
        self.lr, self.shift, self.rescale = float(sd["lr"]), float(sd["shift"]), bool(sd["rescale"])


class BetaSR(SR):
    """Stochastic reconfiguration for BetaVMC: the joint p(n, x) = mu_n(phi) p_n(x; theta), mu = softmax(logits).

        model.sr = optimizer = BetaSR(model, lr=0.05, shift=1e-3)
        gradF_phi, gradF_theta = model(batch); optimizer.zero_grad(); gradF_phi.backward(); gradF_theta.backward(); optimizer.step()

    The scores of the joint are s_phi = e_n - mu and O = d log p_n(x) / d theta, and E_{x|n}[O] = 0 for every state (each p_n is
    normalised): its Fisher matrix is block diagonal.  The sweep (BetaVMC._sweep) leaves on this object, as device tensors,
      fisher      (P, P)   (1/B) [sum_b O_b O_b^T - sum_n o_n o_n^T / c_n]: O centred PER STATE (ff_sr_state_moments / _finish), which
                           makes the in-sample cross block vanish as the population's does,
      obar_state  (Ns, P)  the states' mean scores, grad (P) = (1/B) sum_b O_b (e_b - mean_e[state_b]) (a cross-check of .grad), scores (B, P),
      fisher_phi  (Ns, Ns) diag(mu) - mu mu^T, exact (no sampling noise), singular along the gauge direction 1: the shift regularises it.
    step() solves (fisher + shift I) dtheta = flat theta-.grad and (fisher_phi + shift_phi I) dphi = logits-.grad (SR.solve) and
    updates theta <- theta - lr dtheta, logits <- logits - lr_phi dphi.  Nothing waits for the host.

    lr_phi is a number of its own (default: lr).  Noise-free and without a shift, dphi_k = Fbar_k - F, where Fbar_k is the state's
    mean local free energy.  lr_phi = beta is then the exact jump to the Boltzmann-like fixed point log mu_k = -beta Ebar_k + const;
    anything well below beta is a damped version of that jump."""

    def __init__(self, model, lr=0.05, shift=1e-3, lr_phi=None, shift_phi=None, rescale=True):
        # the flow's parameters in the order of the scores' columns
        super().__init__(model.cnf.parameters(), lr=lr, shift=shift, rescale=rescale)
        self.logits = model.log_state_weights
        self.lr_phi = float(lr if lr_phi is None else lr_phi)
        self.shift_phi = float(shift if shift_phi is None else shift_phi)
        self.obar_state = self.fisher_phi = None      # (with fisher, grad, scores: set by the sweep)
        self.delta_phi = None

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none)
        if self.logits.grad is not None:
            if set_to_none:
                self.logits.grad = None
            else:
                self.logits.grad.zero_()

    @torch.no_grad()
    def step(self):
        if self.fisher is None or self.fisher_phi is None:
            raise RuntimeError("BetaSR.step: no Fisher matrix -- set model.sr to this optimizer before the sweep")
        super().step()
        g = self.logits.grad.to(device=self.fisher_phi.device, dtype=self.fisher_phi.dtype)
        self.delta_phi = self.solve(self.fisher_phi, g, shift=self.shift_phi)
        self.logits.sub_(self.lr_phi * self.delta_phi.to(device=self.logits.device, dtype=self.logits.dtype))

    def state_dict(self):
        return {"kind": self.kind, "lr": self.lr, "shift": self.shift, "lr_phi": self.lr_phi, "shift_phi": self.shift_phi, "rescale": self.rescale}

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.lr_phi, self.shift_phi = float(sd["lr_phi"]), float(sd["shift_phi"])
