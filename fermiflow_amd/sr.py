"""Stochastic reconfiguration (natural gradient) for GSVMC.

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

    def solve(self, fisher, g):
        """delta of (fisher + shift I) delta = g by a Cholesky factorisation on the tensors' device"""
        A = fisher + self.shift * torch.eye(fisher.shape[0], dtype=fisher.dtype, device=fisher.device)
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
