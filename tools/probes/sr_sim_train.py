"""The --optimizer sr training loop under the HOST SIMULATOR (no GPU): 3 + 3 particles, Z = 2, init_zeros(), 20 iterations at the
defaults of fermiflow_amd.SR, every stage through the simulator's build of the kernels (Metropolis, flow, local energy, tabulated
adjoint for the force, ff_cnf_adjoint_scores, ff_sr_moments, ff_sr_finish) and numpy's solve in place of the device Cholesky.
Prints E per iteration and the margin (E_first - E_last) / sqrt(se_first^2 + se_last^2) that tests/test_gpu_sr.py asserts on the
device at B = 4096.   python tools/probes/sr_sim_train.py [B] [iterations] [lr] [shift]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import sr_ref as R                # noqa: E402
from tests.hostsim import simlib as S        # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lr = float(sys.argv[3]) if len(sys.argv) > 3 else 0.05
    shift = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-3
    H, tol = 50, dict(rtol=1e-6, atol=1e-8)
    theta = np.zeros(6 * H)
    hist = []
    for it in range(iters):
        w = [theta[k * H:(k + 1) * H].copy() for k in range(6)]
        net = S.Net(w[:3], w[3:], table=True)
        net_direct = S.Net(w[:3], w[3:])
        z, _, _ = S.mcmc(B, 3, 3, 100, 1000 + it)
        x, _ = S.cnf_generate(z, net, **tol)
        r = S.eloc(x, 3, 3, net, 2.0, **tol)
        e = r["eloc"]
        E, se = e.mean(), e.std(ddof=1) / np.sqrt(B)
        _, g, _ = S.cnf_adjoint_energy(r["z"], r["glogp0"], e, E, 1.0 / B, net, **tol)
        _, O, st = R.sim_scores(S, r["z"], r["glogp0"], net_direct, tol)
        assert st[3] == 0
        _, sums = R.sim_moments(S, O, e, E)
        F, _, gsr = R.sim_finish(S, sums, 6 * H)
        delta = np.linalg.solve(F + shift * np.eye(6 * H), g)
        theta -= lr * delta
        hist.append((E, se))
        print(f"iter {it + 1:02d} E {E:.4f} se {se:.4f} |g - g_scores| {np.abs(g - gsr).max():.2e}", flush=True)
    (e0, s0), (e1, s1) = hist[0], hist[-1]
    print(f"B {B} lr {lr} shift {shift}: drop {e0 - e1:.4f} = {(e0 - e1) / np.hypot(s0, s1):.2f} combined standard errors")


if __name__ == "__main__":
    main()
