"""The --optimizer sr training loop under the HOST SIMULATOR (no GPU): 3 + 3 particles, Z = 2, init_zeros(), 20 iterations at the
defaults of fermiflow_amd.SR, every stage through the simulator's build of the kernels (Metropolis, flow, local energy, tabulated
adjoint for the force, ff_cnf_adjoint_scores, ff_sr_moments, ff_sr_finish) and numpy's solve in place of the device Cholesky.
Prints E per iteration and the margin (E_first - E_last) / sqrt(se_first^2 + se_last^2) that tests/test_gpu_sr.py asserts on the
device at B = 4096.   python tools/probes/sr_sim_train.py [B] [iterations] [lr] [shift]

    python tools/probes/sr_sim_train.py beta [B] [iterations] [Z] [beta]
is the finite-temperature loop of tests/test_gpu_sr_beta.py::test_training_smoke (3 + 0 particles, deltaE = 2, the logits torch.randn
after torch.manual_seed(42) as that test draws them, BetaSR's defaults): states drawn with numpy, Metropolis by state, flow, local
energy, ff_beta_finish, the tabulated adjoint with the per-state baseline, ff_cnf_adjoint_scores, ff_sr_state_moments,
ff_sr_state_finish, numpy's solves for both blocks.  Prints F per iteration and the margin in combined standard errors of F."""
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


def main_beta(argv):
    import torch
    import fermiflow_amd as ff
    from fermiflow_amd.orbitals import orbital_indices
    from tests import sr_beta_ref as RB
    B = int(argv[0]) if len(argv) > 0 else 48
    iters = int(argv[1]) if len(argv) > 1 else 20
    Z = float(argv[2]) if len(argv) > 2 else 0.5
    beta = float(argv[3]) if len(argv) > 3 else 2.0
    lr, shift, H, tol = 0.05, 1e-3, 50, dict(rtol=1e-6, atol=1e-8)
    torch.manual_seed(42)
    eta, mu = ff.MLP(1, H), ff.MLP(1, H)      # (the test constructs them first: they draw from the same generator)
    states, _ = ff.HO2D().fermion_states(3, 0, 2.0)
    logits = torch.randn(len(states), dtype=torch.float64).numpy().copy()
    tab = np.ascontiguousarray([orbital_indices(s[0]) for s in states], dtype=np.int32)
    ns = len(states)
    rng = np.random.default_rng(7)
    theta = np.zeros(6 * H)
    hist, prevE = [], 0.0
    for it in range(iters):
        w = [theta[k * H:(k + 1) * H].copy() for k in range(6)]
        net, net_direct = S.Net(w[:3], w[3:], table=True), S.Net(w[:3], w[3:])
        p = np.exp(logits - logits.max()); p /= p.sum()
        ws = np.sort(rng.choice(ns, size=B, p=p)).astype(np.int32)
        z = np.empty((B, 3, 2)); lp = np.empty(B); cnt = np.empty(B, dtype=np.int32)
        S._ck(S.lib().ff_mcmc_sample(None, B, 3, 0, S._p(tab), None, S._p(ws), 100, 0.1, 1000 + it, 0, S._p(z), S._p(lp), S._p(cnt)))
        x, _ = S.cnf_generate(z, net, **tol)
        r = S.eloc(x, 3, 0, net, Z, tab_up=tab, wstate=ws, **tol)
        e = r["eloc"]
        est, gphi, mean_e, lpa = S.beta_estimator(e, r["logp"], ws, logits, beta, prevE)
        prevE = est[0]
        F, se = est[2], np.sqrt(est[3] / (B - 1)) / np.sqrt(B)
        _, g, _ = S.cnf_adjoint_energy(r["z"], r["glogp0"], e, mean_e, 1.0 / B, net, mean_index=ws, **tol)
        _, O, st = R.sim_scores(S, r["z"], r["glogp0"], net_direct, tol)
        assert st[3] == 0
        _, sums = RB.sim_state_moments(S, O, e, ws, mean_e)
        fisher, _, gsr = RB.sim_state_finish(S, sums, 6 * H, ns)
        theta -= lr * np.linalg.solve(fisher + shift * np.eye(6 * H), g)
        mu_s = np.exp(lpa)
        logits -= lr * np.linalg.solve(np.diag(mu_s) - np.outer(mu_s, mu_s) + shift * np.eye(ns), gphi)
        hist.append((F, se))
        print(f"iter {it + 1:02d} F {F:.4f} se {se:.4f} E {est[0]:.4f} |g - g_scores| {np.abs(g - gsr).max():.2e}", flush=True)
    (f0, s0), (f1, s1) = hist[0], hist[-1]
    m = (f0 - f1) / np.hypot(s0, s1)
    print(f"beta {beta} Z {Z} B {B}: drop {f0 - f1:.4f} = {m:.2f} combined standard errors; scaled to B = 4096: {m * np.sqrt(4096 / B):.1f}")


if __name__ == "__main__":
    main_beta(sys.argv[2:]) if len(sys.argv) > 1 and sys.argv[1] == "beta" else main()
