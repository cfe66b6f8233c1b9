"""Rates of the stochastic-reconfiguration pieces on an MI355X at config 2 (65 536 walkers x 6 particles, benchmark weights):
  (a) ff_cnf_adjoint_scores against the direct ff_cnf_adjoint (radial_table = NULL) -- whose kernels are the parent commit's,
      resource figure for resource figure; FERMIFLOW_LIB=<a build of the parent> runs the direct leg alone on that build,
  (b) ff_sr_moments in TFLOP/s (2 B P^2 flop) against the 78.6 TFLOP/s fp64 matrix peak, and the bytes its design moves (O once per panel pair + the partial tiles twice; no counter is read) against 8 B P,
  (c) one SR iteration against one Adam iteration.
Device events, a warm-up, medians of alternating runs.  Prints one JSON line; python tools/probes/sr_rate.py [B] [reps]

    python tools/probes/sr_rate.py beta [B] [reps]
is the leg at config 3 (BetaFermionHO2D --beta 10 --nup 3 --boltzmann: 65 536 walkers, P = 300, 21 states):
  (d) ff_sr_state_moments against ff_sr_moments -- the parent's kernel, unchanged -- on the same scores (extra work: the flush at
      every change of state and (nchunks + nstates) P partials), and ff_sr_state_finish against ff_sr_finish,
  (e) one BetaSR iteration against one Adam iteration."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import __graft_entry__ as Gm      # noqa: E402
import fermiflow_amd as ff        # noqa: E402
from fermiflow_amd import native, _lib as L   # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = torch.device("cuda:0")
    model = Gm._model(dev)
    torch.manual_seed(0)
    model(B).backward()
    v = model.cnf.v_wrapper.v
    net = v.net(radial="exact")
    tu, td = model._tables(dev)
    r = native.eloc(tu, td, 3, 3, net, model.x, 0.0, 1.0, 1e-6, 1e-8, 2.0, True)
    w = (r["eloc"] - r["eloc"].mean()) / B
    out = {"B": B, "reps": reps}
    have_scores = hasattr(L.lib(), "ff_cnf_adjoint_scores")
    direct = lambda: native.cnf_adjoint(net, r["z"], w[:, None, None] * r["glogp0"], -w, 0.0, 1.0, 1e-6, 1e-8, need_gx=False)
    scores = (lambda: native.cnf_adjoint_scores(net, r["z"], r["glogp0"], 0.0, 1.0, 1e-6, 1e-8)) if have_scores else None
    direct(); scores and scores()
    td_, ts_ = [], []
    for _ in range(reps):      # alternating
        td_.append(timed(direct))
        if scores:
            ts_.append(timed(scores))
    out["direct_adjoint_ms"] = statistics.median(td_)
    if scores:
        out["scores_ms"] = statistics.median(ts_)
        out["scores_over_direct"] = out["scores_ms"] / out["direct_adjoint_ms"]
        O = scores()
        P = O.shape[1]
        em = r["eloc"].mean().reshape(1)
        mom = lambda: native.sr_moments(O, r["eloc"], em)
        mom()
        tm = statistics.median(timed(mom) for _ in range(reps))
        out.update(moments_ms=tm, moments_tflops=2.0 * B * P * P / tm * 1e-9, moments_peak_fraction=2.0 * B * P * P / tm * 1e-9 / 78.6,
                   moments_design_bytes_over_scores_bytes=(8.0 * B * 128 * (((P + 63) // 64) * ((P + 63) // 64 + 1) // 2)
                                                           + 2.0 * L.lib().ff_sr_moments_workspace_bytes(B, P)) / (8.0 * B * P))
        from fermiflow_amd.utils import make_adam
        adam, sr = make_adam(model.parameters(), lr=1e-2), ff.SR(model.parameters())

        def iteration(opt):
            model.sr = opt if opt is sr else None
            g = model(B); opt.zero_grad(); g.backward(); opt.step()
        for opt in (adam, sr):
            iteration(opt)
        ta, tsr = [], []
        for _ in range(reps):
            ta.append(timed(lambda: iteration(adam))); tsr.append(timed(lambda: iteration(sr)))
        out.update(adam_iteration_ms=statistics.median(ta), sr_iteration_ms=statistics.median(tsr))
    print(json.dumps(out))


def main_beta(argv):
    B = int(argv[0]) if len(argv) > 0 else 65536
    reps = int(argv[1]) if len(argv) > 1 else 7
    dev = torch.device("cuda:0")
    eta, mu = ff.MLP(1, 50), ff.MLP(1, 50)
    eta.init_gaussian(1); mu.init_gaussian(2)
    cnf = ff.CNF(ff.Backflow(eta, mu=mu), (0.0, 1.0))
    model = ff.BetaVMC(10.0, 3, 0, 2.0, True, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    model.to(device=dev)
    from fermiflow_amd.utils import make_adam
    adam, sr = make_adam(model.parameters(), lr=1e-2), ff.BetaSR(model)
    torch.manual_seed(0)

    def iteration(opt):
        model.sr = opt if opt is sr else None
        gp, gt = model(B); opt.zero_grad(); gp.backward(); gt.backward(); opt.step()
    for opt in (adam, sr, adam, sr):
        iteration(opt)
    O, e, ws, Ns = sr.scores, model.Eloc, model._ws, model.Nstates
    P = O.shape[1]
    me = torch.full((Ns,), e.mean().item(), dtype=torch.float64, device=dev)
    plain = lambda: native.sr_moments(O, e, me)
    state = lambda: native.sr_state_moments(O, e, ws, me, Ns)
    sp, ss = plain(), state()
    fplain = lambda: native.sr_finish(sp, P)
    fstate = lambda: native.sr_state_finish(ss, P, Ns)
    fplain(); fstate()
    t = {k: [] for k in ("plain", "state", "fplain", "fstate", "adam", "sr")}
    for _ in range(reps):      # alternating
        t["plain"].append(timed(plain)); t["state"].append(timed(state))
        t["fplain"].append(timed(fplain)); t["fstate"].append(timed(fstate))
    for _ in range(reps):
        t["adam"].append(timed(lambda: iteration(adam))); t["sr"].append(timed(lambda: iteration(sr)))
    m = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps({"B": B, "P": P, "nstates": Ns, "reps": reps, "moments_ms": m["plain"], "state_moments_ms": m["state"],
                      "state_over_plain": m["state"] / m["plain"], "finish_ms": m["fplain"], "state_finish_ms": m["fstate"],
                      "adam_iteration_ms": m["adam"], "betasr_iteration_ms": m["sr"],
                      "spread_state_moments_ms": [min(t["state"]), max(t["state"])], "spread_moments_ms": [min(t["plain"]), max(t["plain"])]}))


if __name__ == "__main__":
    main_beta(sys.argv[2:]) if len(sys.argv) > 1 and sys.argv[1] == "beta" else main()
