"""What the robust estimator (GSVMC.clip_eloc) costs on one GPU, at the benchmark's workload (3 + 3 particles, 65 536
walkers, bench.py's step and seed):
  (1) iteration time with clip_eloc = 5 against unset, in alternating blocks in ONE process (the method of DESIGN.md 3t: the same
      process, the same clocks, the same neighbours on the machine), wall clock around a device synchronise;
  (2) stand-alone, device events around 200 back-to-back calls: ff_energy_estimate, ff_energy_robust, ff_energy_robust + _apply.
Prints one JSON line.   python tools/probes/robust_cost.py [--blocks 6] [--steps 100]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as G      # noqa: E402
from fermiflow_amd import native      # noqa: E402
from fermiflow_amd.utils import make_adam      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--clip", type=float, default=5.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = G._model(dev, 3, 3, 2.0)
    opt = make_adam(model.parameters(), lr=2e-5)
    torch.manual_seed(1234)
    B = args.walkers

    def step():
        g = model(B)
        opt.zero_grad()
        g.backward()
        opt.step()

    def block(k):
        model.clip_eloc = k
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for k in (None, args.clip):      # warm up both paths
        model.clip_eloc = k
        for _ in range(20):
            step()
    off, on = [], []
    for _ in range(args.blocks):
        off.append(block(None))
        on.append(block(args.clip))
    stats = {"n_valid": model.n_valid, "n_clipped": model.n_clipped, "E": model.E, "E_std": model.E_std, "E_median": model.E_median,
             "E_width": model.E_width}

    e, lp = model.Eloc.clone(), torch.randn(B, dtype=torch.float64, device=dev) - 20.0
    shift = torch.full((1,), 30.0, dtype=torch.float64, device=dev)

    def timed(fn, reps=200):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3      # us per call

    def both():
        st = native.energy_robust(e, lp, args.clip, shift)
        native.energy_robust_apply(e, lp, st, B, True)

    alone = {"energy_estimate_us": timed(lambda: native.energy_estimate(e, lp, shift, B)),
             "energy_robust_us": timed(lambda: native.energy_robust(e, lp, args.clip, shift)),
             "robust_plus_apply_us": timed(both)}
    print(json.dumps({"walkers": B, "steps_per_block": args.steps, "iteration_ms_unset": off, "iteration_ms_clip": on,
                      "mean_unset": statistics.mean(off), "mean_clip": statistics.mean(on),
                      "spread_unset": max(off) - min(off), "spread_clip": max(on) - min(on), "last_sweep": stats, "standalone": alone}))


if __name__ == "__main__":
    main()
