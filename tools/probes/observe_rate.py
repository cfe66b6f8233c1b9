#!/usr/bin/env python3
"""What the observables cost, in one process on the MI355X:

  (a) ff_observe_accumulate against stand-alone ff_potential -- the yardstick: it reads the same bytes and forms the same pair
      distances -- on the same walkers, 65 536 x 6 and 1 048 576 x 6 particles in 2-D: median time per launch of back-to-back
      launches between two events (windows of some 50 ms and more: 2000 launches at 65 536 walkers, 400 at 1 M; WINDOWS windows,
      the two kernels alternating);
  (b) the benchmark's default training iteration (3 + 3 particles, 65 536 walkers) with model.observables set and with None,
      alternating blocks of iterations in the same process, median over the blocks.

    python tools/probes/observe_rate.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch      # noqa: E402

import __graft_entry__ as G      # noqa: E402
import fermiflow_amd as ff      # noqa: E402
from fermiflow_amd import native      # noqa: E402
from fermiflow_amd.utils import make_adam      # noqa: E402

WINDOWS = 15


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(dev, B, rmax, nbins):
    x = torch.randn(B, 6, 2, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    obs = ff.Observables(3, 3, rmax=rmax, nbins=nbins)
    fo, fp = (lambda: obs.accumulate(x)), (lambda: native.potential(x, 2.0, True))
    reps = 2000 if B <= (1 << 17) else 400
    for f in (fo, fp):
        window_us(f, 50)
    to, tp = [], []
    for _ in range(WINDOWS):
        to.append(window_us(fo, reps))
        tp.append(window_us(fp, reps))
    mo, mp = statistics.median(to), statistics.median(tp)
    return {"walkers": B, "nbins": nbins, "observe_us": round(mo, 2), "potential_us": round(mp, 2), "ratio": round(mo / mp, 2),
            "observe_us_min_max": [round(min(to), 2), round(max(to), 2)], "potential_us_min_max": [round(min(tp), 2), round(max(tp), 2)],
            "GB_per_s_observe": round(B * 96 / mo / 1e3, 1)}


def iteration(dev, B=65536, block=20, blocks=8):
    model = G._model(dev)
    opt = make_adam(model.parameters(), lr=2e-5)
    obs = ff.Observables(3, 3)
    torch.manual_seed(1234)

    def step():
        g = model(B)
        opt.zero_grad()
        g.backward()
        opt.step()

    def timed(o):
        model.observables = o
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(block):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / block

    for _ in range(10):
        step()
    t_none, t_obs = [], []
    for _ in range(blocks):
        t_none.append(timed(None))
        t_obs.append(timed(obs))
    mn, mo = statistics.median(t_none), statistics.median(t_obs)
    return {"walkers": B, "iteration_ms_none": round(mn, 4), "iteration_ms_observables": round(mo, 4), "difference_us": round((mo - mn) * 1e3, 1),
            "none_min_max": [round(min(t_none), 4), round(max(t_none), 4)], "observables_min_max": [round(min(t_obs), 4), round(max(t_obs), 4)],
            "calls": obs.counts()["calls"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-iteration", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("observe_rate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    for B in (65536, 1 << 20):
        for nbins in (240, 16):
            res["kernels"].append(kernels(dev, B, 6.0, nbins))
            print(json.dumps(res["kernels"][-1]), flush=True)
    if not args.no_iteration:
        res["iteration"] = iteration(dev)
        print(json.dumps(res["iteration"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
