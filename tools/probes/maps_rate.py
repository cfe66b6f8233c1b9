#!/usr/bin/env python3
"""What the density maps cost, in one process on the MI355X:

  (a) ff_maps_accumulate against ff_observe_accumulate -- the radial histograms of the same walkers: the same bytes read, 21 LDS adds
      per walker where the maps issue 36, a histogram 13 times smaller to flush -- 3 + 3 particles in 2-D, 65 536 and 1 048 576
      walkers, maps of 64 and 128 bins: median time per launch of back-to-back launches between two events (WINDOWS windows, the two
      kernels alternating);
  (b) the benchmark's default training iteration (3 + 3 particles, 65 536 walkers) with model.density_maps set and with None,
      alternating blocks of iterations in the same process, median over the blocks.

    python tools/probes/maps_rate.py [--out FILE.json]
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
from fermiflow_amd.utils import make_adam      # noqa: E402

WINDOWS = 11


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(dev, B, extent, nbins):
    x = torch.randn(B, 6, 2, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 1.3
    maps = ff.DensityMaps(3, 3, extent=extent, nbins=nbins)
    obs = ff.Observables(3, 3, rmax=extent, nbins=240)
    fm, fo = (lambda: maps.accumulate(x)), (lambda: obs.accumulate(x))
    reps = 1000 if B <= (1 << 17) else 100
    for f in (fm, fo):
        window_us(f, 50)
    tm, to = [], []
    for _ in range(WINDOWS):
        tm.append(window_us(fm, reps))
        to.append(window_us(fo, reps))
    mm, mo = statistics.median(tm), statistics.median(to)
    occupied = int(sum((maps.counts()[k] > 0).sum() for k in ff.observables.PLANES))
    return {"walkers": B, "nbins": nbins, "maps_us": round(mm, 2), "observe_us": round(mo, 2), "ratio": round(mm / mo, 2),
            "maps_us_min_max": [round(min(tm), 2), round(max(tm), 2)], "observe_us_min_max": [round(min(to), 2), round(max(to), 2)],
            "occupied_cells": occupied}


def iteration(dev, B=65536, block=20, blocks=8):
    model = G._model(dev)
    opt = make_adam(model.parameters(), lr=2e-5)
    maps = ff.DensityMaps(3, 3)
    torch.manual_seed(1234)

    def step():
        g = model(B)
        opt.zero_grad()
        g.backward()
        opt.step()

    def timed(m):
        model.density_maps = m
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(block):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / block

    for _ in range(10):
        step()
    t_none, t_maps = [], []
    for _ in range(blocks):
        t_none.append(timed(None))
        t_maps.append(timed(maps))
    mn, mm = statistics.median(t_none), statistics.median(t_maps)
    return {"walkers": B, "iteration_ms_none": round(mn, 4), "iteration_ms_maps": round(mm, 4), "difference_us": round((mm - mn) * 1e3, 1),
            "none_min_max": [round(min(t_none), 4), round(max(t_none), 4)], "maps_min_max": [round(min(t_maps), 4), round(max(t_maps), 4)],
            "calls": maps.counts()["calls"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-iteration", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("maps_rate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    for B in (65536, 1 << 20):
        for nbins in (64, 128):
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
