#!/usr/bin/env python3
"""What a diffusion Monte Carlo step costs, in one process on the MI355X, at config 2 (3 + 3 particles, Z = 2, the
benchmark's synthetic flow, 65 536 walkers):

  steps per second of fermiflow_amd.DMC.run (blocks of STEPS steps between two host reads, median of WINDOWS blocks), and the small
  kernels alone -- ff_dmc_propose, ff_slater_sign, ff_dmc_accept and the three launches of ff_dmc_comb on the same population,
  back-to-back launches between two events -- as a share of the step.

    python tools/probes/dmc_rate.py [--batch 65536] [--out FILE.json]
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

import fermiflow_amd as ff      # noqa: E402
from fermiflow_amd import native      # noqa: E402
from __graft_entry__ import _model      # noqa: E402

WINDOWS = 7
STEPS = 20
REPS = 200


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dmc_rate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    B = args.batch
    dmc = ff.DMC(_model(dev), tau=0.005, steps_per_block=STEPS, seed=1)
    dmc.start(B)
    dmc.run(1)                                                   # warm-up
    blocks = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dmc.run(1)
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / STEPS * 1e6)
    step_us = statistics.median(blocks)
    # the pieces alone, on the population as it stands
    st, w = dmc._state, dmc.weights
    tu, td = dmc.model._tables(dev)
    x1, _ = native.dmc_propose(3, 3, st["x"], st["grad"], dmc.tau, 1.0, seed=1, step=0)
    with torch.no_grad():
        prop = dmc._guide(x1)
    z = dmc.model.local_energy(x1)["z"].clone()
    rec = torch.zeros(native.DMC_REC, dtype=torch.int64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    far = torch.ones(B, dtype=torch.float64, device=dev) * 2.0    # uniforms that accept nothing: the state stays put
    fs = {"propose": lambda: native.dmc_propose(3, 3, st["x"], st["grad"], dmc.tau, 1.0, seed=1, step=0, out=x1),
          "slater_sign": lambda: native.slater_sign(tu, td, 3, 3, z),
          "accept": lambda: native.dmc_accept(3, 3, dict(st, w=w), prop, dmc.tau, 1.0, dmc._ctrl, rec, 0, dmc._ws_accept, u=far),
          "comb": lambda: native.dmc_comb(3, 3, dict(st, w=w), dmc._spare, dmc._src, info, dmc._ws_comb, seed=1, step=0),
          "local_energy": lambda: dmc.model.local_energy(x1)}
    out = {"device": torch.cuda.get_device_name(0), "walkers": B, "step_us": round(step_us, 1), "step_us_min_max": [round(min(blocks), 1), round(max(blocks), 1)],
           "steps_per_second": round(1e6 / step_us, 1)}
    with torch.no_grad():
        for k, f in fs.items():
            window_us(f, 20)
            v = [window_us(f, REPS if k != "local_energy" else 30) for _ in range(WINDOWS)]
            out[k + "_us"] = round(statistics.median(v), 2)
    small = sum(out[k + "_us"] for k in ("propose", "slater_sign", "accept", "comb"))
    out["small_kernels_us"], out["small_kernels_share"] = round(small, 2), round(small / step_us, 4)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
