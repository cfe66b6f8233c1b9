#!/usr/bin/env python3
"""What the energy components cost, in one process on the MI355X, on 65 536 walkers:

  ff_energy_parts_accumulate at 3 + 3 and at 12 + 12 particles in two dimensions, without states and with per-state sums (16 states: the
  second launch), beside ff_maps_accumulate at 128 bins on the same walkers: median time per launch of back-to-back launches between two
  events (WINDOWS windows, the kernels alternating).  The same call on 256 walkers (one chunk) is the floor of a call: the Python method,
  the launch and the kernel's fixed parts; a launch time below it says how fast the host enqueues, not how fast the kernel runs.

    python tools/probes/energy_parts_rate.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch      # noqa: E402

import fermiflow_amd as ff      # noqa: E402

WINDOWS = 11
REPS = 400
NSTATES = 16


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(dev, nup, ndn, B=65536, Z=2.0):
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=dev, generator=gen)
    n = nup + ndn
    x, grad, lap = rnd(B, n, 2) * 1.3, rnd(B, n, 2) * 2.0, -4.0 * n + 3.0 * rnd(B)
    ws = torch.sort(torch.randint(0, NSTATES, (B,), device=dev, generator=gen)).values.to(torch.int32)
    plain, states, free = ff.EnergyParts(nup, ndn, Z), ff.EnergyParts(nup, ndn, Z, nstates=NSTATES), ff.EnergyParts(nup, ndn, 0.0)
    maps = ff.DensityMaps(nup, ndn, extent=6.0, nbins=128)
    floor = ff.EnergyParts(nup, ndn, Z)
    xs, gs, ls = x[:256].contiguous(), grad[:256].contiguous(), lap[:256].contiguous()
    fs = {"energy_parts": lambda: plain.accumulate_raw(x, grad, lap), "energy_parts_states": lambda: states.accumulate_raw(x, grad, lap, ws),
          "energy_parts_Z0": lambda: free.accumulate_raw(x, grad, lap), "maps_accumulate": lambda: maps.accumulate(x),
          "energy_parts_256_walkers": lambda: floor.accumulate_raw(xs, gs, ls)}
    for f in fs.values():
        window_us(f, 50)
    t = {k: [] for k in fs}
    for _ in range(WINDOWS):
        for k, f in fs.items():
            t[k].append(window_us(f, REPS))
    out = {"walkers": B, "nup": nup, "ndown": ndn, "nstates": NSTATES, "bytes_read": B * (2 * n * 2 + 1) * 8}
    for k, v in t.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    torch.cuda.synchronize()
    out["counts"] = list(plain.counts())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("energy_parts_rate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0)}
    for nup, ndn in ((3, 3), (12, 12)):
        key = f"{nup}+{ndn}"
        res[key] = kernels(dev, nup, ndn)
        print(json.dumps({key: res[key]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
