#!/usr/bin/env python3
"""What a flow trajectory costs, in one process on the MI355X: CNF.generate(z, nframes = K) as ONE call of
ff_cnf_generate_frames against K - 1 chained calls of ff_cnf_generate over the sub-intervals (t_k, t_k+1) -- what the frames
would cost without the kernel -- on the same base walkers and the benchmark's flow (65 536 x 6 particles in 2-D, K = 50).
Median over RUNS runs between two device events after a warm-up, and the right-hand-side evaluations per walker (stats[0] / B).

    python tools/probes/frames_rate.py [--walkers B] [--nframes K] [--chained-only] [--out FILE.json]

--chained-only: for a library without the symbol (FERMIFLOW_LIB=<an older build>)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch      # noqa: E402

import __graft_entry__ as G      # noqa: E402
from fermiflow_amd import _lib      # noqa: E402
from fermiflow_amd import _lib as L      # noqa: E402

RUNS = 20


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--nframes", type=int, default=50)
    ap.add_argument("--chained-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frames_rate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = G._model(dev)
    torch.manual_seed(1234)
    B, K = args.walkers, args.nframes
    z = model.basedist.sample(model.orbitals_up, model.orbitals_down, (B,))
    cnf = model.cnf
    net = cnf.v_wrapper.v.net()
    t0, t1 = cnf.t_span
    ts = [t1 if k == K - 1 else t0 + k * ((t1 - t0) / (K - 1)) for k in range(K)]

    # every buffer of both legs is allocated once, outside the timed regions; the legs call the C ABI directly
    lib, st = L.lib(), L.stream()
    odes = [L.ode(ts[k - 1], ts[k], cnf.rtol, cnf.atol) for k in range(1, K)]
    ode_all = L.ode(t0, t1, cnf.rtol, cnf.atol)
    fr_one = torch.empty((K,) + tuple(z.shape), dtype=torch.float64, device=dev)
    fr_ch = torch.empty_like(fr_one)
    st_one = torch.zeros(32, dtype=torch.int32, device=dev)
    st_ch = torch.zeros(32, dtype=torch.int32, device=dev)          # (stats accumulate: one buffer for the K - 1 calls)
    n, d = z.shape[1], z.shape[2]
    fr_ch[0] = z

    def one_call():
        L.check(lib.ff_cnf_generate_frames(st, B, n, d, net.ref(), C.byref(ode_all), L.ptr(z), K, L.ptr(fr_one), L.ptr(st_one)), "frames")
        return fr_one, st_one

    def chained():
        for k in range(1, K):
            L.check(lib.ff_cnf_generate(st, B, n, d, net.ref(), C.byref(odes[k - 1]), L.ptr(fr_ch[k - 1]), L.ptr(fr_ch[k]), L.ptr(st_ch)), "generate")
        return fr_ch, st_ch

    res = {"device": torch.cuda.get_device_name(0), "library": _lib.LIB_PATH, "walkers": B, "nframes": K, "runs": RUNS}
    todo = [("chained", chained)] + ([] if args.chained_only else [("one_call", one_call)])
    outs = {}
    for name, fn in todo:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in todo}
    for _ in range(RUNS):          # (alternating, so that drift of the machine hits both alike)
        for name, fn in todo:
            (st_ch if name == "chained" else st_one).zero_()
            ms, outs[name] = timed_ms(fn)
            times[name].append(ms)
    for name, _ in todo:
        t = times[name]
        nev = outs[name][1][0]
        res[name] = {"median_ms": round(statistics.median(t), 4), "min_max_ms": [round(min(t), 4), round(max(t), 4)],
                     "rhs_evaluations_per_walker": round(float(nev) / B, 2)}
    if "one_call" in outs:
        res["max_abs_difference_of_the_frames"] = float((outs["one_call"][0] - outs["chained"][0]).abs().max())
        res["one_call"]["failed"] = int(outs["one_call"][1][3])
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
