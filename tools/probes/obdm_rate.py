#!/usr/bin/env python3
"""What the one-body density matrix costs, in one process on the MI355X, 3 + 3 particles, nshells = 4:

  (a) ff_slater_sign and ff_obdm_accumulate beside ff_maps_accumulate at 128 bins on 65 536 walkers: median time per launch of
      back-to-back launches between two events (WINDOWS windows, the kernels alternating);
  (b) the benchmark's default training iteration (65 536 walkers) with model.obdm set and with None, alternating blocks of iterations
      in the same process, and the stages of one measure() -- moved batch, backward flows, log-density, signs, accumulation -- between
      events;
  (c) the diagonal block errors of rho on the benchmark's weights after SWEEPS sweeps of 16 384 walkers at sigma = 0.7, 1.0, 1.4, each
      with two seeds of r' (the same walkers for all six accumulators).

    python tools/probes/obdm_rate.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch      # noqa: E402

import __graft_entry__ as G      # noqa: E402
import fermiflow_amd as ff      # noqa: E402
from fermiflow_amd import native      # noqa: E402
from fermiflow_amd.utils import make_adam      # noqa: E402

WINDOWS = 11
SWEEPS = 24


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(dev, B=65536, nshells=4):
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=dev, generator=gen)
    x, rp = rnd(B, 6, 2) * 1.3, rnd(B, 2, 2)
    logp = -8.0 + 2.0 * rnd(B)
    lpm = logp[:, None] + 1.5 * rnd(B, 6)
    sg, sgm = torch.sign(rnd(B)), torch.sign(rnd(B, 6))
    tu = native.orbital_table([0, 1, 2], dev)
    obdm, maps = ff.OneBodyDensityMatrix(3, 3, nshells=nshells), ff.DensityMaps(3, 3, extent=6.0, nbins=128)
    fs = {"slater_sign": lambda: native.slater_sign(tu, tu, 3, 3, x), "obdm_accumulate": lambda: obdm.accumulate_raw(x, rp, logp, sg, lpm, sgm),
          "maps_accumulate": lambda: maps.accumulate(x)}
    for f in fs.values():
        window_us(f, 50)
    t = {k: [] for k in fs}
    for _ in range(WINDOWS):
        for k, f in fs.items():
            t[k].append(window_us(f, 1000))
    out = {"walkers": B, "nshells": nshells}
    for k, v in t.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    return out


def stages(model, obdm, B):
    """one measure() taken apart between events (the same calls in the same order)"""
    dev = model.x.device
    v = model.cnf.v_wrapper.v
    net = v.net(refresh=True)
    tu, td = native.orbital_table([0, 1, 2], dev), native.orbital_table([0, 1, 2], dev)
    x = model.x
    z, dl = native.cnf_delta_logp(net, x, 0.0, 1.0, model.cnf.rtol, model.cnf.atol)
    logp = native.logprob(tu, td, 3, 3, z) - dl
    n = 6
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    gen = torch.Generator(device=dev).manual_seed(5)
    ar = torch.arange(n, device=dev)
    species = (ar >= 3).to(torch.int64)
    res = []
    for _ in range(5):
        ev[0].record()
        rp = torch.randn(B, 2, 2, generator=gen, device=dev, dtype=torch.float64)
        xm = x[:, None].expand(B, n, n, 2).clone()
        xm[:, ar, ar] = rp[:, species]
        xm = xm.view(B * n, n, 2)
        ev[1].record()
        zm, dlm = native.cnf_delta_logp(net, xm, 0.0, 1.0, model.cnf.rtol, model.cnf.atol)
        ev[2].record()
        lpm = (native.logprob(tu, td, 3, 3, zm) - dlm).view(B, n)
        ev[3].record()
        sgm = native.slater_sign(tu, td, 3, 3, zm).view(B, n)
        sg = native.slater_sign(tu, td, 3, 3, z)
        ev[4].record()
        obdm.accumulate_raw(x, rp, logp, sg, lpm, sgm)
        ev[5].record()
        ev[5].synchronize()
        res.append([ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(5)])
    med = [round(statistics.median(r[k] for r in res), 1) for k in range(5)]
    return dict(zip(("moved_batch_us", "moved_flows_us", "logprob_us", "signs_us", "accumulate_us"), med))


def iteration(dev, B=65536, block=10, blocks=6):
    model = G._model(dev)
    opt = make_adam(model.parameters(), lr=2e-5)
    obdm = ff.OneBodyDensityMatrix(3, 3, nshells=4)
    torch.manual_seed(1234)

    def step():
        g = model(B)
        opt.zero_grad()
        g.backward()
        opt.step()

    def timed(m):
        model.obdm = m
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(block):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / block

    for _ in range(10):
        step()
    t_none, t_obdm = [], []
    for _ in range(blocks):
        t_none.append(timed(None))
        t_obdm.append(timed(obdm))
    model.obdm = None
    mn, mo = statistics.median(t_none), statistics.median(t_obdm)
    c = obdm.counts()
    out = {"walkers": B, "iteration_ms_none": round(mn, 4), "iteration_ms_obdm": round(mo, 4), "difference_ms": round(mo - mn, 4),
           "none_min_max": [round(min(t_none), 4), round(max(t_none), 4)], "obdm_min_max": [round(min(t_obdm), 4), round(max(t_obdm), 4)],
           "calls": c["calls"], "invalid": [c["invalid_up"], c["invalid_down"]], "trace": [float(np.trace(m)) for m in obdm.matrix().values()]}
    out["stages"] = stages(model, ff.OneBodyDensityMatrix(3, 3, nshells=4), B)
    return out


class _Fan:
    """model.obdm for several accumulators at once: the same sweeps feed them all"""

    def __init__(self, objs):
        self.objs = objs

    def on_sweep(self, *a, **k):
        for o in self.objs:
            o.on_sweep(*a, **k)


def sigmas(dev, B=16384):
    model = G._model(dev)
    objs = {(s, seed): ff.OneBodyDensityMatrix(3, 3, nshells=4, sigma=s, seed=seed) for s in (0.7, 1.0, 1.4) for seed in (0, 1)}
    model.obdm = _Fan(list(objs.values()))
    torch.manual_seed(99)
    for _ in range(SWEEPS):
        model(B)
    torch.cuda.synchronize()
    out = []
    for (s, seed), o in objs.items():
        err, rho = o.matrix_err(), o.matrix()
        out.append({"sigma": s, "seed": seed, "mean_diag_err_up": float(np.diag(err["up"]).mean()), "mean_diag_err_down": float(np.diag(err["down"]).mean()),
                    "max_diag_err": float(max(np.diag(err["up"]).max(), np.diag(err["down"]).max())),
                    "trace_up": float(np.trace(rho["up"])), "trace_down": float(np.trace(rho["down"])),
                    "occ_up": [round(float(v), 4) for v in o.occupations()["up"][0][:4]], "invalid": [o.counts()["invalid_up"], o.counts()["invalid_down"]]})
    return {"walkers": B, "sweeps": SWEEPS, "results": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("obdm_rate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0)}
    for key, fn in (("kernels", kernels), ("iteration", iteration), ("sigmas", sigmas)):
        res[key] = fn(dev)
        print(json.dumps({key: res[key]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
