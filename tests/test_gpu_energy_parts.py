"""The energy components on the MI355X: ff_energy_parts_accumulate against the numpy restatement (tests/energy_ref.py) with the bounds of
the host-simulator test, then inside GSVMC and BetaVMC sweeps -- against the sweep's own local energies, on a zero flow where every
component sum is known, and with the hook off."""
import numpy as np
import pytest
import torch

import fermiflow_amd as ff
from fermiflow_amd import EnergyParts, native
from tests import energy_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 2), (3, 3, 2), (2, 2, 3), (12, 12, 2)]
IDS = [f"{a}+{b}-{d}d" for a, b, d in SHAPES]
BMAX = 2 * R.CHUNK + 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _run(dev, inp, nup, ndn, d, Z, wstate=None, nstates=0, centre=None):
    """two fresh objects, one call each: bitwise equal; returns (accumulator words, parts of the call)"""
    tin = {k: _t(v, dev) for k, v in inp.items()}
    ws = None if wstate is None else _t(wstate, dev, torch.int32)
    objs = [EnergyParts(nup, ndn, Z, dim=d, nstates=nstates, centre=centre) for _ in range(2)]
    for o in objs:
        o.accumulate_raw(tin["x"], tin["grad"], tin["lap"], ws)
    torch.cuda.synchronize()
    a, b = (o._buf.cpu().numpy() for o in objs)
    assert np.array_equal(a, b) and objs[0].last.cpu().numpy().tobytes() == objs[1].last.cpu().numpy().tobytes()
    return a, objs[0].last.cpu().numpy(), objs[0]


def _check(dev, inp, nup, ndn, d, Z, wstate=None, nstates=0, centre=None):
    acc, po, obj = _run(dev, inp, nup, ndn, d, Z, wstate, nstates, centre)
    ref = R.reference(**inp, nup=nup, Z=Z, wstate=wstate, nstates=nstates, centre=centre)
    got = R.split(acc, nstates)
    return got, po, ref, max(R.compare(got, ref, nstates), R.compare_parts(po, ref)), obj


@pytest.mark.parametrize("nup,ndn,d", SHAPES, ids=IDS)
def test_kernel_against_numpy_on_the_device(dev, nup, ndn, d):
    """the hostsim cases at B in {65, 2 CHUNK + 3}, with the same bounds: Z = 0 and 2, three states with an empty one and a centre, every
    invalid rule; two runs on fresh buffers are bitwise equal"""
    full = R.inputs(300 + 7 * nup + ndn + d, BMAX, nup, ndn, d)
    worst = 0.0
    for B in (65, BMAX):
        inp = {k: v[:B] for k, v in full.items()}
        for Z in (0.0, 2.0):
            got, po, ref, w, obj = _check(dev, inp, nup, ndn, d, Z)
            worst = max(worst, w)
            assert obj.counts() == (1, B, 0)
            if Z == 0.0:
                assert not po[:, 3:].any()
        ws = R.states(9, B, 3, empty=(1,))
        centre = np.array([1.0, 2.0, 3.0, 0.5, 1.5, 0.25])
        got, po, ref, w, obj = _check(dev, inp, nup, ndn, d, 2.0, wstate=ws, nstates=3, centre=centre)
        worst = max(worst, w)
        assert got["count"].sum() == B and got["count"][1] == 0
        # the invalid rules
        bad, wb = {k: v.copy() for k, v in inp.items()}, ws.copy()
        bad["x"][5, 1, 0] = np.nan
        bad["lap"][40] = np.nan
        bad["x"][9, 1] = bad["x"][9, 0]
        wb[-1], wb[0] = 3, -1
        for Z, want in ((2.0, 5), (0.0, 4)):
            got, po, ref, w, obj = _check(dev, bad, nup, ndn, d, Z, wstate=wb, nstates=3)
            worst = max(worst, w)
            assert obj.counts() == (1, B - want, want) and got["count"].sum() == B - want
        with pytest.raises(ValueError):
            obj.accumulate_raw(*(_t(bad[k][:10], dev) for k in ("x", "grad", "lap")), _t(wb[:10], dev, torch.int32))      # equal calls only
    print(f"{nup}+{ndn} d={d}: largest error / bound {worst:.3e}")


@pytest.mark.parametrize("d", [2, 3])
def test_gaussian_inputs_against_the_restatement(dev, d):
    """the one-particle inputs of the statistical identities (checked on the CPU): here against the restatement only"""
    worst = 0.0
    for B in (65, BMAX, 4096):
        got, po, ref, w, obj = _check(dev, R.gaussian_inputs(B, d), 1, 0, d, 0.0)
        worst = max(worst, w)
        assert obj.counts() == (1, B, 0)
    print(f"d={d}: largest error / bound {worst:.3e}")


def _spy(monkeypatch):
    """records what the sweeps' native.eloc calls take and leave: x, grad, lap, V, eloc of every call, cloned"""
    seen, real = [], native.eloc

    def eloc(*a, **k):
        r = real(*a, **k)
        seen.append({"x": a[5].clone(), **{key: r[key].clone() for key in ("grad", "lap", "V", "eloc")}})
        return r
    monkeypatch.setattr(native, "eloc", eloc)
    return seen


def _sum_of(refs):
    """the reference of several calls on one buffer: the fields add, the bounds add and every later addition to the accumulator rounds once"""
    out = dict(calls=len(refs), walkers=sum(r["walkers"] for r in refs), invalid=sum(r["invalid"] for r in refs))
    for name in ("sum", "sum2", "blocksq"):
        out[name] = sum(r[name] for r in refs)
        out["b_" + name] = sum(r["b_" + name] for r in refs) + (len(refs) - 1) * R.LD(R.U) * sum(np.abs(r[name]) for r in refs)
    return out


def test_inside_a_gsvmc_sweep(dev, monkeypatch):
    """3 + 3, the benchmark's weights, 1024 walkers, two sweeps: the buffer equals the restatement on the sweeps' own x, grad and lap, and
    per walker the components add up to the sweep's E_loc and V within 1e-12 of the scale of their terms (fewer than a hundred fp64
    roundings on either path, each at most 2^-53 of that scale)."""
    from __graft_entry__ import _model
    B = 1024
    model = _model(dev)
    for kw in (dict(Z=1.0), dict(nup=2), dict(ndown=2), dict(dim=3), dict(nstates=4)):
        args = {**dict(nup=3, ndown=3, Z=2.0, dim=2, nstates=0), **kw}
        with pytest.raises(ValueError):
            model.energy_parts = EnergyParts(args.pop("nup"), args.pop("ndown"), args.pop("Z"), **args)      # before any launch
    assert model.energy_parts is None
    parts = EnergyParts(3, 3, 2.0)
    model.energy_parts = parts
    seen = _spy(monkeypatch)
    torch.manual_seed(11)
    for _ in range(2):
        model(B).backward()
    torch.cuda.synchronize()
    assert len(seen) == 2 and parts.counts() == (2, 2 * B, 0)
    host = [{k: v.cpu().numpy() for k, v in s.items()} for s in seen]
    assert np.array_equal(host[1]["x"], model.x.cpu().numpy()) and np.array_equal(host[1]["eloc"], model.Eloc.cpu().numpy())
    refs = [R.reference(h["x"], h["grad"], h["lap"], nup=3, Z=2.0) for h in host]
    got = R.split(parts._buf.cpu().numpy())
    ref = _sum_of(refs)
    assert (got["calls"], got["walkers"], got["invalid"], got["ticket"]) == (2, 2 * B, 0, 0)
    worst = 0.0
    for name in ("sum", "sum2", "blocksq"):
        err = np.abs(got[name].astype(R.LD) - ref[name])
        assert (err <= ref["b_" + name]).all(), name
        worst = max(worst, float((err / ref["b_" + name]).max()))
    c, h = parts.last.cpu().numpy(), host[1]
    worst = max(worst, R.compare_parts(c, refs[1]))
    vee = c[:, 3] + c[:, 4] + c[:, 5]
    gg = (h["grad"] ** 2).sum((1, 2))
    r1 = np.abs(c[:, 0] + c[:, 2] + vee - h["eloc"]) / (np.abs(h["lap"]) / 4 + gg / 8 + c[:, 2] + vee + 1)
    r2 = np.abs(c[:, 2] + vee - h["V"]) / (h["V"] + 1)
    print(f"largest error / bound {worst:.3e}; |sum of parts - E_loc| / scale {r1.max():.3e}, |V_trap + V_ee - V| / scale {r2.max():.3e}")
    assert (r1 <= 1e-12).all() and (r2 <= 1e-12).all()
    m, e = parts.means(), parts.errors()
    # the mean energy is the mean of the sweeps' local energies: the per-walker bar above on average, and the roundings of two sums of 2 B terms
    scale = np.concatenate([np.abs(q["lap"]) / 4 + (q["grad"] ** 2).sum((1, 2)) / 8 + np.abs(q["V"]) + 1 for q in host])
    e_all = np.concatenate([q["eloc"] for q in host]).astype(R.LD)
    assert abs(m["E"] - float(e_all.mean())) <= 1e-12 * scale.mean() + 2 * (2 * B) * R.U * float(np.abs(e_all).mean())
    assert all(np.isfinite(v) for v in m.values()) and all(np.isfinite(v) and v >= 0 for v in e.values())
    # the potentials are attributes too: another Z behind the object's back is refused by the sweep
    model.pair_potential = ff.CoulombPairPotential(1.0)
    with pytest.raises(ValueError):
        model(B)
    assert parts.counts() == (2, 2 * B, 0)


def _zero_flow(model):
    v = model.cnf.v_wrapper.v
    v.eta.init_zeros()
    v.mu.init_zeros()
    return model


def test_zero_flow_without_interaction(dev):
    """Zero eta and mu, CoulombPairPotential(0): the walkers sample the free ground state of 3 + 3, an eigenfunction, so T_L + V_trap = 10
    (orbital energies 1 + 2 + 2 per species) for every walker within 1e-9 -- the project's eigenfunction bar, the one test_gpu_parity.py
    holds ff_logprob to -- and V_ee is exactly 0.  The virial residual and dT are printed with their errors, not asserted: their law
    depends on the sampler."""
    from __graft_entry__ import _model
    B = 1024
    model = _zero_flow(_model(dev, Z=0.0))
    parts = EnergyParts(3, 3, 0.0)
    model.energy_parts = parts
    torch.manual_seed(5)
    model(B)
    torch.cuda.synchronize()
    calls, walkers, invalid = parts.counts()
    assert calls == 1 and walkers + invalid == B and walkers > 0
    c = parts.last.cpu().numpy()
    ok = np.isfinite(c).all(1)
    assert ok.sum() == walkers
    assert (np.abs(c[ok, 0] + c[ok, 2] - 10.0) <= 1e-9).all()
    assert not c[:, 3:].any()
    m, e = parts.means(), parts.errors()
    assert m["V_ee"] == 0.0 and e["V_ee"] == 0.0 and abs(m["E"] - 10.0) <= 1e-9
    assert np.isnan(parts.dE_dZ()[0])
    print(f"zero flow: E = {m['E']:.12f}; virial {m['virial']:+.4f} +- {e['virial']:.4f}, dT {m['dT']:+.4f} +- {e['dT']:.4f}, "
          f"T_L {m['T_L']:.4f} +- {e['T_L']:.4f}, V_trap {m['V_trap']:.4f} +- {e['V_trap']:.4f}; invalid {invalid}")


def test_inside_a_betavmc_sweep(dev):
    """nup = 3, ndown = 0, deltaE = 2, a zero flow and Z = 0: every walker of state s has E_loc = Es_original[s], so per_state()["E"][s]
    equals it within 1e-9 for every state that drew walkers, the counts are the sweep's own, and the spread is zero within rounding:
    with the moments about zero the variance sumE2 / n - mean^2 cancels two numbers of size E^2; sumE2 / n carries at most n + 12
    roundings of E^2 and mean^2 twice as many (the depth n + 10 of tests/energy_ref.py for a state's sums, the division, the square),
    so E_err^2 (n - 1) <= 3 (n + 12) 2^-53 E^2 + (1e-9)^2, the last for what the walkers' energies themselves may be off by."""
    B, nup = 512, 3
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 50), mu=ff.MLP(1, 50)), (0.0, 1.0))
    model = ff.BetaVMC(2.0, nup, 0, 2.0, True, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(0.0), sp_potential=ff.HO())
    _zero_flow(model).to(device=dev)
    Ns = len(model.Es_original)
    assert Ns > 1
    with pytest.raises(ValueError):
        model.energy_parts = EnergyParts(nup, 0, 0.0, nstates=Ns + 1)
    parts = EnergyParts(nup, 0, 0.0, nstates=Ns)
    model.energy_parts = parts
    torch.manual_seed(7)
    model(B)
    torch.cuda.synchronize()
    calls, walkers, invalid = parts.counts()
    assert calls == 1 and walkers + invalid == B
    ws = model._ws.cpu().numpy()
    c = parts.last.cpu().numpy()
    ok = np.isfinite(c).all(1)
    ps = parts.per_state()
    assert np.array_equal(ps["count"], np.bincount(ws[ok], minlength=Ns)) and ps["count"].sum() == walkers
    if invalid == 0:
        assert np.array_equal(ps["count"], np.bincount(ws, minlength=Ns))
    Es = model.Es_original.cpu().numpy()
    drew = ps["count"] > 0
    assert drew.sum() > 1
    assert (np.abs(ps["E"][drew] - Es[drew]) <= 1e-9).all()
    two = ps["count"] > 1
    n = ps["count"][two].astype(np.float64)
    tol = np.sqrt((3 * (n + 12) * R.U * Es[two] ** 2 + 1e-18) / (n - 1))
    print(f"BetaVMC: {int(drew.sum())} of {Ns} states drew walkers; max |E_s - Es_original| {np.abs(ps['E'][drew] - Es[drew]).max():.3e}, "
          f"max E_err {ps['E_err'][two].max():.3e} (allowed {tol.max():.3e}); invalid {invalid}")
    assert (ps["E_err"][two] <= tol).all() and np.isnan(ps["E_err"][drew & ~two]).all()
    assert not c[:, 3:].any()


def test_the_hook_off_changes_nothing(dev):
    """model.energy_parts = None: E, E_std and every .grad of a sweep are bitwise those of a model that never had the attribute set --
    and those of a model that has it set, for the hook only reads."""
    from __graft_entry__ import _model
    out = []
    for mode in ("never", "none", "set"):
        model = _model(dev)
        if mode == "none":
            model.energy_parts = EnergyParts(3, 3, 2.0)
            model.energy_parts = None
        elif mode == "set":
            model.energy_parts = EnergyParts(3, 3, 2.0)
        torch.manual_seed(4)
        model(256).backward()
        torch.cuda.synchronize()
        out.append((np.float64(model.E).tobytes(), np.float64(model.E_std).tobytes(), model.Eloc.cpu().numpy().tobytes(),
                    [p.grad.cpu().numpy().tobytes() for p in model.parameters()]))
    assert out[0] == out[1] == out[2]
