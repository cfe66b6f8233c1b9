"""The kernels at batch sizes that loop their persistent grids (tests/common.py kernel_families): every workgroup of every family
involved handles a second walker group and the last group is ragged, so LDS tables shared across groups, deposit tickets, s_st
statistics, queue counters, per-wave scratch reused by the next group and the reduction over many private tables all run.

Three checks per shape, on a probe set S of walkers chosen at the grid's seams (tests/common.py probe_set):
  * S against the oracle (GPU rtol 1e-9 / atol 1e-11, oracle 1e-10 / 1e-12);
  * S bit-identical between the looping batch and a batch of S alone (outputs and per-walker step counts): nothing a walker
    computes may depend on the batch size or on its place in the grid;
  * the theta-gradient at full size with seeds that are exactly zero outside S (plain, energy-seeded, energy-seeded with a
    per-state mean): the exact answer is the oracle's gradient of S alone, gx is exactly 0 outside S, and the full-size gp
    equals the gp of the S-only call to rounding -- the last isolates the reduction over the private tables.

Observed maxima over all shapes on an MI355X, and the bars (about 10x, never above the bars of test_gpu_parity.py):
  flow x / z / dlogp (absolute)               3.6e-10 / 3.4e-10 / 1.2e-9 (dlogp of the 10+10 3-D local energy)   bar 1e-8
  E_loc, lap (relative per walker)            2.4e-9 (7+6), 5.8e-10                                                bar 3e-8
  grad, glogp0 (relative to the largest)      4.1e-10                                                              bar 5e-9
  fp32 sensitivities (10+10 3-D): E_loc 1.6e-6, lap 5.7e-7, grad 3.1e-7                                            bars 1e-5, 3e-6
  gp, gx (relative to the largest)            4.1e-9 (6+6), 2.6e-9 (12+12)                                         bar 5e-8
  full-size gp against the S-only gp          6.8e-16                                                              bar 1e-12
  off-table batch: x 2.6e-10, E_loc 1.1e-8 (4+4), gx 1.0e-9                                                        bars 1e-8, 1e-7, 5e-8

The one launch-wide decision: when any walker's trajectory meets a radius beyond the radial table (r > 32,
ff_radial.h), the table kernel hands the WHOLE launch to the direct kernel behind it, whose arithmetic differs in the last bits.
A batch of 32 769 random 12+12 walkers holds such walkers (one reaches a pair distance of 33.4 on its way from x to z; the batch
falls back without it too): that launch is served by the direct kernel while the probe walkers alone are not, and every walker
differed by ~1e-15.  Walkers whose trajectory ends leave the table's inner 24 are replaced (in_table), which does not clear the
12+12 batch, so the local-energy test asserts the decision exactly: S of the full launch is bit-identical either to the S-only
launch (table kernels served both) or to the exact net's S-only launch (the launch fell back).  The S-only launches must be
served by the table kernels.  The fallback is also tested on purpose at a looping size in test_off_table_fallback_at_looping_batch.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.common import (N, T, assert_loops, cu_count, kernel_families, looping_batch, make_flow, net_arrays, probe_set)

pytestmark = pytest.mark.gpu

RT, AT = 1e-9, 1e-11            # GPU solves
ORT, OAT = 1e-10, 1e-12         # oracle solves
# bars (first column: flow x / z / dlogp, absolute; then eloc relative per walker, grad / glogp0 relative to the largest entry,
# lap relative per walker, gp / gx relative to the largest entry); see the module docstring
BAR_FLOW = 1e-8
BAR_ELOC = 3e-8
BAR_GRAD = 5e-9
BAR_ELOC32, BAR_GRAD32 = 1e-5, 3e-6
BAR_GP = 5e-8
BAR_OFF_ELOC = 1e-7

SHAPES = [(1, 0, 2), (2, 1, 2), (2, 2, 2), (3, 2, 2), (3, 3, 2), (4, 3, 2), (4, 4, 2), (5, 4, 2), (5, 5, 2), (6, 5, 2), (6, 6, 2),
          (7, 6, 2), (12, 12, 2), (2, 1, 3), (2, 2, 3), (5, 4, 3), (10, 10, 3)]
IDS = [f"{a}+{b}_{d}d" for a, b, d in SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(golden):
    eta, mu = net_arrays(golden["g5_gsvmc"], "z2_nt_")
    return eta, mu, O.Net(eta, mu)


_CASES = {}


def _case(dev, nets, nup, ndn, d):
    """(B, S, z, x, net, exact, fams) of one shape: B loops every family of the three calls at least twice with a ragged end
    (asserted); z (flow and adjoint) and x (local energy) are walkers whose trajectories stay well inside the radial table."""
    key = (nup, ndn, d)
    if key not in _CASES:
        n = nup + ndn
        cus = cu_count()
        fams = {}
        for call in ("flow", "eloc", "adjoint"):
            fams.update(kernel_families(call, n, d, cus))
        B = looping_batch(fams)
        assert_loops(fams, B)
        big = n * d >= 40            # (the oracle takes seconds per walker there: the seams of the first and last round only)
        S = probe_set(B, fams, seed=n * d, nrand=2 if big else 12, edge_rounds=1 if big else 3)
        g = torch.Generator().manual_seed(1000 + 10 * n + d)
        z = torch.randn(B, n, d, generator=g, dtype=torch.float64).to(dev)
        v = make_flow(nets[0], nets[1], dev).v_wrapper.v
        net, exact = v.net(radial="table"), v.net(radial="exact")
        from fermiflow_amd import native
        z = in_table(z, native.cnf_generate(exact, z, 0.0, 1.0, RT, AT))
        x = z * 1.1
        x = in_table(x, native.cnf_delta_logp(exact, x, 0.0, 1.0, RT, AT)[0])
        _CASES[key] = (B, S, z, x, net, exact, fams)
    return _CASES[key]


def in_table(y0, y1, rmax=24.0):
    """y0 with every walker whose pair distances at either end of its flow trajectory (y0, y1) exceed rmax (the table ends at 32)
    replaced by a copy of an in-range walker."""
    far = (torch.cdist(y0, y0).flatten(1).max(1).values > rmax) | (torch.cdist(y1, y1).flatten(1).max(1).values > rmax)
    if bool(far.any()):
        y0 = y0.clone()
        near = (~far).nonzero().squeeze(1)
        bad = far.nonzero().squeeze(1)
        y0[bad] = y0[near[torch.arange(len(bad), device=y0.device) % len(near)]]
    return y0


def _rel_max(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _tables(nup, ndn, dev):
    from fermiflow_amd import native
    return (native.orbital_table(list(range(nup)), dev) if nup else None,
            native.orbital_table(list(range(ndn)), dev) if ndn else None)


@pytest.mark.parametrize("nup,ndn,d", SHAPES, ids=IDS)
def test_flow_at_looping_batch_vs_oracle(dev, nets, nup, ndn, d):
    from fermiflow_amd import native
    B, S, z, _, net, exact, fams = _case(dev, nets, nup, ndn, d)
    Si = torch.as_tensor(S, device=dev)
    c_full, c_sub = (torch.full((m,), -1, dtype=torch.int32, device=dev) for m in (B, len(S)))
    x = native.cnf_generate(net, z, 0.0, 1.0, RT, AT, walker_cost=c_full)
    xs = native.cnf_generate(net, z[Si].contiguous(), 0.0, 1.0, RT, AT, walker_cost=c_sub)
    assert torch.equal(x[Si], xs) and torch.equal(c_full[Si], c_sub)
    d_full, d_sub = (torch.full((m,), -1, dtype=torch.int32, device=dev) for m in (B, len(S)))
    zb, dl = native.cnf_delta_logp(net, x, 0.0, 1.0, RT, AT, walker_cost=d_full)
    zbs, dls = native.cnf_delta_logp(net, x[Si].contiguous(), 0.0, 1.0, RT, AT, walker_cost=d_sub)
    assert torch.equal(zb[Si], zbs) and torch.equal(dl[Si], dls) and torch.equal(d_full[Si], d_sub)
    # the table kernels served both launches (a fallback to the direct kernel would give the exact net's results)
    assert not torch.equal(x[Si], native.cnf_generate(exact, z[Si].contiguous(), 0.0, 1.0, RT, AT))
    assert not torch.equal(dl[Si], native.cnf_delta_logp(exact, x[Si].contiguous(), 0.0, 1.0, RT, AT)[1])
    xo, _ = O.cnf_generate(N(z[Si]), nets[2], rtol=ORT, atol=OAT)
    zo, dlo, _ = O.cnf_delta_logp(N(x[Si]), nets[2], rtol=ORT, atol=OAT)
    ex, ez, ed = (float(np.abs(a - b).max()) for a, b in ((N(xs), xo), (N(zbs), zo), (N(dls), dlo)))
    print(f"GEOM flow {nup}+{ndn} {d}d B={B} |S|={len(S)} {sorted(fams)}: x {ex:.2e} z {ez:.2e} dlogp {ed:.2e}")
    assert max(ex, ez, ed) < BAR_FLOW


ELOC_CASES = [s + (64,) for s in SHAPES] + [(10, 10, 3, 32)]


@pytest.mark.parametrize("nup,ndn,d,bits", ELOC_CASES, ids=[f"{a}+{b}_{d}d_sens{s}" for a, b, d, s in ELOC_CASES])
def test_local_energy_at_looping_batch_vs_oracle(dev, nets, nup, ndn, d, bits):
    from fermiflow_amd import native
    B, S, _, x, net, exact, fams = _case(dev, nets, nup, ndn, d)
    Si = torch.as_tensor(S, device=dev)
    tu, td = _tables(nup, ndn, dev)
    Z = 1.0
    prev = native.set_sens_precision(bits)
    try:
        c_full, c_sub = (torch.full((m,), -1, dtype=torch.int32, device=dev) for m in (B, len(S)))
        r = native.eloc(tu, td, nup, ndn, net, x, 0.0, 1.0, RT, AT, Z, True, walker_cost=c_full)
        rs = native.eloc(tu, td, nup, ndn, net, x[Si].contiguous(), 0.0, 1.0, RT, AT, Z, True, walker_cost=c_sub)
        # queue order by the cost classes of the flow pass (what the sweeps do): the same results for every walker
        order = native.walker_order(c_full)
        ro = native.eloc(tu, td, nup, ndn, net, x, 0.0, 1.0, RT, AT, Z, True, walker_order=order)
        re = native.eloc(tu, td, nup, ndn, exact, x[Si].contiguous(), 0.0, 1.0, RT, AT, Z, True)
        torch.cuda.synchronize()
    finally:
        native.set_sens_precision(prev)
    assert not torch.equal(order, torch.arange(B, dtype=torch.int32, device=dev))
    assert not torch.equal(rs["lap"], re["lap"])        # the table kernels served the S-only launch
    # the full launch: served by the table kernels (S bit-identical to the S-only launch) or, by the launch-wide off-table decision,
    # by the direct kernel -- then S is bit-identical to the exact net's S-only launch (see the module docstring)
    fell_back = torch.equal(r["lap"][Si], re["lap"])
    want = re if fell_back else rs
    for k in ("logp", "grad", "lap", "V", "eloc", "z", "dlogp", "glogp0"):
        assert torch.equal(r[k][Si], want[k]), k
        assert torch.equal(ro[k], r[k]), k
    if not fell_back:
        assert torch.equal(c_full[Si], c_sub)
    xs = N(x[Si])
    ref = (O.eloc if d == 2 else O.eloc3d)(xs, nup, ndn, nets[2], Z, rtol=ORT, atol=OAT)
    zo, dlo, _ = O.cnf_delta_logp(xs, nets[2], rtol=ORT, atol=OAT)
    _, g0o, _ = (O.logprob if d == 2 else O.logprob3d)(zo, nup, ndn)
    g = {k: N(rs[k]) for k in rs}
    e_el = float((np.abs(g["eloc"] - ref["eloc"]) / np.abs(ref["eloc"])).max())
    e_lap = float((np.abs(g["lap"] - ref["lap"]) / np.maximum(np.abs(ref["lap"]), 1.0)).max())
    e_gr, e_g0 = _rel_max(g["grad"], ref["grad"]), _rel_max(g["glogp0"], g0o)
    e_z, e_dl = float(np.abs(g["z"] - zo).max()), float(np.abs(g["dlogp"] - dlo).max())
    print(f"GEOM eloc {nup}+{ndn} {d}d sens{bits} B={B} |S|={len(S)} {sorted(fams)} full launch fell back: {fell_back}: eloc {e_el:.2e} grad {e_gr:.2e} lap {e_lap:.2e} "
          f"z {e_z:.2e} dlogp {e_dl:.2e} glogp0 {e_g0:.2e}")
    be, bg = (BAR_ELOC, BAR_GRAD) if bits == 64 else (BAR_ELOC32, BAR_GRAD32)
    assert e_el < be and e_lap < be
    assert e_gr < bg and e_g0 < bg
    assert e_z < BAR_FLOW and e_dl < BAR_FLOW


@pytest.mark.parametrize("nup,ndn,d", SHAPES, ids=IDS)
def test_masked_seed_adjoint_at_looping_batch_vs_oracle(dev, nets, nup, ndn, d):
    """ff_cnf_adjoint and ff_cnf_adjoint_energy (one mean, and mean_index) at a looping B with seeds that are exactly zero outside
    S.  The energies are dyadic (E = e_mean + k / 64, scale = 2^-10) so that w_b = (E_b - e_mean) * scale is exact and the same
    in all three calls: one oracle solve of S serves them all."""
    from fermiflow_amd import native
    B, S, z, _, net, exact, fams = _case(dev, nets, nup, ndn, d)
    Si = torch.as_tensor(S, device=dev)
    n = nup + ndn
    rng = np.random.RandomState(7 + n)
    inS = np.zeros(B, dtype=bool); inS[S] = True
    k = np.where(inS, rng.randint(1, 257, size=B) * rng.choice([-1, 1], size=B), 0)
    e_mean, scale = 2.5, 2.0 ** -10
    w = (k / 64.0) * scale
    e_one = e_mean + k / 64.0
    e_vec = np.array([1.0, 1.5, 2.25, 3.0, 4.75])
    mi = rng.randint(0, len(e_vec), size=B).astype(np.int32)
    e_idx = e_vec[mi] + k / 64.0
    assert np.array_equal((e_one - e_mean) * scale, w) and np.array_equal((e_idx - e_vec[mi]) * scale, w)
    g0 = torch.randn(B, n, d, generator=torch.Generator().manual_seed(n), dtype=torch.float64).to(dev)
    wd = T(w, dev)
    a_z, a_d = wd[:, None, None] * g0, -wd
    costs = [torch.full((B,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
    runs = {
        "plain": native.cnf_adjoint(net, z, a_z, a_d, 0.0, 1.0, RT, AT, walker_cost=costs[0]),
        "energy": native.cnf_adjoint(net, z, g0, None, 0.0, 1.0, RT, AT, walker_cost=costs[1],
                                     energy=(T(e_one, dev), torch.tensor([e_mean], dtype=torch.float64, device=dev), scale)),
        "mean_index": native.cnf_adjoint(net, z, g0, None, 0.0, 1.0, RT, AT, walker_cost=costs[2],
                                         energy=(T(e_idx, dev), T(e_vec, dev), scale, T(mi, dev, torch.int32))),
    }
    c_sub = torch.full((len(S),), -1, dtype=torch.int32, device=dev)
    gx_s, gp_s = native.cnf_adjoint(net, z[Si].contiguous(), a_z[Si].contiguous(), a_d[Si].contiguous(), 0.0, 1.0, RT, AT,
                                    walker_cost=c_sub)
    gx_e, _ = native.cnf_adjoint(exact, z[Si].contiguous(), a_z[Si].contiguous(), a_d[Si].contiguous(), 0.0, 1.0, RT, AT)
    assert not torch.equal(gx_s, gx_e)                  # the table kernels served
    gxo, gpo, _ = O.cnf_adjoint(N(z[Si]), np.zeros(len(S)), N(a_z[Si]), N(a_d[Si]), nets[2], rtol=ORT, atol=OAT)
    out = N(gx_s)
    errs = []
    for name, (gx, gp) in runs.items():
        gxn, gpn = N(gx), N(gp)
        assert not gxn[~inS].any(), name                        # exactly zero outside S
        assert np.array_equal(gxn[S], out), name               # S bit-identical to the S-only call
        e_gp, e_gx = _rel_max(gpn, gpo), _rel_max(gxn[S], gxo)
        e_red = _rel_max(gpn, N(gp_s))                          # the reduction alone: full size vs S only
        errs.append((name, e_gp, e_gx, e_red))
        assert e_gp < BAR_GP and e_gx < BAR_GP, (name, e_gp, e_gx)
        assert e_red < 1e-12, (name, e_red)
    for c in costs:
        assert torch.equal(c[Si], c_sub)
    print(f"GEOM adjoint {nup}+{ndn} {d}d B={B} |S|={len(S)} {sorted(fams)}: " +
          " ".join(f"{nm}: gp {a:.2e} gx {b:.2e} full-vs-S {c:.1e}" for nm, a, b, c in errs))


@pytest.mark.parametrize("nup,ndn", [(3, 3), (4, 4)])
def test_off_table_fallback_at_looping_batch(dev, nets, nup, ndn):
    """One walker far off the radial table (the clusters of test_off_table_radii_are_served_by_the_direct_kernels) at index
    B - 1 of a batch whose fallback grids (grid-stride direct kernels behind the table kernels) loop: the table net and the exact
    net then give bit-identical results for the flow, the local energy and the adjoint, and S matches the oracle."""
    from fermiflow_amd import native
    n, d = nup + ndn, 2
    cus = cu_count()
    fams = {}
    for call in ("flow_fb", "eloc_fb", "adj_fb"):
        fams.update(kernel_families(call, n, d, cus))
    B = looping_batch(fams)
    assert_loops(fams, B)
    S = probe_set(B, fams, seed=5, nrand=8)
    Si = torch.as_tensor(S, device=dev)
    v = make_flow(nets[0], nets[1], dev).v_wrapper.v
    tab, exact = v.net(radial="table"), v.net(radial="exact")
    tu, td = _tables(nup, ndn, dev)
    z = torch.randn(B, n, d, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dev)
    z[B - 1, ::2, 0] += 17.0
    z[B - 1, 1::2, 0] -= 17.0
    assert torch.cdist(z[B - 1:], z[B - 1:]).max() > 33
    xt, xe = (native.cnf_generate(nt, z, 0.0, 1.0, RT, AT) for nt in (tab, exact))
    assert torch.equal(xt, xe)
    rt, re = (native.eloc(tu, td, nup, ndn, nt, z, 0.0, 1.0, RT, AT, 2.0, True) for nt in (tab, exact))
    for k in ("z", "dlogp", "grad", "lap", "eloc"):
        assert torch.allclose(rt[k], re[k], rtol=0.0, atol=0.0, equal_nan=True), k
    g = torch.Generator().manual_seed(4)
    a_z = torch.randn(B, n, d, generator=g, dtype=torch.float64).to(dev) / B
    a_d = torch.randn(B, generator=g, dtype=torch.float64).to(dev) / B
    (gxt, gpt), (gxe, gpe) = (native.cnf_adjoint(nt, z, a_z, a_d, 0.0, 1.0, RT, AT) for nt in (tab, exact))
    assert torch.equal(gxt, gxe) and torch.equal(gpt, gpe)
    # S includes the far walker B - 1: the oracle integrates it like any other.  Its local energy can be NaN on both sides (the flow
    # carries particles to |r| ~ 38, where the orbitals' exp(-r^2/2) underflows): compared where the oracle's is finite.
    xo, _ = O.cnf_generate(N(z[Si]), nets[2], rtol=ORT, atol=OAT)
    ref = O.eloc(N(z[Si]), nup, ndn, nets[2], 2.0, rtol=ORT, atol=OAT)
    gxo, _, _ = O.cnf_adjoint(N(z[Si]), np.zeros(len(S)), N(a_z[Si]), N(a_d[Si]), nets[2], rtol=ORT, atol=OAT)
    fin = np.isfinite(ref["eloc"])
    assert fin[:-1].all()
    e_x = float(np.abs(N(xt[Si]) - xo).max())
    e_far = float(np.abs(N(xt[B - 1]) - xo[-1]).max())
    e_el = float((np.abs(N(rt["eloc"][Si])[fin] - ref["eloc"][fin]) / np.abs(ref["eloc"][fin])).max())
    e_gx = _rel_max(N(gxt[Si]), gxo)
    print(f"GEOM off-table {nup}+{ndn} B={B} |S|={len(S)} {sorted(fams)}: x {e_x:.2e} (far walker {e_far:.2e}) eloc {e_el:.2e} "
          f"(far walker finite: {bool(fin[-1])}) gx {e_gx:.2e}")
    assert e_x < BAR_FLOW and e_el < BAR_OFF_ELOC and e_gx < BAR_GP


@pytest.mark.parametrize("B", [1, 2, 3, 255, 257, 65539, 131075])
def test_gsvmc_sweep_estimator_at_ragged_batches(dev, B):
    """GSVMC.forward -> backward at ragged batch sizes up to the benchmark's 65 536 + 3 and twice that: E and E_std equal the
    reference's estimator (src/VMC.py:57: mean and unbiased std of E_loc) evaluated in exact arithmetic on the GPU's own E_loc; at
    B = 1 E_std is NaN, as the reference's unbiased std of one value is.  At the benchmark's size E_loc on S matches the oracle."""
    import math
    import __graft_entry__ as Gm
    model = Gm._model(dev, 3, 3, 2.0)
    torch.manual_seed(B)
    model(B).backward()
    torch.cuda.synchronize()
    e = N(model.Eloc).astype(np.longdouble)
    assert e.shape == (B,) and np.isfinite(e).all()
    E = np.longdouble(math.fsum(N(model.Eloc))) / B
    assert abs(model.E - float(E)) <= 1e-12 * abs(float(E))
    if B == 1:
        assert math.isnan(model.E_std)
    else:
        std = float(np.sqrt(((e - E) ** 2).sum() / (B - 1)))
        assert abs(model.E_std - std) <= 1e-10 * std, (model.E_std, std)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    if B == 65539:
        fams = kernel_families("eloc", 6, 2, cu_count())
        fams.update(kernel_families("adjoint", 6, 2, cu_count()))
        assert_loops(fams, B)
        S = probe_set(B, fams, seed=1, nrand=16)
        v = model.cnf.v_wrapper.v
        net = O.Net(tuple(N(t) for t in (v.eta.fc1.weight, v.eta.fc1.bias, v.eta.fc2.weight)),
                    tuple(N(t) for t in (v.mu.fc1.weight, v.mu.fc1.bias, v.mu.fc2.weight)))
        ref = O.eloc(N(model.x[torch.as_tensor(S, device=dev)]), 3, 3, net, 2.0, rtol=ORT, atol=OAT)
        rel = np.abs(N(model.Eloc)[S] - ref["eloc"]) / np.abs(ref["eloc"])
        print(f"GEOM sweep B={B} |S|={len(S)}: E_loc vs oracle {rel.max():.2e}")
        assert rel.max() < 1e-5            # the production tolerances (1e-6 / 1e-8): the north-star bar of test_gpu_parity.py
