"""The ODE kernels on the device at time spans other than (0, 1) (tests/span_cases.py): SPANS = (0.25, 1.75), (1, 0),
(2, 0.5), (0.1, 0.7), with (0, 1) as the control.

  1. plain solves -- native.cnf_generate, cnf_delta_logp, eloc and cnf_adjoint at the smallest shapes that reach every kernel family
     of csrc/ff_plan.h, with the radial table and with radial = "exact", against the oracle called with the span itself and against
     the same call over (0, 1) with both fc2 weight vectors multiplied by b - a;
  2. a walker's x, cost class and walker_h_out bit-identical in the reversed batch, under an explicit order and in a sub-batch;
  3. opening steps: walker_h_init per walker and uniform, walker_h_equal, the clamp to the interval;
  4. the empty interval (0.5, 0.5);
  5. the autograd wrappers: d / dz and d / dtheta through CNF.generate, solve_ivp_nnmodule and CNF.delta_logp against the oracle's
     adjoint and against autograd through a fixed-step RK4 of the plainly restated field (span_cases.rk4_reference);
  6. the production sweeps: GSVMC (3 + 3, and 1 + 1 in three dimensions) and BetaVMC, two sweeps each with the warm start and the
     adaptive first steps on, against the oracle on the same base walkers and against a second model over (0, 1) with scaled fc2.

Worst errors measured on an MI355X: docs/LOG.md (the SPANS MAX line this file prints)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import span_cases as cases
from tests.common import N, T, cu_count, make_mlp
from tests.span_cases import AT, BAR_ELOC, BAR_FLOW, BAR_GP, ORT, OAT, RT, rel_max, sid

pytestmark = pytest.mark.gpu

SPAN_IDS = [sid(s) for s in cases.ALL_SPANS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


def flow_over(golden, dev, span, s=1.0, use_mu=True):
    import fermiflow_amd as ff
    eta, mu = cases.weights(golden, s, use_mu)
    cnf = ff.CNF(ff.Backflow(make_mlp(eta, dev), mu=make_mlp(mu, dev) if mu is not None else None), tuple(span))
    cnf.rtol, cnf.atol = RT, AT
    return cnf


@pytest.fixture(scope="module")
def K(golden, dev):
    from fermiflow_amd import native
    nets = {}

    def warm_args(h_init=None, h_scale=1.0, uniform=False, equal=False, max_steps=0):
        if h_init is None:
            return dict(max_steps=max_steps)
        return dict(walker_h_init=T(h_init, dev), walker_h_scale=h_scale, walker_h_uniform=uniform, walker_h_equal=equal, max_steps=max_steps)

    @contextlib.contextmanager
    def sens64():
        prev = native.set_sens_precision(64)
        try:
            yield
        finally:
            native.set_sens_precision(prev)

    class Dev:
        gp_reproducible = True

        @staticmethod
        def plan(call, n, d):
            fam, g, _ = native.kernel_plan(call, n, d, cu_count())
            return fam, g

        @staticmethod
        def net(s, table):
            if (s, table) not in nets:
                cnf = flow_over(golden, dev, (0.0, 1.0), s)
                nets[s, table] = (cnf, cnf.v_wrapper.v.net(radial="table" if table else "exact"))
            return nets[s, table]

        @staticmethod
        def generate(h, z, t0, t1, order=None, **warm):
            B = len(z)
            cost = torch.full((B,), -1, dtype=torch.int32, device=dev)
            hout = torch.zeros(B, dtype=torch.float64, device=dev)
            x, st = native.cnf_generate(h[1], T(z, dev), t0, t1, RT, AT, want_stats=True, walker_cost=cost,
                                        walker_order=None if order is None else T(order, dev, torch.int32), walker_h_out=hout, **warm_args(**warm))
            return N(x), N(cost), N(hout), N(st)

        @staticmethod
        def delta_logp(h, x, t0, t1):
            z, dl, st = native.cnf_delta_logp(h[1], T(x, dev), t0, t1, RT, AT, want_stats=True)
            return N(z), N(dl), N(st)

        @staticmethod
        def eloc(h, x, nup, ndn, Z, t0, t1, **warm):
            tu = native.orbital_table(list(range(nup)), dev) if nup else None
            td = native.orbital_table(list(range(ndn)), dev) if ndn else None
            hout = torch.zeros(len(x), dtype=torch.float64, device=dev)
            with sens64():
                r = native.eloc(tu, td, nup, ndn, h[1], T(x, dev), t0, t1, RT, AT, Z, True, want_stats=True, walker_h_out=hout, **warm_args(**warm))
                torch.cuda.synchronize()
            out = {k: N(v).copy() for k, v in r.items()}
            out["hout"] = N(hout)
            return out

        @staticmethod
        def adjoint(h, y, a_z, a_d, t0, t1, **warm):
            gx, gp, st = native.cnf_adjoint(h[1], T(y, dev), T(a_z, dev), T(a_d, dev), t0, t1, RT, AT, need_gx=True, want_stats=True,
                                            **warm_args(**warm))
            return N(gx), N(gp), N(st)
    yield Dev
    cases.report("MI355X")


# ---- 1. plain solves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["table", "exact"])
@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("n,d", cases.FLOW_SHAPES)
def test_flow_and_delta_logp_vs_oracle_and_identity(K, golden, n, d, span, table):
    cases.flow_case(K, golden, n, d, table, span)


@pytest.mark.parametrize("table", [True, False], ids=["table", "exact"])
@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("nup,ndn,d", cases.ELOC_SHAPES)
def test_local_energy_vs_oracle_and_identity(K, golden, nup, ndn, d, span, table):
    cases.eloc_case(K, golden, nup, ndn, d, table, span)


@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("n,d,table", cases.ADJ_SHAPES)
def test_adjoint_vs_oracle_and_identity(K, golden, n, d, table, span):
    cases.adjoint_case(K, golden, n, d, table, span)


def test_kernel_families_reached(K):
    """the shapes are the smallest that reach each kernel family of csrc/ff_plan.h"""
    assert [K.plan("flow", n, d) for n, d in cases.FLOW_SHAPES] == [("narrow", 10), ("narrow", 5), ("narrow", 10), ("wide", 1), ("wide", 1)]
    assert [K.plan("eloc", a + b, d)[0] for a, b, d in cases.ELOC_SHAPES] == ["columns", "mfma", "rows", "split", "rows", "wide"]
    assert [K.plan("adjoint" if t else "adj_fb", n, d)[0] for n, d, t in cases.ADJ_SHAPES] == ["tabulated", "direct", "tabulated", "wide"]


# ---- 2. batch and order independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", cases.SLOT_SPANS, ids=[sid(s) for s in cases.SLOT_SPANS])
@pytest.mark.parametrize("n,d", cases.NARROW_FLOW)
def test_walker_is_the_same_in_every_batch_slot_and_order(K, golden, n, d, span):
    cases.slots_case(K, golden, n, d, span)


# ---- 3. opening steps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("n,d", cases.NARROW_FLOW)
def test_flow_opens_with_the_given_step(K, golden, n, d, span):
    cases.open_flow_case(K, golden, n, d, span)


@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("nup,ndn", [(3, 3), (2, 1)], ids=["mfma", "columns"])
def test_local_energy_opens_with_the_given_step(K, golden, nup, ndn, span):
    cases.open_eloc_case(K, golden, nup, ndn, span)


@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
def test_equal_steps_of_the_interval(K, golden, span):
    cases.equal_case(K, golden, span)


@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
def test_opening_step_is_clamped_to_the_interval(K, golden, span):
    cases.clamp_case(K, golden, span)


# ---- 4. the empty interval ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [True, False], ids=["table", "exact"])
@pytest.mark.parametrize("n,d", cases.FLOW_SHAPES)
def test_empty_interval_flow_and_adjoint(K, golden, n, d, table):
    cases.empty_flow_case(K, golden, n, d, table)


@pytest.mark.parametrize("table", [True, False], ids=["table", "exact"])
@pytest.mark.parametrize("nup,ndn,d,E", cases.EMPTY_ELOC)
def test_empty_interval_local_energy(K, golden, nup, ndn, d, E, table):
    cases.empty_eloc_case(K, golden, nup, ndn, d, E, table)


# ---- 5. the autograd wrappers ------------------------------------------------------------------------------------------------------
def _param_grads(cnf):
    return np.concatenate([N(p.grad).reshape(-1) for p in cnf.v_wrapper.v.parameters()])


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("n,d", cases.AUTOGRAD_SHAPES)
def test_autograd_through_generate(golden, dev, n, d, span, use_mu):
    """_Generate.backward (fermiflow_amd/NeuralODE/nnModule.py): the adjoint kernel integrating from b back to a with a zero a_d seed,
    and _split mapping the flat gradient onto Backflow.parameters() (three tensors with mu = None).  d / dz through CNF.generate and
    d / dtheta through solve_ivp_nnmodule(cnf.v_wrapper, (a, b), z) against the oracle's adjoint on the device's x, against autograd
    through RK4 of the plain field (128 steps: agrees with the oracle within 3.6e-11, span_cases.rk4_reference), and against the
    model over (0, 1) with scaled fc2."""
    from fermiflow_amd.NeuralODE.nnModule import solve_ivp_nnmodule
    a, b = span
    z, c, _, _ = cases.autograd_inputs(n, d)
    B = len(z)
    cnf = flow_over(golden, dev, span, 1.0, use_mu)
    zt = T(z, dev).requires_grad_()
    x = cnf.generate(zt)
    (T(c, dev) * x).sum().backward()
    assert all(p.grad is None for p in cnf.parameters())            # (CNF.generate differentiates with respect to z alone)
    zs = T(z, dev).requires_grad_()
    xs = solve_ivp_nnmodule(cnf.v_wrapper, (a, b), zs, rtol=RT, atol=AT)
    assert torch.equal(xs, x)
    (T(c, dev) * xs).sum().backward()
    assert torch.equal(zs.grad, zt.grad)
    gz, gp = N(zt.grad), _param_grads(cnf)
    assert [tuple(p.grad.shape) for p in cnf.v_wrapper.v.parameters()] == [(50, 1), (50,), (1, 50)] * (2 if use_mu else 1)
    gzo, gpo = cases.ref_adjoint(golden, N(x), c, np.zeros(B), (b, a), use_mu)
    xr, gzr, gpr = cases.rk4_reference(golden, use_mu, span, z=z, c=c)
    unit = flow_over(golden, dev, (0.0, 1.0), b - a, use_mu)
    z1 = T(z, dev).requires_grad_()
    (T(c, dev) * solve_ivp_nnmodule(unit.v_wrapper, (0.0, 1.0), z1, rtol=RT, atol=AT)).sum().backward()
    e = dict(oracle_gz=rel_max(gz, gzo), oracle_gp=rel_max(gp, gpo), rk4_x=float(np.abs(N(x) - xr).max()), rk4_gz=rel_max(gz, gzr),
             rk4_gp=rel_max(gp, gpr), identity_gz=rel_max(gz, N(z1.grad)), identity_gp=rel_max(gp, cases.scale_gp(_param_grads(unit), b - a)))
    print(f"SPANS autograd generate {n}x{d} mu={use_mu} {sid(span)}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    cases.note(**{"generate_" + k: v for k, v in e.items()})
    assert e.pop("rk4_x") < BAR_FLOW
    assert all(v < BAR_GP for v in e.values()), e


@pytest.mark.parametrize("use_mu", [True, False], ids=["mu", "nomu"])
@pytest.mark.parametrize("span", cases.ALL_SPANS, ids=SPAN_IDS)
@pytest.mark.parametrize("n,d", cases.AUTOGRAD_SHAPES)
def test_autograd_through_delta_logp(golden, dev, n, d, span, use_mu):
    """CNF.delta_logp(x, params_require_grad=True) over the span with the loss of test_cnf_generate_logp_adjoint, sum(cz z) + sum(cd Delta):
    z, Delta, d / dx and d / dtheta against the oracle (its adjoint from a to b on the device's z), the RK4 reference and the identity."""
    a, b = span
    xin, _, cz, cd = cases.autograd_inputs(n, d)
    cnf = flow_over(golden, dev, span, 1.0, use_mu)
    xg = T(xin, dev).requires_grad_()
    z, dl = cnf.delta_logp(xg, params_require_grad=True)
    loss = (T(cz, dev) * z).sum() + (T(cd, dev) * dl).sum()
    grads = torch.autograd.grad(loss, [xg] + list(cnf.v_wrapper.v.parameters()))
    gx, gp = N(grads[0]), np.concatenate([N(g).reshape(-1) for g in grads[1:]])
    zo, dlo = cases.ref_delta_logp(golden, xin, span) if use_mu else O.cnf_delta_logp(xin, cases.onet(golden, 1.0, False), a, b, ORT, OAT)[:2]
    gxo, gpo = cases.ref_adjoint(golden, N(z), cz, cd, (a, b), use_mu)
    zr, dlr, gxr, gpr = cases.rk4_reference(golden, use_mu, span, x=xin, cz=cz, cd=cd)
    unit = flow_over(golden, dev, (0.0, 1.0), b - a, use_mu)
    x1 = T(xin, dev).requires_grad_()
    z1, dl1 = unit.delta_logp(x1, params_require_grad=True)
    g1 = torch.autograd.grad((T(cz, dev) * z1).sum() + (T(cd, dev) * dl1).sum(), [x1] + list(unit.v_wrapper.v.parameters()))
    gp1 = cases.scale_gp(np.concatenate([N(g).reshape(-1) for g in g1[1:]]), b - a)
    flow = dict(oracle_z=float(np.abs(N(z) - zo).max()), oracle_dlogp=float(np.abs(N(dl) - dlo).max()), rk4_z=float(np.abs(N(z) - zr).max()),
                rk4_dlogp=float(np.abs(N(dl) - dlr).max()), identity_z=float(np.abs(N(z) - N(z1)).max()), identity_dlogp=float(np.abs(N(dl) - N(dl1)).max()))
    e = dict(oracle_gx=rel_max(gx, gxo), oracle_gp=rel_max(gp, gpo), rk4_gx=rel_max(gx, gxr), rk4_gp=rel_max(gp, gpr),
             identity_gx=rel_max(gx, N(g1[0])), identity_gp=rel_max(gp, gp1))
    print(f"SPANS autograd delta_logp {n}x{d} mu={use_mu} {sid(span)}: " + " ".join(f"{k} {v:.2e}" for k, v in {**flow, **e}.items()))
    cases.note(**{"delta_logp_" + k: v for k, v in {**flow, **e}.items()})
    assert all(v < BAR_FLOW for v in flow.values()), flow
    assert all(v < BAR_GP for v in e.values()), e


# ---- 6. the production sweeps ------------------------------------------------------------------------------------------------------
SWEEP_B = 257


def _gsvmc(golden, dev, nup, ndn, dim, span, s, Zc, rt, at):
    import fermiflow_amd as ff
    cnf = flow_over(golden, dev, span, s)
    cnf.rtol, cnf.atol = rt, at
    model = ff.GSVMC(nup, ndn, ff.HO2D() if dim == 2 else ff.HO3D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(Zc), sp_potential=ff.HO())
    model.to(dev)
    assert model.warm_start and model.adaptive_h        # production settings
    return model


def _two_sweeps(model, z):
    """forward_from then backward, twice: the second sweep opens from the first one's steps and runs walker_schedule with the interval"""
    out = []
    for _ in range(2):
        g = model.forward_from(z)
        model.zero_grad()
        g.backward()
        torch.cuda.synchronize()
        out.append(dict(x=N(model.x), eloc=N(model.Eloc), E=model.E, E_std=model.E_std,
                        gp=np.concatenate([N(p.grad).reshape(-1) for p in model.cnf.v_wrapper.v.parameters()])))
    return out


def _std_bar(eloc):
    # the unbiased standard deviation moves by at most sqrt(B / (B - 1)) rms(delta) <= that times max|delta| under a perturbation delta
    return BAR_ELOC * float(np.abs(eloc).max()) * float(np.sqrt(len(eloc) / (len(eloc) - 1.0)))


def _sweep_errors(sw, ref):
    return dict(x=float(np.abs(sw["x"] - ref["x"]).max()), eloc=float(np.abs(sw["eloc"] / ref["eloc"] - 1.0).max()), E=abs(sw["E"] / ref["E"] - 1.0),
                E_std=abs(sw["E_std"] - ref["E_std"]), gp=rel_max(sw["gp"], ref["gp"]))


def _gsvmc_case(golden, dev, nup, ndn, dim, span, Zc=2.0, tight=1.0):
    """Both sweeps against the model over (0, 1) with scaled fc2 and against each other; the second one -- opened from the first one's
    steps, its local-energy pass scheduled by ff_walker_schedule with the interval -- against the oracle on the same base walkers.
    tight: a factor on the four tolerances of the solves (the bars stay).  The oracle controls its step by the error norm of the whole
    batch, so among 257 walkers the ones next to a node of the determinant (|E_loc| in the thousands) carry more than their share: the
    case asserts, on the oracle alone, that its E_loc at the device's tolerances is within half of the bar of its E_loc at its own."""
    a, b = span
    n, B = nup + ndn, SWEEP_B
    rt, at, ort, oat = (tight * t for t in (RT, AT, ORT, OAT))
    z = cases.walkers(n, dim, B)
    net = cases.onet(golden)
    oe, ol = (O.eloc, O.logprob) if dim == 2 else (O.eloc3d, O.logprob3d)
    xo, _ = O.cnf_generate(z, net, a, b, ort, oat)
    eo = oe(xo, nup, ndn, net, Zc, t0=a, t1=b, rtol=ort, atol=oat)["eloc"]
    own = float(np.abs(oe(xo, nup, ndn, net, Zc, t0=a, t1=b, rtol=rt, atol=at)["eloc"] / eo - 1.0).max())
    assert own < BAR_ELOC / 2, ("the oracle's own truncation error beyond half of the bar: tighten this case's solve", span, own)
    sweeps = _two_sweeps(_gsvmc(golden, dev, nup, ndn, dim, span, 1.0, Zc, rt, at), T(z, dev))
    units = _two_sweeps(_gsvmc(golden, dev, nup, ndn, dim, (0.0, 1.0), b - a, Zc, rt, at), T(z, dev))
    for u in units:
        u["gp"] = cases.scale_gp(u["gp"], b - a)
    sw = sweeps[1]
    ref = dict(x=xo, eloc=oe(sw["x"], nup, ndn, net, Zc, t0=a, t1=b, rtol=ort, atol=oat)["eloc"])
    ref["E"], ref["E_std"] = float(ref["eloc"].mean()), float(ref["eloc"].std(ddof=1))
    w = (sw["eloc"] - sw["eloc"].mean()) / B
    zo, dlo, _ = O.cnf_delta_logp(sw["x"], net, a, b, ort, oat)
    ref["gp"] = O.cnf_adjoint(zo, dlo, w[:, None, None] * ol(zo, nup, ndn)[1], -w, net, a, b, ort, oat)[1]
    figs = {"oracle_2": _sweep_errors(sw, ref), "identity_1": _sweep_errors(sweeps[0], units[0]), "identity_2": _sweep_errors(sw, units[1]),
            "sweep_1_vs_2": _sweep_errors(sweeps[0], sw)}
    print(f"SPANS GSVMC {nup}+{ndn} {dim}d {sid(span)} tolerances x {tight:g}: E {sw['E']:.9f} +- {sw['E_std']:.6f} (oracle's own {own:.2e}); " +
          "; ".join(name + " " + " ".join(f"{q} {v:.2e}" for q, v in f.items()) for name, f in figs.items()))
    cases.note(**{"sweep_" + q: v for q, v in figs["oracle_2"].items()},
               **{"identity_sweep_" + q: max(figs["identity_1"][q], figs["identity_2"][q]) for q in figs["identity_1"]})
    for name, f in figs.items():
        assert f["x"] < BAR_FLOW and f["eloc"] < BAR_ELOC and f["E"] < BAR_ELOC and f["E_std"] < _std_bar(ref["eloc"]) and f["gp"] < BAR_GP, (name, f)


@pytest.mark.parametrize("span", cases.SPANS, ids=SPAN_IDS[:4])
def test_gsvmc_sweeps_over_the_span(golden, dev, span):
    """GSVMC at 3 + 3, Z = 2, 257 walkers, the production settings (warm start, adaptive first steps, heavy-walker routing): model.x,
    per-walker E_loc, E, E_std and every parameter's .grad (_gsvmc_case; the seeds (E_loc - mean) / B of the oracle's adjoint are formed
    from the device's E_loc, as test_config4_six_plus_six forms them).  The solves are ten times tighter than 1e-9 / 1e-11 and
    1e-10 / 1e-12: at those the oracle's own truncation error in E_loc of these 257 walkers, measured on the CPU, is 1.5e-8, 4.3e-8,
    6.2e-8 and 7.4e-9 over the four spans -- beyond half of BAR_ELOC at three of them; at a tenth it is 1.5e-9, 4.5e-9, 6.6e-9, 8.6e-10."""
    _gsvmc_case(golden, dev, 3, 3, 2, span, tight=0.1)


def test_gsvmc_sweeps_in_three_dimensions_reversed(golden, dev):
    """1 + 1 particles in three dimensions (HO3D, the 3-D row layout) over (1, 0); the oracle's own truncation error there is 1.1e-11"""
    _gsvmc_case(golden, dev, 1, 1, 3, (1.0, 0.0))


@pytest.mark.parametrize("span", cases.SLOT_SPANS, ids=[sid(s) for s in cases.SLOT_SPANS])
def test_betavmc_sweeps_over_the_span(golden, dev, span):
    """BetaVMC(beta = 2, 3 + 0 particles) with three many-body states inside the first wave: x and per-walker E_loc of both sweeps
    against the oracle with every walker's own orbital set; E, F, S, the logit gradient and the flow gradients against the model over
    (0, 1) with scaled fc2 -- that unit-span path is pinned to the reference's goldens by tests/test_gpu_parity.py."""
    import fermiflow_amd as ff
    a, b = span
    B, Zc, beta = SWEEP_B, 2.0, 2.0
    z = cases.walkers(3, 2, B)
    ws = np.repeat([0, 1, 2, 3, 5], [3, 3, 100, 100, B - 206]).astype(np.int32)
    net = cases.onet(golden)
    runs = []
    for sp, s in ((span, 1.0), ((0.0, 1.0), b - a)):
        model = ff.BetaVMC(beta, 3, 0, 2.0, True, ff.HO2D(), ff.FreeFermion(device=dev), flow_over(golden, dev, sp, s), ff.CoulombPairPotential(Zc),
                           sp_potential=ff.HO())
        model.to(dev)
        assert model.warm_start and model.adaptive_h and model.Nstates > 5
        up = np.array([[o.k for o in st[0]] for st in model.states], dtype=np.int32)
        out = []
        for _ in range(2):
            gphi, gtheta = model.forward_from(T(z, dev), ws)
            model.zero_grad()
            (gphi + gtheta).backward()
            torch.cuda.synchronize()
            out.append(dict(x=N(model.x), eloc=N(model.Eloc), E=model.E, F=model.F, S=model.S, glogits=N(model.log_state_weights.grad),
                            gp=np.concatenate([N(p.grad).reshape(-1) for p in model.cnf.v_wrapper.v.parameters()])))
        runs.append(out)
    xo, _ = O.cnf_generate(z, net, a, b, ORT, OAT)
    for k, (sw, un) in enumerate(zip(*runs)):
        ref = O.eloc(sw["x"], 3, 0, net, Zc, t0=a, t1=b, rtol=ORT, atol=OAT, tab_up=up, wstate=ws)["eloc"]
        emax = float(np.abs(ref).max())
        e = dict(x=float(np.abs(sw["x"] - xo).max()), eloc=float(np.abs(sw["eloc"] / ref - 1.0).max()))
        i = dict(x=float(np.abs(sw["x"] - un["x"]).max()), eloc=float(np.abs(sw["eloc"] / un["eloc"] - 1.0).max()), E=abs(sw["E"] - un["E"]),
                 F=abs(sw["F"] - un["F"]), S=abs(sw["S"] - un["S"]), glogits=rel_max(sw["glogits"], un["glogits"]),
                 gp=rel_max(sw["gp"], cases.scale_gp(un["gp"], b - a)))
        print(f"SPANS BetaVMC {sid(span)} sweep {k + 1}: E {sw['E']:.9f} F {sw['F']:.9f} S {sw['S']:.9f}; oracle " +
              " ".join(f"{q} {v:.2e}" for q, v in e.items()) + "; identity " + " ".join(f"{q} {v:.2e}" for q, v in i.items()))
        cases.note(**{"beta_" + q: v for q, v in e.items()}, **{"identity_beta_" + q: v for q, v in i.items()})
        assert e["x"] < BAR_FLOW and e["eloc"] < BAR_ELOC, e
        assert i["x"] < BAR_FLOW and i["eloc"] < BAR_ELOC, i
        # E and F are means of per-walker quantities that agree within BAR_ELOC of the largest |E_loc|; S = beta (E - F)
        assert i["E"] < BAR_ELOC * emax and i["F"] < BAR_ELOC * emax and i["S"] < 2.0 * beta * BAR_ELOC * emax, (i, emax)
        assert i["glogits"] < BAR_GP and i["gp"] < BAR_GP, i
