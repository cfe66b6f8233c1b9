"""Stochastic reconfiguration for BetaVMC on the device: ff_sr_state_moments / ff_sr_state_finish through fermiflow_amd.native, the
BetaVMC.sr hook and a short --optimizer sr training of the finite-temperature driver."""
import numpy as np
import pytest
import torch

from tests import sr_beta_ref as RB
from tests import sr_ref as R
from tests.common import N, T, make_flow, net_arrays
from tests.test_gpu_sr import _theta_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", RB.IDS)
def test_state_moments(dev, name):
    """the assertions of tests/test_sr_beta_hostsim.py::test_state_moments, on the device"""
    from fermiflow_amd import native
    B, P, counts = RB.CASES[name]
    ns = len(counts)
    O, e, ws, me = RB.state_data(name)
    met = T(me, dev)
    call = lambda o, ee, w: native.sr_state_moments(T(o, dev).reshape(-1, P), T(ee, dev), torch.as_tensor(w, dtype=torch.int32, device=dev), met, ns)
    sums_t = call(O, e, ws)
    sums = N(sums_t)
    assert sums.shape == (RB.sums_len(P, ns),) and np.isfinite(sums).all()
    ref = RB.raw_ref(O, e, ws, me)
    RB.check_raw_sums(sums, ref)
    assert torch.equal(call(O, e, ws), sums_t)
    f, ob, g = (N(t) for t in native.sr_state_finish(sums_t, P, ns))
    if B == 0:
        assert (sums == 0.0).all()
        assert np.isnan(f).all() and np.isnan(g).all() and (ob == 0.0).all()
        return
    fr = RB.finished_ref(ref)
    RB.check_finished(f, ob, g, fr)
    for a, b in zip(native.sr_state_finish(sums_t, P, ns), (f, ob, g)):
        assert np.array_equal(N(a), b)
    if name == "d":
        print(f"FIGURES d: max|fisher| {np.abs(f).max():.3e}, largest bound {float(fr['bF'].max()):.3e}")
    if name == "c":
        for cut in (1000, R.SR_CHUNK):
            both = call(O[:cut], e[:cut], ws[:cut]) + call(O[cut:], e[cut:], ws[cut:])
            assert (RB.split_sums(N(both), P, ns)[3] == np.asarray(counts)).all()
            RB.check_finished(*(N(t) for t in native.sr_state_finish(both, P, ns)), fr, scale=2.0)
        lam = np.linalg.eigvalsh(f).min()
        bar = -float(fr["bF"].max()) * P
        print(f"FIGURES c: smallest eigenvalue {lam:.3e}, bar {bar:.3e}; fisher error / bound {float((np.abs(f - fr['F']) / fr['bF']).max()):.3f}")
        assert lam >= bar


@pytest.mark.parametrize("tag", ["boltz", "hot"])
def test_sweep_hook_end_to_end(golden, dev, tag):
    import fermiflow_amd as ff
    G = golden["g6_betavmc"]
    eta, mu = net_arrays(G, "")
    ws = np.repeat(G[tag + "_keys"], G[tag + "_counts"])
    z = T(G[tag + "_z"], dev)

    def model_of():
        cnf = make_flow(eta, mu, dev)
        cnf.rtol, cnf.atol = 1e-10, 1e-12
        model = ff.BetaVMC(float(G[tag + "_beta"]), 3, 0, float(G[tag + "_dE"]), True, ff.HO2D(), ff.FreeFermion(device=dev), cnf,
                           ff.CoulombPairPotential(2.0), sp_potential=ff.HO())
        model.to(dev)
        with torch.no_grad():
            model.log_state_weights.copy_(T(G[tag + "_logits"], dev))
        return model

    def sweep(model):
        gphi, gtheta = model.forward_from(z, ws)
        model.zero_grad()
        gphi.backward()
        gtheta.backward()
        return (gphi.detach().clone(), gtheta.detach().clone(), torch.tensor([model.E, model.F, model.S], dtype=torch.float64),
                model.log_state_weights.grad.clone(), torch.cat([p.grad.reshape(-1) for p in model.cnf.parameters()]))
    model = model_of()
    opt = model.sr = ff.BetaSR(model)
    with_sr = sweep(model)
    flat = opt.flat_grad()
    B, P, Ns = z.shape[0], flat.numel(), model.Nstates
    assert opt.scores.shape == (B, P) and opt.fisher.shape == (P, P) and opt.obar_state.shape == (Ns, P)
    assert opt.grad.shape == (P,) and opt.fisher_phi.shape == (Ns, Ns)
    for t in (opt.scores, opt.fisher, opt.obar_state, opt.grad, opt.fisher_phi):
        assert t.is_cuda and torch.isfinite(t).all()
    assert torch.equal(opt.fisher, opt.fisher.T)
    err = (opt.grad - flat).abs().max().item()
    print(f"FIGURES {tag}: sr.grad against the sweep's gradient: {err:.3e} of {flat.abs().max().item():.3e}")
    assert err < _theta_bar() * flat.abs().max().item()
    # fisher: the same expression in torch fp64 from the scores and the state list, within the propagated bound
    wst = torch.as_tensor(ws, dtype=torch.int64, device=dev)
    cnt = torch.bincount(wst, minlength=Ns).to(torch.float64)
    onehot = torch.nn.functional.one_hot(wst, Ns).to(torch.float64)
    o_state = onehot.T @ opt.scores
    gram = (o_state / cnt.clamp(min=1.0)[:, None]).T @ o_state
    F_t = (opt.scores.T @ opt.scores - gram) / B
    fr = RB.finished_ref(RB.raw_ref(N(opt.scores), N(model.Eloc), ws.astype(np.int32), np.zeros(Ns)))
    dF = np.abs(N(opt.fisher) - N(F_t))
    print(f"FIGURES {tag}: fisher against torch: error / bound {float((dF / fr['bF']).max()):.3f}")
    assert (dF <= fr["bF"]).all()
    # the in-sample cross block vanishes: O is centred per state
    cross = (onehot - cnt / B).T @ (opt.scores - opt.obar_state[wst])
    cbar = B * R.EPS * opt.scores.abs().max().item() * P
    print(f"FIGURES {tag}: cross block {cross.abs().max().item():.3e}, bar {cbar:.3e}")
    assert cross.abs().max().item() <= cbar
    mu_s = torch.exp(model.logp_states_all.to(dev))
    assert (opt.fisher_phi - (torch.diag(mu_s) - torch.outer(mu_s, mu_s))).abs().max().item() <= 1e-12
    F, g, Fp, gp = N(opt.fisher), N(flat), N(opt.fisher_phi), N(model.log_state_weights.grad)
    opt.step()
    for A, d, rhs in ((F + opt.shift * np.eye(P), N(opt.delta), g), (Fp + opt.shift_phi * np.eye(Ns), N(opt.delta_phi), gp)):
        assert np.isfinite(d).all()
        assert np.linalg.norm(A @ d - rhs) <= R.sr_residual_bound(A, d)
    # the hook changes nothing it does not own: a model that never had sr set gives the same bits
    for a, b in zip(with_sr, sweep(model_of())):
        assert torch.equal(a, b)


def test_training_smoke(dev):
    """3 + 0 particles, beta = 2, Z = 0.5, deltaE = 2, random logits, B = 4096, seeded, 20 iterations of --optimizer sr at the defaults:
    F of the last iteration below F of the first by more than 3 sqrt(se_first^2 + se_last^2), se = F_std / sqrt(B)."""
    import fermiflow_amd as ff
    from fermiflow_amd import BetaFermionHO2D as drv
    args = drv.build_parser().parse_args(["--nup", "3", "--ndown", "0", "--beta", "2.0", "--Z", "0.5", "--deltaE", "2.0", "--batch", "4096",
                                          "--optimizer", "sr"])
    torch.manual_seed(42)
    eta, mu = ff.MLP(1, args.Deta), ff.MLP(1, args.Dmu)
    eta.init_zeros(); mu.init_zeros()
    cnf = ff.CNF(ff.Backflow(eta, mu=mu), (args.t0, args.t1))
    model = ff.BetaVMC(args.beta, args.nup, args.ndown, args.deltaE, args.boltzmann, ff.HO2D(), ff.FreeFermion(device=dev), cnf,
                       ff.CoulombPairPotential(args.Z), sp_potential=ff.HO())
    model.to(device=dev)
    opt = drv.make_optimizer(args, model)
    assert (opt.lr, opt.shift, opt.lr_phi, opt.shift_phi) == (0.05, 1e-3, 0.05, 1e-3)
    hist = []
    for _ in range(20):
        gphi, gtheta = model(args.batch)
        opt.zero_grad()
        gphi.backward()
        gtheta.backward()
        opt.step()
        hist.append((model.F, model.F_std / np.sqrt(args.batch)))
    print("F:", " ".join(f"{f:.4f}" for f, _ in hist))
    (f0, s0), (f1, s1) = hist[0], hist[-1]
    margin = (f0 - f1) / np.sqrt(s0 * s0 + s1 * s1)
    print(f"FIGURES drop {f0 - f1:.4f} = {margin:.1f} combined standard errors")
    assert np.isfinite(f1) and margin > 3.0, (f0, f1, margin)
