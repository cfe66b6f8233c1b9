"""Stochastic reconfiguration on the device: ff_cnf_adjoint_scores, ff_sr_moments / ff_sr_finish through fermiflow_amd.native, the
GSVMC.sr hook and a short --optimizer sr training."""
import inspect
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import sr_ref as R
from tests.common import N, T, make_flow, net_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


def _flow_end(dev, cnf, n, d, B, tol):
    from fermiflow_amd import native
    import fermiflow_amd as ff
    nup, ndn = R.spins(n)
    orb = (ff.HO2D() if d == 2 else ff.HO3D()).orbitals
    from fermiflow_amd.orbitals import orbital_indices
    tu = native.orbital_table(orbital_indices(orb[:nup]), dev)
    td = native.orbital_table(orbital_indices(orb[:ndn]), dev)
    net = cnf.v_wrapper.v.net(radial="exact")
    r = native.eloc(tu, td, nup, ndn, net, T(R.walkers(n, d, B), dev), R.T0, R.T1, tol["rtol"], tol["atol"], R.Z, True)
    return net, r


def test_scores_against_oracle(golden, dev):
    """scores at rtol 1e-10 / atol 1e-12 against oracle.cnf_adjoint walker by walker, each row relative to its largest |entry|; bar:
    4 x the same error of the existing direct ff_cnf_adjoint (B = 1 calls, no radial table), measured here on the device first."""
    from fermiflow_amd import native
    yard = worst = 0.0
    for use_mu in (True, False):
        eta, mu = net_arrays(golden["g3_backflow"], "c1_", use_mu)
        cnf = make_flow(eta, mu, dev)
        onet = O.Net(eta, mu)
        for n, d, B in R.SHAPES:
            net, r = _flow_end(dev, cnf, n, d, B, R.TIGHT)
            z, g0, dl = r["z"], r["glogp0"], N(r["dlogp"])
            sc, st = native.cnf_adjoint_scores(net, z, g0, R.T0, R.T1, R.TIGHT["rtol"], R.TIGHT["atol"], want_stats=True)
            assert int(st[3]) == 0
            sc, zn, gn = N(sc), N(z), N(g0)
            ad = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
            for b in range(B):
                _, ref, _ = O.cnf_adjoint(zn[b:b + 1], dl[b:b + 1], gn[b:b + 1], np.array([-1.0]), onet, t0=R.T0, t1=R.T1, **R.TIGHT)
                _, gp = native.cnf_adjoint(net, z[b:b + 1], g0[b:b + 1], ad, R.T0, R.T1, R.TIGHT["rtol"], R.TIGHT["atol"], need_gx=False)
                yard = max(yard, R.row_rel_err(N(gp), ref))
                worst = max(worst, R.row_rel_err(sc[b], ref))
    print(f"existing direct adjoint against the oracle: {yard:.3e}; scores: {worst:.3e}; bar {4 * yard:.3e}")
    assert yard > 0.0
    assert worst <= 4 * yard, (worst, yard)


@pytest.mark.parametrize("B,P", R.MOMENT_CASES, ids=[f"B{B}_P{P}" for B, P in R.MOMENT_CASES])
def test_moments(dev, B, P):
    from fermiflow_amd import native
    Om, e, em = R.moment_data(B, P)
    emt = torch.full((1,), em, dtype=torch.float64, device=dev)
    call = lambda o, ee: native.sr_moments(T(o, dev).reshape(-1, P), T(ee, dev), emt)
    sums_t = call(Om, e)
    sums = N(sums_t)
    assert np.isfinite(sums).all()
    if B == 0:
        assert (sums == 0.0).all()
        return
    ref = R.moment_ref(Om, e, em)
    R.check_raw_sums(sums, ref, P)
    fr = R.finished_ref(ref)
    R.check_finished(*(N(t) for t in native.sr_finish(sums_t, P)), fr)
    assert torch.equal(call(Om, e), sums_t)
    if B > R.SR_CHUNK:
        both = call(Om[:R.SR_CHUNK], e[:R.SR_CHUNK]) + call(Om[R.SR_CHUNK:], e[R.SR_CHUNK:])
        R.check_finished(*(N(t) for t in native.sr_finish(both, P)), fr, scale=2.0)


def _theta_bar():
    """the theta-gradient bar of table against direct evaluation, read from the test that owns it"""
    from tests import test_gpu_parity as Pm
    src = inspect.getsource(Pm.test_radial_table_equals_direct_evaluation_and_is_deterministic)
    m = re.search(r"\(gpt - gpe\)\.abs\(\)\.max\(\)\.item\(\) < ([0-9.eE+-]+) \* gpe\.abs\(\)\.max\(\)", src)
    return float(m.group(1))


def test_sweep_hook_end_to_end(golden, dev):
    import fermiflow_amd as ff
    G = golden["g5_gsvmc"]
    name = "z2_nt"
    nup, ndn, B, _ = (int(v) for v in G[name + "_cfg"])
    assert (nup, ndn) == (3, 3)
    eta, mu = net_arrays(G, name + "_", True)

    def model_of():
        cnf = make_flow(eta, mu, dev)
        cnf.rtol, cnf.atol = 1e-10, 1e-14
        return ff.GSVMC(nup, ndn, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(float(G[name + "_Z"])), sp_potential=ff.HO())
    z = T(G[name + "_z"], dev)
    model = model_of()
    opt = model.sr = ff.SR(model.parameters())
    gradE = model.forward_from(z)
    opt.zero_grad()
    gradE.backward()
    flat = opt.flat_grad()
    P = flat.numel()
    assert opt.scores.shape == (B, P) and opt.fisher.shape == (P, P) and torch.isfinite(opt.fisher).all()
    assert torch.equal(opt.fisher, opt.fisher.T)
    err = (opt.grad - flat).abs().max().item()
    print(f"sr.grad against the sweep's gradient: {err:.3e} of {flat.abs().max().item():.3e}")
    assert err < _theta_bar() * flat.abs().max().item()
    F, g = N(opt.fisher), N(flat)
    opt.step()
    A = F + opt.shift * np.eye(P)
    delta = N(opt.delta)
    assert np.isfinite(delta).all()
    assert np.linalg.norm(A @ delta - g) <= R.sr_residual_bound(A, delta)
    # sr = None: the sweep is what it is for a model that never had the attribute
    m1, m2 = model_of(), model_of()
    m1.sr = ff.SR(m1.parameters()); m1.sr = None
    del m2.sr
    outs = []
    for m in (m1, m2):
        gE = m.forward_from(z)
        m.zero_grad()
        gE.backward()
        outs.append((gE.detach().clone(), m.Eloc.clone(), m.x.clone(), torch.cat([p.grad.reshape(-1) for p in m.parameters()])))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_training_smoke(dev):
    """3 + 3 particles, Z = 2, init_zeros(), B = 4096, seeded, 20 iterations of --optimizer sr at the defaults: E of the last iteration
    below E of the first by more than 3 sqrt(se_first^2 + se_last^2), se = E_std / sqrt(B)."""
    import fermiflow_amd as ff
    from fermiflow_amd import FermionHO2D as drv
    args = drv.build_parser().parse_args(["--nup", "3", "--ndown", "3", "--Z", "2.0", "--batch", "4096", "--optimizer", "sr"])
    torch.manual_seed(42)
    eta, mu = ff.MLP(1, args.Deta), ff.MLP(1, args.Dmu)
    eta.init_zeros(); mu.init_zeros()
    cnf = ff.CNF(ff.Backflow(eta, mu=mu), (args.t0, args.t1))
    model = ff.GSVMC(3, 3, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(args.Z), sp_potential=ff.HO())
    model.to(device=dev)
    opt = drv.make_optimizer(args, model)
    assert (opt.lr, opt.shift) == (0.05, 1e-3)
    hist = []
    for _ in range(20):
        gradE = model(args.batch)
        opt.zero_grad()
        gradE.backward()
        opt.step()
        hist.append((model.E, model.E_std / np.sqrt(args.batch)))
    print("E:", " ".join(f"{e:.4f}" for e, _ in hist))
    (e0, s0), (e1, s1) = hist[0], hist[-1]
    margin = (e0 - e1) / np.sqrt(s0 * s0 + s1 * s1)
    print(f"drop {e0 - e1:.4f} = {margin:.1f} combined standard errors")
    assert np.isfinite(e1) and margin > 3.0, (e0, e1, margin)
