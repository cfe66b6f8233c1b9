"""The one-body density matrix on the MI355X: ff_slater_sign and ff_obdm_accumulate against the numpy restatement (tests/obdm_ref.py),
the whole pipeline inside a GSVMC sweep on a flow that is zero (where an identity is exact), on the benchmark's flow against the CPU
oracle, and inside a BetaVMC sweep with each walker's own state."""
import numpy as np
import pytest
import torch

import fermiflow_amd as ff
from fermiflow_amd import OneBodyDensityMatrix, native
from oracle import oracle as O
from tests import obdm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


@pytest.mark.parametrize("nup,ndn", [(2, 1), (3, 3), (12, 12)], ids=["2+1", "3+3", "12+12"])
def test_sign_and_accumulate_on_the_device(dev, nup, ndn):
    """the hostsim cases at B in {65, 2 CHUNK + 3}, with the same bounds; two runs on fresh buffers are bitwise equal"""
    Bmax = 2 * R.CHUNK + 3
    z = R.good_walkers(40 + 3 * nup + ndn, Bmax, nup, ndn)
    ref, margin = R.slater_sign(z, nup, ndn)
    assert (margin > R.MARGIN).all()
    tu = native.orbital_table(list(range(nup)), dev) if nup else None
    td = native.orbital_table(list(range(ndn)), dev) if ndn else None
    full = R.inputs(200 + 5 * nup + ndn, Bmax, nup, ndn)
    for B in (65, Bmax):
        got = native.slater_sign(tu, td, nup, ndn, _t(z[:B], dev)).cpu().numpy()
        assert np.array_equal(got, ref[:B])
        inp = {k: v[:B] for k, v in full.items()}
        tin = {k: _t(v, dev) for k, v in inp.items()}
        for nshells in (1, 2, 4, 8):
            a, b = OneBodyDensityMatrix(nup, ndn, nshells=nshells), OneBodyDensityMatrix(nup, ndn, nshells=nshells)
            a.accumulate_raw(**tin)
            b.accumulate_raw(**tin)
            torch.cuda.synchronize()
            assert np.array_equal(a._buf.cpu().numpy(), b._buf.cpu().numpy())
            r = R.estimate(**inp, sigma=1.0, nshells=nshells, nup=nup, ft=np.longdouble)
            delta = R.term_delta(**inp, sigma=1.0, nshells=nshells, nup=nup)
            got = R.split(a._buf.cpu().numpy(), nshells)
            bound = R.bound(r, delta)
            err = np.abs(got["sum"] - r["T"].astype(np.float64))
            print(f"{nup}+{ndn} B={B} nshells={nshells}: delta {delta:.3e} max err {err.max():.3e} max err / bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
            assert (got["calls"], got["walkers"], got["ticket"]) == (1, B, 0) and np.array_equal(got["invalid"], r["invalid"])
            assert (err <= bound).all()
            assert np.array_equal(got["sum"], got["sum"].transpose(0, 2, 1))
    # a coincident pair and a NaN coordinate
    w = z[:4].copy()
    w[0, 1] = w[0, 0]
    w[1, 0, 1] = np.nan
    got = native.slater_sign(tu, td, nup, ndn, _t(w, dev)).cpu().numpy()
    assert got[0] == 0.0 and np.isnan(got[1]) and np.array_equal(got[2:], ref[2:4])
    with pytest.raises(ValueError):
        a.accumulate_raw(**{k: v[:10] for k, v in tin.items()})          # equal calls only


def _zero_flow(model):
    v = model.cnf.v_wrapper.v
    v.eta.init_zeros()
    v.mu.init_zeros()
    return model


def _ratios(x, rp, nup, ndn, tab_up=None, tab_dn=None, state=0):
    """numpy: q_i of ONE walker x (n, 2) by determinants with row i replaced, the scale |phi(r')| |Phi^-1 e_i| of its rounding error
    and cond(Phi), per particle"""
    q, scale, cond = [], [], []
    for s, (lo, ns, tab) in enumerate(((0, nup, tab_up), (nup, ndn, tab_dn))):
        if not ns:
            continue
        orb = R._tab(ns, tab)[state]
        Phi = R.orbitals(orb, x[lo:lo + ns, 0], x[lo:lo + ns, 1])
        at_r = R.orbitals(orb, rp[s, 0], rp[s, 1])
        inv = np.linalg.inv(Phi)                                        # q_i = (phi(r')^T Phi^-1)_i
        q += list(at_r @ inv)
        scale += [np.linalg.norm(at_r) * np.linalg.norm(inv[:, i]) for i in range(ns)]
        cond += [np.linalg.cond(Phi)] * ns
    return np.array(q), np.array(scale), np.array(cond)


def test_zero_flow_end_to_end(dev):
    """GSVMC(3, 3) with a zero flow, one sweep: for occupied a, c the walker's A_a is phi_a(r') exactly, so the occupied block of sum
    is sum_b phi_a(r'_b) phi_c(r'_b) / g(r'_b), recomputed here from obdm.last["rprime"].  Bound per walker as in the hostsim test,
    64 eps cond(Phi(x_b)) (mass_a |C_c| + |C_a| mass_c) / 2, plus the summation's B eps sum_b |term_b|."""
    from __graft_entry__ import _model
    B, nshells, nup, ndn = 1024, 3, 3, 3
    model = _zero_flow(_model(dev))
    obdm = OneBodyDensityMatrix(nup, ndn, nshells=nshells)
    model.obdm = obdm
    torch.manual_seed(3)
    model(B)
    torch.cuda.synchronize()
    c = obdm.counts()
    assert (c["calls"], c["walkers"], c["invalid_up"], c["invalid_down"]) == (1, B, 0, 0)
    x, rp = model.x.cpu().numpy(), obdm.last["rprime"].cpu().numpy()
    got = R.split(obdm._buf.cpu().numpy(), nshells)["sum"]
    for s, lo in enumerate((0, nup)):
        want, bound, mag = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
        C = R.weights(rp[:, s], 1.0, nshells)[:, :3]
        at_r = R.orbitals(range(3), rp[:, s, 0], rp[:, s, 1])
        for b in range(B):
            Phi = R.orbitals(range(3), x[b, lo:lo + 3, 0], x[b, lo:lo + 3, 1])
            q = at_r[b] @ np.linalg.inv(Phi)
            mass = np.abs(Phi * q[:, None]).sum(0)
            term = 0.5 * (np.outer(at_r[b], C[b]) + np.outer(C[b], at_r[b]))
            want += term
            mag += np.abs(term)
            bound += 64.0 * R.EPS * np.linalg.cond(Phi) * 0.5 * (np.outer(mass, np.abs(C[b])) + np.outer(np.abs(C[b]), mass))
        bound += B * R.EPS * mag
        err = np.abs(got[s][:3, :3] - want)
        print(f"species {s}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}; tr rho {np.trace(got[s]) / B:.4f}")
        assert (err <= bound).all()


# torch seeds of the sweeps below, chosen so that no moved (or unmoved) base walker of the oracle's 1e-10 solve has a determinant within
# 1e-3 of zero relative to its row norms (the test asserts it: a property of the oracle's walkers alone)
FLOW_SEEDS = {(2, 1): 2, (3, 3): 6}


@pytest.mark.parametrize("nup,ndn", [(2, 1), (3, 3)], ids=["2+1", "3+3"])
def test_with_the_benchmarks_flow(dev, nup, ndn, seed=None):
    """The pipeline's moved walkers against the CPU oracle's backward flow at rtol 1e-10 / atol 1e-12: sign_moved exactly, logp_moved
    within 10 x what the ORACLE's own 1e-6 / 1e-8 solve differs from its 1e-10 solve (printed; DESIGN 3ac records it).  And the hook
    only reads: E_loc and the gradient of the sweep are bitwise those of the same sweep without it."""
    from __graft_entry__ import _model
    B, n = 64, nup + ndn
    out = []
    for with_obdm in (True, False):
        model = _model(dev, nup, ndn)
        obdm = OneBodyDensityMatrix(nup, ndn, nshells=4) if with_obdm else None
        model.obdm = obdm
        torch.manual_seed(FLOW_SEEDS[(nup, ndn)] if seed is None else seed)
        g = model(B)
        g.backward()
        torch.cuda.synchronize()
        out.append((model.Eloc.cpu().numpy().copy(), [p.grad.cpu().numpy().copy() for p in model.parameters()], model.x.cpu().numpy().copy(), obdm, model))
    (e1, g1, x, obdm, model), (e0, g0, x0, _, _) = out
    assert e1.tobytes() == e0.tobytes() and x.tobytes() == x0.tobytes()
    assert len(g1) == len(g0) and all(a.tobytes() == b.tobytes() for a, b in zip(g1, g0))
    c = obdm.counts()
    assert (c["calls"], c["walkers"], c["invalid_up"], c["invalid_down"]) == (1, B, 0, 0)
    v = model.cnf.v_wrapper.v
    net = O.Net(tuple(t.detach().cpu().numpy() for t in (v.eta.fc1.weight, v.eta.fc1.bias, v.eta.fc2.weight)),
                tuple(t.detach().cpu().numpy() for t in (v.mu.fc1.weight, v.mu.fc1.bias, v.mu.fc2.weight)))
    rp = obdm.last["rprime"].cpu().numpy()
    xm = np.repeat(x[:, None], n, axis=1)                               # [walker, moved particle, row, coordinate]
    for i in range(n):
        xm[:, i, i] = rp[:, 0 if i < nup else 1]
    xm = xm.reshape(B * n, n, 2)
    z_hi, dl_hi, _ = O.cnf_delta_logp(xm, net, rtol=1e-10, atol=1e-12)
    z_lo, dl_lo, _ = O.cnf_delta_logp(xm, net, rtol=1e-6, atol=1e-8)
    lp_hi = O.logprob(z_hi, nup, ndn, derivs=False) - dl_hi
    lp_lo = O.logprob(z_lo, nup, ndn, derivs=False) - dl_lo
    sign_ref, margin = R.slater_sign(z_hi, nup, ndn)
    print(f"{nup}+{ndn}: smallest relative |det| of the oracle's moved base walkers {margin.min():.3e}")
    assert (margin > 1e-3).all()                                        # the seed leaves no moved walker out
    assert np.array_equal(obdm.last["sign_moved"].cpu().numpy().reshape(-1), sign_ref)
    z0, _, _ = O.cnf_delta_logp(x, net, rtol=1e-10, atol=1e-12)
    s0, m0 = R.slater_sign(z0, nup, ndn)
    print(f"{nup}+{ndn}: smallest relative |det| of the oracle's unmoved base walkers {m0.min():.3e}")
    assert (m0 > 1e-3).all() and np.array_equal(obdm.last["sign"].cpu().numpy(), s0)
    own = float(np.abs(lp_lo - lp_hi).max())
    err = float(np.abs(obdm.last["logp_moved"].cpu().numpy().reshape(-1) - lp_hi).max())
    print(f"{nup}+{ndn}: oracle 1e-6 vs 1e-10 solve of the moved walkers: max |dlogp| {own:.3e}; pipeline vs oracle 1e-10: {err:.3e}")
    assert err <= 10.0 * own
    assert np.isfinite(obdm.matrix()["up"]).all()


def test_inside_a_betavmc_sweep(dev):
    """nup = 3, ndown = 0, deltaE = 2, zero flow, given base walkers in sorted states: q = sign sign' exp((logp' - logp) / 2) from
    obdm.last against numpy's determinant ratios under each walker's OWN state.  q_i = phi(r')^T Phi^-1 e_i: its rounding error is
    bounded by 64 eps cond(Phi) |phi(r')| |Phi^-1 e_i|."""
    B, nup = 256, 3
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 50), mu=ff.MLP(1, 50)), (0.0, 1.0))
    model = ff.BetaVMC(10.0, nup, 0, 2.0, True, ff.HO2D(), ff.FreeFermion(device=dev), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    _zero_flow(model).to(device=dev)
    Ns = model.Nstates
    assert Ns > 1
    rng = np.random.default_rng(12)
    ws = np.sort(rng.integers(0, Ns, B)).astype(np.int32)
    assert len(set(ws)) == Ns
    tab = model._state_tables(dev)[0].cpu().numpy()
    z = R.good_walkers(13, B, nup, 0, tab, None, ws)
    obdm = OneBodyDensityMatrix(nup, 0, nshells=4)
    model.obdm = obdm
    model.forward_from(_t(z, dev), ws)
    torch.cuda.synchronize()
    c = obdm.counts()
    assert (c["calls"], c["walkers"], c["invalid_up"], c["invalid_down"]) == (1, B, 0, 0)
    last = {k: v.cpu().numpy() for k, v in obdm.last.items()}
    q_dev = (last["sign"][:, None] * last["sign_moved"]) * np.exp(0.5 * (last["logp_moved"] - last["logp"][:, None]))
    worst, differs = 0.0, 0
    for b in range(B):
        q, scale, cond = _ratios(z[b], last["rprime"][b], nup, 0, tab, None, ws[b])
        bound = 64.0 * R.EPS * cond * scale
        worst = max(worst, float((np.abs(q_dev[b] - q) / bound).max()))
        assert (np.abs(q_dev[b] - q) <= bound).all(), (b, ws[b])
        q0, _, _ = _ratios(z[b], last["rprime"][b], nup, 0, tab, None, 0)
        differs += int(ws[b] != 0 and np.abs(q0 - q).max() > 1e-6)
    print(f"BetaVMC: {Ns} states, max |q - numpy| / bound {worst:.3e}")
    assert differs > B // 4                                              # (the own state matters: state 0's ratios are others)
