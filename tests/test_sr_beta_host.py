"""Host logic of stochastic reconfiguration for BetaVMC (fermiflow_amd/sr.py: BetaSR; the driver's --optimizer flags; BetaVMC.sr).  No GPU."""
import numpy as np
import pytest
import torch

from tests import sr_ref as R


def _model(boltzmann=True):
    import fermiflow_amd as ff
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=ff.MLP(1, 4)), (0.0, 1.0))
    return ff.BetaVMC(2.0, 2, 1, 2, boltzmann, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())


def _systems(P, Ns, seed=0):
    rng = np.random.default_rng(seed)
    Om = 1.0 + rng.standard_normal((4 * P, P))
    Oc = Om - Om.mean(axis=0)
    mu = rng.random(Ns) + 0.1
    mu /= mu.sum()
    return Oc.T @ Oc / Om.shape[0], rng.standard_normal(P), np.diag(mu) - np.outer(mu, mu), rng.standard_normal(Ns)


@pytest.mark.parametrize("rescale", [True, False], ids=["rescale", "plain"])
def test_step_reproduces_two_dense_solves(rescale):
    import fermiflow_amd as ff
    model = _model()
    params = list(model.cnf.parameters())
    P, Ns = sum(p.numel() for p in params), model.Nstates
    assert P == 24 and Ns > 1
    F, g, Fp, gp = _systems(P, Ns)
    opt = ff.BetaSR(model, lr=0.05, shift=1e-3, lr_phi=0.7, shift_phi=1e-2, rescale=rescale)
    assert opt.kind == "sr" and [id(p) for p in opt.params] == [id(p) for p in params] and opt.logits is model.log_state_weights
    with torch.no_grad():      # from zero, so that the change is the product itself, without a rounding of the sum
        for p in params + [model.log_state_weights]:
            p.zero_()
    theta0 = torch.cat([p.detach().reshape(-1).clone() for p in params])
    phi0 = model.log_state_weights.detach().clone()
    off = 0
    for p in params:
        p.grad = torch.as_tensor(g[off:off + p.numel()]).view_as(p).clone()
        off += p.numel()
    model.log_state_weights.grad = torch.as_tensor(gp).clone()
    with pytest.raises(RuntimeError):
        opt.step()      # no sweep yet
    opt.fisher, opt.fisher_phi = torch.as_tensor(F), torch.as_tensor(Fp)
    opt.step()
    A, Ap = F + 1e-3 * np.eye(P), Fp + 1e-2 * np.eye(Ns)
    d, dp = opt.delta.numpy(), opt.delta_phi.numpy()
    assert np.linalg.norm(A @ d - g) <= R.sr_residual_bound(A, d)
    assert np.linalg.norm(Ap @ dp - gp) <= R.sr_residual_bound(Ap, dp)
    ref, refp = np.linalg.solve(A, g), np.linalg.solve(Ap, gp)
    np.testing.assert_allclose(d, ref, rtol=0, atol=np.linalg.cond(A) * P * R.EPS * np.abs(ref).max())
    np.testing.assert_allclose(dp, refp, rtol=0, atol=np.linalg.cond(Ap) * Ns * R.EPS * np.abs(refp).max())
    got = torch.cat([p.detach().reshape(-1) for p in params]) - theta0
    np.testing.assert_array_equal(got.numpy(), -(0.05 * opt.delta).numpy())
    np.testing.assert_array_equal((model.log_state_weights.detach() - phi0).numpy(), -(0.7 * opt.delta_phi).numpy())
    opt.zero_grad()
    assert all(p.grad is None for p in params) and model.log_state_weights.grad is None
    sd = opt.state_dict()
    assert sd == {"kind": "sr", "lr": 0.05, "shift": 1e-3, "lr_phi": 0.7, "shift_phi": 1e-2, "rescale": rescale}
    other = ff.BetaSR(model)
    assert (other.lr, other.shift, other.lr_phi, other.shift_phi, other.rescale) == (0.05, 1e-3, 0.05, 1e-3, True)
    other.load_state_dict(sd)
    assert other.state_dict() == sd


def test_betavmc_takes_a_betasr_and_nothing_else():
    import fermiflow_amd as ff
    model = _model()
    assert model.sr is None
    opt = ff.BetaSR(model)
    model.sr = opt
    assert model.sr is opt
    assert "sr" not in model.state_dict() and "_sr" not in model.state_dict()
    model.sr = None
    assert model.sr is None
    with pytest.raises(NotImplementedError, match="BetaSR"):
        model.sr = ff.SR(model.parameters())
    with pytest.raises(NotImplementedError, match="BetaSR"):
        model.sr = object()
    assert model.sr is None


def test_driver_flags_and_default_optimizer():
    import fermiflow_amd as ff
    from fermiflow_amd import BetaFermionHO2D as drv
    args = drv.build_parser().parse_args([])
    assert (args.optimizer, args.sr_lr, args.sr_shift, args.sr_lr_phi, args.sr_shift_phi) == ("adam", 0.05, 1e-3, None, None)
    a2 = drv.build_parser().parse_args(["--optimizer", "sr", "--sr_lr", "0.1", "--sr_shift", "1e-2", "--sr_lr_phi", "2.0", "--sr_shift_phi", "1e-4"])
    assert (a2.optimizer, a2.sr_lr, a2.sr_shift, a2.sr_lr_phi, a2.sr_shift_phi) == ("sr", 0.1, 1e-2, 2.0, 1e-4)
    with pytest.raises(SystemExit):
        drv.build_parser().parse_args(["--optimizer", "sgd"])
    model = _model()
    opt = drv.make_optimizer(args, model)
    assert model.sr is None and type(opt) is type(drv.make_adam(model.parameters(), lr=1e-2))
    assert opt.param_groups[0]["lr"] == 1e-2
    opt2 = drv.make_optimizer(a2, model)
    assert model.sr is opt2 and isinstance(opt2, ff.BetaSR)
    assert (opt2.lr, opt2.shift, opt2.lr_phi, opt2.shift_phi) == (0.1, 1e-2, 2.0, 1e-4)
    opt3 = drv.make_optimizer(drv.build_parser().parse_args(["--optimizer", "sr"]), model)
    assert (opt3.lr, opt3.shift, opt3.lr_phi, opt3.shift_phi) == (0.05, 1e-3, 0.05, 1e-3)


def test_checkpoint_round_trip_and_optimizer_kind(tmp_path):
    from fermiflow_amd import BetaFermionHO2D as drv, checkpoint
    sr_args = drv.build_parser().parse_args(["--optimizer", "sr", "--sr_lr", "0.1", "--sr_shift", "1e-2", "--sr_lr_phi", "2.0"])
    adam_args = drv.build_parser().parse_args([])
    m = _model(boltzmann=False)
    opt = drv.make_optimizer(sr_args, m)
    path = str(tmp_path / "sr.pt")
    checkpoint.save(path, m, opt, 7)
    m2 = _model(boltzmann=False)
    opt2 = drv.make_optimizer(drv.build_parser().parse_args(["--optimizer", "sr"]), m2)
    assert checkpoint.load(path, m2, opt2) == 7
    assert (opt2.lr, opt2.shift, opt2.lr_phi, opt2.shift_phi, opt2.rescale) == (0.1, 1e-2, 2.0, 1e-2, True)
    assert m2.sr is opt2
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="--optimizer sr"):      # an SR checkpoint under Adam ...
        m5 = _model()
        checkpoint.load(path, m5, drv.make_optimizer(adam_args, m5))
    m3 = _model()
    adam_path = str(tmp_path / "adam.pt")
    checkpoint.save(adam_path, m3, drv.make_optimizer(adam_args, m3), 3)
    m4 = _model()
    with pytest.raises(ValueError, match="--optimizer adam"):    # ... and an Adam checkpoint under SR
        checkpoint.load(adam_path, m4, drv.make_optimizer(sr_args, m4))
