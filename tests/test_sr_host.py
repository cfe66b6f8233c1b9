"""Host logic of stochastic reconfiguration (fermiflow_amd/sr.py, the driver's --optimizer flags, BetaVMC's refusal).  No GPU."""
import numpy as np
import pytest
import torch

from tests import sr_ref as R


def _system(P, seed=0):
    rng = np.random.default_rng(seed)
    Om = 1.0 + rng.standard_normal((4 * P, P))
    Oc = Om - Om.mean(axis=0)
    return Oc.T @ Oc / Om.shape[0], rng.standard_normal(P)


@pytest.mark.parametrize("rescale", [True, False], ids=["rescale", "plain"])
@pytest.mark.parametrize("P", [6, 75, 300])
def test_step_reproduces_the_dense_solve(P, rescale):
    from fermiflow_amd.sr import SR
    F, g = _system(P)
    sizes = [P // 3, P // 3, P - 2 * (P // 3)]
    params = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64)) for n in sizes]
    theta0 = [p.detach().clone() for p in params]
    off = 0
    for p, n in zip(params, sizes):
        p.grad = torch.as_tensor(g[off:off + n]).clone()
        off += n
    opt = SR(params, lr=0.05, shift=1e-3, rescale=rescale)
    with pytest.raises(RuntimeError):
        opt.step()      # no Fisher matrix yet
    opt.fisher = torch.as_tensor(F)
    opt.step()
    A = F + 1e-3 * np.eye(P)
    ref = np.linalg.solve(A, g)
    delta = opt.delta.numpy()
    assert np.linalg.norm(A @ delta - g) <= R.sr_residual_bound(A, delta)
    np.testing.assert_allclose(delta, ref, rtol=0, atol=np.linalg.cond(A) * P * R.EPS * np.abs(ref).max())
    got = torch.cat([p.detach() - t for p, t in zip(params, theta0)]).numpy()
    np.testing.assert_array_equal(got, -(0.05 * opt.delta).numpy())
    opt.zero_grad()
    assert all(p.grad is None for p in params)
    sd = opt.state_dict()
    assert sd["kind"] == "sr"
    SR(params).load_state_dict(sd)


def test_betavmc_refuses_sr():
    import fermiflow_amd as ff
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=None), (0.0, 1.0))
    model = ff.BetaVMC(2.0, 2, 1, 2, True, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    assert model.sr is None
    model.sr = None
    with pytest.raises(NotImplementedError):
        model.sr = ff.SR(model.parameters())


def test_driver_flags_and_default_optimizer():
    import fermiflow_amd as ff
    from fermiflow_amd import FermionHO2D as drv
    args = drv.build_parser().parse_args([])
    assert (args.optimizer, args.sr_lr, args.sr_shift) == ("adam", 0.05, 1e-3)
    a2 = drv.build_parser().parse_args(["--optimizer", "sr", "--sr_lr", "0.1", "--sr_shift", "1e-2"])
    assert (a2.optimizer, a2.sr_lr, a2.sr_shift) == ("sr", 0.1, 1e-2)
    with pytest.raises(SystemExit):
        drv.build_parser().parse_args(["--optimizer", "sgd"])
    cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=ff.MLP(1, 4)), (0.0, 1.0))
    model = ff.GSVMC(1, 1, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    assert model.sr is None
    opt = drv.make_optimizer(args, model)
    assert model.sr is None and type(opt) is type(drv.make_adam(model.parameters(), lr=1e-2))
    assert opt.param_groups[0]["lr"] == 1e-2
    opt2 = drv.make_optimizer(a2, model)
    assert model.sr is opt2 and isinstance(opt2, ff.SR) and (opt2.lr, opt2.shift) == (0.1, 1e-2)


def test_checkpoint_round_trip_and_optimizer_kind(tmp_path):
    import fermiflow_amd as ff
    from fermiflow_amd import FermionHO2D as drv, checkpoint

    def model_of():
        cnf = ff.CNF(ff.Backflow(ff.MLP(1, 4), mu=ff.MLP(1, 4)), (0.0, 1.0))
        return ff.GSVMC(1, 1, ff.HO2D(), ff.FreeFermion(device="cpu"), cnf, ff.CoulombPairPotential(0.5), sp_potential=ff.HO())
    sr_args = drv.build_parser().parse_args(["--optimizer", "sr", "--sr_lr", "0.1", "--sr_shift", "1e-2"])
    adam_args = drv.build_parser().parse_args([])
    m = model_of()
    opt = drv.make_optimizer(sr_args, m)
    path = str(tmp_path / "sr.pt")
    checkpoint.save(path, m, opt, 7)
    m2 = model_of()
    opt2 = drv.make_optimizer(drv.build_parser().parse_args(["--optimizer", "sr"]), m2)
    assert checkpoint.load(path, m2, opt2) == 7
    assert (opt2.lr, opt2.shift, opt2.rescale) == (0.1, 1e-2, True)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="--optimizer sr"):      # an SR checkpoint under Adam ...
        checkpoint.load(path, model_of(), drv.make_optimizer(adam_args, model_of()))
    m3 = model_of()
    adam_path = str(tmp_path / "adam.pt")
    checkpoint.save(adam_path, m3, drv.make_optimizer(adam_args, m3), 3)
    m4 = model_of()
    with pytest.raises(ValueError, match="--optimizer adam"):    # ... and an Adam checkpoint under SR
        checkpoint.load(adam_path, m4, drv.make_optimizer(sr_args, m4))
