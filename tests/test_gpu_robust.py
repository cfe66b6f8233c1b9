"""The robust estimator (csrc/ff_robust.h) on the device, through fermiflow_amd.native and GSVMC.clip_eloc: the cases of
tests/robust_cases.py (run under the host simulator by tests/test_robust_hostsim.py) at B = 1, 2, 257 and 65 539 -- one, one, one and
65 segments, the last of three walkers --, three tests that pin the real adjoint kernels behind it (failed rows, dyadic energies, a
sweep end to end), and the sweep on two ranks over gloo and on one rank over RCCL.  Floating-point results go by the derived bounds of
tests/robust_ref.py; integers, the median and everything compared between two device results are exact."""
import math

import numpy as np
import pytest
import torch

from tests import robust_cases as cases
from tests import robust_ref as R
from tests.common import N, T, bits_equal, cu_count, kernel_families, looping_batch, make_flow, net_arrays

pytestmark = pytest.mark.gpu

RT, AT = 1e-9, 1e-11
SIZES = [1, 2, 257, 65539]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


class _Dev:
    """the backend of tests/robust_cases.py over fermiflow_amd.native"""

    def __init__(self, dev):
        self.dev = dev

    def robust(self, e, logp, k, shift):
        from fermiflow_amd import native
        stat = native.energy_robust(T(e, self.dev), None if logp is None else T(logp, self.dev), k, T([shift], self.dev))
        return N(stat)

    def apply(self, e, logp, stat, n_global, finish, z=None, g=None):
        from fermiflow_amd import native
        st = T(stat, self.dev)
        zt, gt = (None, None) if z is None else (T(z, self.dev), T(g, self.dev))
        u, s = native.energy_robust_apply(T(e, self.dev), T(logp, self.dev), st, n_global, bool(finish), zt, gt)
        return N(u), N(s), N(st), None if zt is None else N(zt), None if gt is None else N(gt)


@pytest.mark.parametrize("B", SIZES)
def test_sizes(dev, B):
    cases.sizes(_Dev(dev), B)


@pytest.mark.parametrize("B", SIZES)
def test_all_energies_equal(dev, B):
    cases.all_equal(_Dev(dev), B)


@pytest.mark.parametrize("B", SIZES[2:])
def test_ties_last_bit_outliers_invalid(dev, B):
    K = _Dev(dev)
    cases.heavy_ties(K, B)
    cases.last_digit(K, B)
    cases.finite_outliers(K, B)
    cases.every_walker_invalid(K, B)


@pytest.mark.parametrize("B", SIZES[2:])
def test_clip_widths_and_padding(dev, B):
    cases.clip_widths(_Dev(dev), B)
    cases.padding(_Dev(dev), B)


@pytest.mark.parametrize("n,d", [(1, 2), (6, 2), (20, 3)])
def test_apply_sanitises_invalid_rows_only(dev, n, d):
    cases.rows(_Dev(dev), 2049, n, d)


def test_one_workspace_serves_twenty_calls(dev):
    """robust + apply twenty times on the cached workspace with no host sync in between: bit-identical results, and the workspace's
    tickets, selection state and histogram read zero afterwards"""
    from fermiflow_amd import native
    B = 65539
    e, lp = R.spoil(*R.energies(B))
    et, lt, sh = T(e, dev), T(lp, dev), T([29.5], dev)
    res = []
    for _ in range(20):
        stat = native.energy_robust(et, lt, 5.0, sh)
        u, s = native.energy_robust_apply(et, lt, stat, B, True)
        res.append((stat, u, s))
    torch.cuda.synchronize(dev)
    key = (str(et.device), int(torch.cuda.current_stream(dev).cuda_stream), B)
    assert not N(native._ROB_WS[key][:8 + 2048].view(torch.int64)).any()
    for stat, u, s in res[1:]:
        assert bits_equal(N(stat), N(res[0][0])) and bits_equal(N(u), N(res[0][1])) and bits_equal(N(s), N(res[0][2]))


# ---------------------------------------------------------------------------------------------------- behind it: the adjoint kernels
@pytest.fixture(scope="module")
def flow(dev, golden):
    """3 + 3 particles in two dimensions at the smallest batch that loops the adjoint's grid (tests/test_gpu_geometry.py picks it so)"""
    eta, mu = net_arrays(golden["g5_gsvmc"], "z2_nt_")
    net = make_flow(eta, mu, dev).v_wrapper.v.net(radial="table")
    B = looping_batch(kernel_families("adjoint", 6, 2, cu_count()))
    g = torch.Generator().manual_seed(61)
    z = torch.randn(B, 6, 2, generator=g, dtype=torch.float64).to(dev)
    g0 = torch.randn(B, 6, 2, generator=g, dtype=torch.float64).to(dev)
    return net, B, z, g0


def test_failed_rows_contribute_nothing_to_the_gradient(dev, flow):
    """NaN rows and NaN energies at a handful of walkers: robust -> apply -> the energy-seeded adjoint gives a finite gradient that agrees
    with the adjoint run with explicit seeds on the valid walkers alone to 1e-12 of its largest entry (the reduction alone)."""
    from fermiflow_amd import native
    net, B, z, g0 = flow
    e, lp = R.energies(B, seed=3)
    bad = np.array([0, 1, 63, 64, B // 2, B - 1])
    e[bad[:4]] = np.nan
    lp[bad[4:]] = np.nan                                  # (a finite energy beside a failed log-probability is a failed walker too)
    zt, gt = z.clone(), g0.clone()
    zt[T(bad, dev, torch.int64)] = float("nan")
    gt[T(bad, dev, torch.int64)] = float("nan")
    et, lt = T(e, dev), T(lp, dev)
    stat = native.energy_robust(et, lt, 2.0, T([29.5], dev))
    u, _ = native.energy_robust_apply(et, lt, stat, B, True, zt, gt)
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    _, gp = native.cnf_adjoint(net, zt, gt, None, 0.0, 1.0, RT, AT, need_gx=False, energy=(u, zero, 1.0 / B))
    ok = torch.ones(B, dtype=torch.bool, device=dev)
    ok[T(bad, dev, torch.int64)] = False
    w = (u[ok] - 0.0) * (1.0 / B)
    _, gp_valid = native.cnf_adjoint(net, z[ok].contiguous(), (w[:, None, None] * g0[ok]).contiguous(), (-w).contiguous(), 0.0, 1.0, RT, AT,
                                     need_gx=False)
    gp, gp_valid, st = N(gp), N(gp_valid), N(stat)
    assert st[R.NV] == B - len(bad) and st[R.NC] > 0 and np.isfinite(gp).all() and np.abs(gp_valid).max() > 0
    err = np.abs(gp - gp_valid).max() / np.abs(gp_valid).max()
    print(f"failed rows B={B}: n_v {int(st[R.NV])}, n_c {int(st[R.NC])}, gradient against the valid walkers alone {err:.2e} of its largest entry")
    assert err < 1e-12, err
    assert bits_equal(N(zt[~ok]), np.broadcast_to(R.safe_rows(6, 2), (len(bad), 6, 2))) and not N(gt[~ok]).any()
    assert torch.equal(zt[ok], z[ok]) and torch.equal(gt[ok], g0[ok])


def test_dyadic_energies_give_todays_gradient_bit_for_bit(dev, flow):
    """e_b = 2.5 + k_b / 64 with sum k_b = 0, N = n_v = 256, k = 1e6: every step of the robust estimator is exact, so u_b = e_b - 2.5 and
    the gradient is torch.equal to the plain energy-seeded call"""
    from fermiflow_amd import native
    net, _, z, g0 = flow
    B = 256
    z, g0 = z[:B].contiguous(), g0[:B].contiguous()
    e = R.dyadic(B)
    et, lt = T(e, dev), T(np.linspace(-3.0, 3.0, B), dev)
    stat = native.energy_robust(et, lt, 1e6, T([0.0], dev))
    u, _ = native.energy_robust_apply(et, lt, stat, B, True, z, g0)
    assert bits_equal(N(u), e - 2.5) and N(stat)[R.NV] == B and N(stat)[R.NC] == 0 and N(stat)[R.EC] == 2.5
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    _, gp = native.cnf_adjoint(net, z, g0, None, 0.0, 1.0, RT, AT, need_gx=False, energy=(u, zero, 1.0 / B))
    _, gp0 = native.cnf_adjoint(net, z, g0, None, 0.0, 1.0, RT, AT, need_gx=False,
                                energy=(et, torch.tensor([2.5], dtype=torch.float64, device=dev), 1.0 / B))
    assert torch.equal(gp, gp0) and torch.isfinite(gp).all() and gp.abs().max() > 0


@pytest.mark.parametrize("nup,ndn", [(3, 3), (1, 1)])
def test_sweep_with_a_failed_walker(dev, nup, ndn):
    """End to end: 257 base walkers from the sampler, one coordinate NaN.  Default: E, the value and eta's gradients are NaN (unchanged).  With
    clip_eloc = 5: 256 valid walkers, E / E_std of the finite local energies (the bars of test_gsvmc_sweep_estimator_at_ragged_batches),
    the statistics of tests/robust_ref.py on model.Eloc, finite gradients, carried sweep state finite, a second sweep finite."""
    import __graft_entry__ as G
    B = 257
    torch.manual_seed(5)
    model = G._model(dev, nup, ndn, 2.0)
    z = model.basedist.sample(model.orbitals_up, model.orbitals_down, (B,)).clone()
    z[17, 0, 0] = float("nan")
    out = model.forward_from(z)
    out.backward()
    assert math.isnan(model.E) and math.isnan(model.E_std) and math.isnan(float(out.detach())) and model.Eloc_weights is None
    # (measured on the default path, at both shapes: all 150 entries of eta's three gradients are NaN, none of mu's 150 -- the poisoned
    # gradient is pinned where it shows, mu's entries are not part of the contract)
    grads = dict(model.named_parameters())
    assert all(torch.isnan(p.grad).all() for name, p in grads.items() if ".eta." in name) and sum(".eta." in name for name in grads) == 3

    model = G._model(dev, nup, ndn, 2.0)
    model.clip_eloc = 5
    out = model.forward_from(z)
    out.backward()
    eloc, u, stat = N(model.Eloc), N(model.Eloc_weights), N(model.robust_stat)
    fin = np.isfinite(eloc)
    assert model.n_valid == 256 == int(fin.sum()) and not fin[17] and u[17] == 0.0
    Eref = math.fsum(eloc[fin]) / 256
    sref = math.sqrt(math.fsum((eloc[fin] - Eref) ** 2) / 255)
    print(f"{nup}+{ndn} robust sweep: E {model.E!r} (fsum {Eref!r}), E_std {model.E_std!r} ({sref!r}), n_clipped {model.n_clipped}, "
          f"median {model.E_median!r}, width {model.E_width!r}")
    assert abs(model.E - Eref) <= 1e-12 * abs(Eref) and abs(model.E_std - sref) <= 1e-10 * sref
    want, scale = R.statistics(eloc, None, 5.0, 0.0)                 # (the first sweep's shift is 0)
    assert stat[R.NV] == want[R.NV] and bits_equal(stat[R.MED], want[R.MED]) and model.E_median == want[R.MED]
    for i in (R.WIDTH, R.LO, R.HI, R.E, R.ESS):
        assert abs(stat[i] - want[i]) <= R.FIN_TOL * scale[i], (i, stat[i], want[i])
    c, nc, ec, ec_scale = R.clipped(eloc, None, stat[R.LO], stat[R.HI], stat[R.MED])
    assert stat[R.NC] == nc == model.n_clipped and abs(stat[R.EC] - ec) <= R.FIN_TOL * ec_scale and model.E_width == stat[R.WIDTH]
    uw, ub, _, _ = R.weights(eloc, np.zeros(B), c, stat[R.EC], B)
    assert (np.abs(u - uw) <= ub).all()
    assert math.isfinite(float(out.detach())) and all(torch.isfinite(p.grad).all() for p in model.parameters())
    # the sweep state that carries over
    assert torch.isfinite(model._h_flow).all() and (model._h_tab is None or torch.isfinite(model._h_tab).all())
    for p in model.parameters():
        p.grad = None
    out2 = model(B)
    out2.backward()
    assert model.n_valid == B and math.isfinite(model.E) and math.isfinite(model.E_std) and math.isfinite(float(out2.detach()))
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


# ------------------------------------------------------------------------------------------------------------ data parallelism
def _dp_run(rank, world, port, B, out, backend="gloo"):
    """one sweep with clip_eloc on GIVEN base walkers (one of them failed), this rank's shard of a global batch of B; backend "nccl":
    a single rank over RCCL with every collective of the sweep forced to run (FERMIFLOW_DIST_FORCE)"""
    import os
    import torch.distributed as dist
    import __graft_entry__ as G
    from fermiflow_amd import dist as D
    dev = torch.device("cuda:0")
    if world > 1 or backend == "nccl":
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        if backend == "nccl":
            os.environ["FERMIFLOW_DIST_FORCE"] = "1"
            torch.cuda.set_device(dev)
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    model = G._model(dev, 3, 3, 2.0)
    model.clip_eloc = 2.0
    z = torch.randn(B, 6, 2, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    z[700, 2, 1] = float("nan")
    off, cnt = D.shard(B)
    g = model.forward_from(z[off:off + cnt].to(dev), batch=B)
    g.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    out[rank] = (N(model.robust_stat), N(model.Eloc_weights), N(model.Eloc), float(g.detach()), N(grads), model.E, model.E_std, model.n_valid,
                 model.n_clipped, off, cnt)
    if dist.is_initialized():
        dist.destroy_process_group()


def test_two_ranks_with_uneven_shards_equal_one_rank():
    """1025 walkers on two ranks sharing the GPU (gloo; shards of 513 and 512, the failed walker in the second): one padded all-gather,
    the same statistics on both ranks -- bit-identical to the single process --, the same weights, the gradient to rounding."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dist import _free_port
    B = 1025
    mgr = mp.get_context("spawn").Manager()
    one, two = mgr.dict(), mgr.dict()
    mp.spawn(_dp_run, args=(1, 0, B, one), nprocs=1, join=True)
    mp.spawn(_dp_run, args=(2, _free_port(), B, two), nprocs=2, join=True)
    stat, u, eloc, val, grads, E, Es, nv, nc, _, _ = one[0]
    assert nv == B - 1 and nc > 0 and np.isfinite(grads).all() and math.isfinite(E) and math.isfinite(Es) and u[700] == 0.0
    for r in (0, 1):
        stat2, u2, eloc2, val2, grads2, E2, Es2, nv2, nc2, off, cnt = two[r]
        assert cnt == (513, 512)[r] and bits_equal(eloc2, eloc[off:off + cnt])
        assert bits_equal(stat2[:R.VALUE], stat[:R.VALUE]) and bits_equal(u2, u[off:off + cnt]), (r, stat2, stat)
        assert (E2, Es2, nv2, nc2) == (E, Es, nv, nc)
        assert abs(val2 - val) <= 1e-10 * max(1.0, abs(val))
        np.testing.assert_allclose(grads2, grads, rtol=0, atol=1e-10 * np.abs(grads).max())
    assert bits_equal(two[0][0], two[1][0]) and two[0][3] == two[1][3] == two[0][0][R.VALUE]      # (the value is in stat[9] on every rank)


def test_rccl_single_rank_robust_sweep_equals_plain_robust_sweep():
    """the nccl (RCCL) branch of the padded all-gather and of the all-reduce of the apply step's sum, inside a full sweep: changes nothing"""
    import torch.multiprocessing as mp
    from tests.test_gpu_dist import _free_port
    B = 1025
    mgr = mp.get_context("spawn").Manager()
    one, rc = mgr.dict(), mgr.dict()
    mp.spawn(_dp_run, args=(1, 0, B, one), nprocs=1, join=True)
    mp.spawn(_dp_run, args=(1, _free_port(), B, rc, "nccl"), nprocs=1, join=True)
    stat, u, eloc, val, grads = one[0][:5]
    stat2, u2, eloc2, val2, grads2 = rc[0][:5]
    assert bits_equal(eloc2, eloc) and bits_equal(stat2, stat) and bits_equal(u2, u) and val2 == val and bits_equal(grads2, grads)
    assert one[0][5:] == rc[0][5:]
