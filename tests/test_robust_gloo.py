"""world_size-2 and -3 CPU tests (gloo) of the data-parallel robust estimator, in the call order of GSVMC._robust_estimate
(fermiflow_amd/VMC.py): every rank marks its invalid walkers, ONE padded all-gather (dist.all_gather_padded), the padding cut off by
the shard sizes every rank knows, ff_energy_robust on the same N-vector on every rank, ff_energy_robust_apply on the shard, one
all-reduce of its one-double sum -- with the kernels' host build (tests/hostsim) standing in for the GPU.  Uneven shards: statistics and
u on each rank are bit-identical to the single-process call on the whole batch."""
import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import robust_ref as R
from tests.common import bits_equal
from tests.test_dist_gloo import _free_port, _init


def _worker(rank, world, port, e_all, lp_all, k, shift, out):
    _init(rank, world, port)
    from fermiflow_amd import dist as D
    from tests import test_robust_hostsim as H
    B = len(e_all)
    off, cnt = D.shard(B)
    e, lp = e_all[off:off + cnt].copy(), lp_all[off:off + cnt].copy()
    counts = [D.shard(B, r, world)[1] for r in range(world)]
    marked = torch.from_numpy(np.where(np.isfinite(lp), e, np.nan))
    g = D.all_gather_padded(marked, maxlen=max(counts))
    g_asked = D.all_gather_padded(marked)                              # the ranks are asked for the longest shard
    assert g.shape == (world, max(counts)) and bits_equal(g.numpy(), g_asked.numpy())
    for r in range(world):                                             # NaN behind every shard's end, the shard in front of it
        assert np.isnan(g[r, counts[r]:].numpy()).all()
    gathered = torch.cat([g[r, :counts[r]] for r in range(world)]).numpy()
    stat = H.robust(gathered, None, k, shift)
    stat_padded = H.robust(g.reshape(-1).numpy(), None, k, shift)       # the padding left in: simply invalid walkers
    u, s, _, _, _ = H.apply(e, lp, stat, B, 0)
    st = torch.from_numpy(s.copy())
    D.all_reduce_sum_(st)
    out[rank] = (stat, u, float(st[0] / stat[R.NV]), stat_padded, gathered)
    dist.destroy_process_group()


def _run(world, B):
    from tests import test_robust_hostsim as H
    from tests.hostsim import simlib as S
    S.lib()      # build the host library once, here, not in every worker at the same time
    e, lp = R.spoil(*R.energies(B))
    k, shift = 2.0, 29.5
    marked = np.where(np.isfinite(lp), e, np.nan)
    one = H.robust(e, lp, k, shift)
    u_one, s_one, one2, _, _ = H.apply(e, lp, one, B, 1)
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), e, lp, k, shift, out), nprocs=world, join=True)
    from fermiflow_amd import dist as D
    for r in range(world):
        stat, u, value, stat_padded, gathered = out[r]
        off, cnt = D.shard(B, r, world)
        assert bits_equal(gathered, marked)
        assert bits_equal(stat[:R.VALUE], one[:R.VALUE]), (r, stat, one)                 # bit-identical to the single process
        assert bits_equal(u, u_one[off:off + cnt]), r
        assert bits_equal(stat, out[0][0]) and value == out[0][2]                       # ... and from rank to rank
        # the value: two (three) partial sums added instead of one tree
        _, _, sw, smag = R.weights(e, lp, R.clipped(e, lp, one[R.LO], one[R.HI], one[R.MED])[0], one[R.EC], B)
        assert abs(value - sw / one[R.NV]) <= R.FIN_TOL * smag / one[R.NV]
        assert abs(value - one2[R.VALUE]) <= 2 * R.FIN_TOL * smag / one[R.NV]
        # with the padding left in: the same integers and median; the sums within their bounds of the same reference
        assert stat_padded[R.NV] == one[R.NV] and stat_padded[R.NC] == one[R.NC] and bits_equal(stat_padded[R.MED], one[R.MED])
        want, scale = R.statistics(e, lp, k, shift)
        for i in (R.WIDTH, R.LO, R.HI, R.E, R.ESS):
            assert abs(stat_padded[i] - want[i]) <= R.FIN_TOL * scale[i], (i, stat_padded[i], want[i])


def test_two_ranks_uneven_shards_match_the_single_process_bit_for_bit():
    """1001 walkers: shards of 501 and 500, one NaN of padding behind the second"""
    _run(2, 1001)


def test_three_ranks_padding_inside_the_gathered_vector():
    """1099 walkers: shards of 367, 366, 366, a NaN behind the second INSIDE the gathered vector -- cut to the shard sizes it is the
    global batch again"""
    _run(3, 1099)
