"""world_size-2 CPU test (gloo) of EnergyParts.all_reduce_(), after tests/test_dist_gloo.py: two ranks hold the halves of one batch, run
the kernel's host build (tests/hostsim) on their own half, load the accumulator into an EnergyParts and all-reduce.  The counts must equal
one rank's on the whole batch; the sums agree within the restatement's rounding bounds of the three accumulations involved."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import energy_ref as R

NUP, NDN, D, Z, NS = 2, 1, 2, 2.0, 3
CENTRE = (5.0, 6.0, 2.0, 0.5, 1.5, 0.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _accumulated(inp, ws):
    """the simulated kernel on these walkers, its accumulator loaded into an EnergyParts on the host"""
    from fermiflow_amd import EnergyParts
    from tests.hostsim import simlib as S
    acc = R.new_buffer(S.lib(), NS)
    assert R.accumulate(S.lib(), **inp, nup=NUP, ndn=NDN, Z=Z, acc=acc, wstate=ws, nstates=NS, centre=np.array(CENTRE)) == 0
    obj = EnergyParts(NUP, NDN, Z, dim=D, nstates=NS, centre=CENTRE)
    st = obj.state_dict()
    st["acc"] = torch.from_numpy(acc.view(np.int64).copy())
    obj.load_state_dict(st)
    return obj


def _worker(rank, world, port, inp, ws, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    half = len(ws) // 2
    sl = slice(0, half) if rank == 0 else slice(half, None)
    obj = _accumulated({k: v[sl] for k, v in inp.items()}, ws[sl])
    obj.all_reduce_()
    out[rank] = obj.state_dict()["acc"].numpy().copy()
    dist.destroy_process_group()


def test_two_ranks_with_halves_equal_one_rank():
    from tests.hostsim import simlib as S
    S.lib()      # build the host library once, here, not in both workers at the same time
    B = 2 * R.CHUNK + 10          # equal halves: equal blocks
    inp = R.inputs(77, B, NUP, NDN, D)
    inp["x"][3, 0, 0] = np.nan                                         # an invalid walker on rank 0, one on rank 1
    inp["lap"][B - 2] = np.nan
    ws = R.states(3, B, NS)
    one = R.split(_accumulated(inp, ws).state_dict()["acc"].numpy().view(np.uint64), NS)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), inp, ws, out), nprocs=2, join=True)
    assert np.array_equal(out[0], out[1])                              # every rank holds the totals
    two = R.split(out[0].view(np.uint64), NS)
    assert (one["calls"], one["walkers"], one["invalid"]) == (1, B - 2, 2)
    assert (two["calls"], two["walkers"], two["invalid"], two["ticket"]) == (2, B - 2, 2, 0)      # one block per rank and call
    assert np.array_equal(two["count"], one["count"])
    half = B // 2
    refs = [R.reference(**{k: v[sl] for k, v in inp.items()}, nup=NUP, Z=Z, wstate=ws[sl], nstates=NS, centre=CENTRE)
            for sl in (slice(0, B), slice(0, half), slice(half, None))]
    worst = 0.0
    for name in ("sum", "sum2", "ssum", "sumE2"):
        # |two - one| <= the whole batch's bound + the halves' bounds + the one rounding of adding the halves
        bound = refs[0]["b_" + name] + refs[1]["b_" + name] + refs[2]["b_" + name] + R.LD(R.U) * (np.abs(refs[1][name]) + np.abs(refs[2][name]))
        err = np.abs(two[name].astype(R.LD) - one[name].astype(R.LD))
        assert (err <= bound).all(), name
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0).max()))
    # blocksq differs by construction: two blocks of half a batch each
    want = refs[1]["blocksq"] + refs[2]["blocksq"]
    bound = refs[1]["b_blocksq"] + refs[2]["b_blocksq"] + R.LD(R.U) * want
    assert (np.abs(two["blocksq"].astype(R.LD) - want) <= bound).all()
    print(f"largest |two ranks - one rank| / bound {worst:.3e}")
