"""ff_observe_accumulate (csrc/ff_observe.h) under the host simulator: the kernel source against a numpy restatement of the
definitions in include/fermiflow.h.  CPU only; the two symbols are called through simlib.lib() with ctypes directly."""
import numpy as np
import pytest

from tests import observe_ref as R
from tests.hostsim import simlib as S

RMAX = 6.0
SHAPES = [(3, 3, 2), (1, 0, 2), (0, 2, 2), (4, 3, 2), (2, 2, 3), (10, 10, 3)]


def walkers(seed, B, n, d, scale=1.3):
    return np.random.default_rng(seed).standard_normal((B, n, d)) * scale


def run(x, nup, ndn, nbins, rmax=RMAX, acc=None):
    lib = S.lib()
    acc = R.new_buffer(lib, nbins) if acc is None else acc
    st = R.accumulate(lib, x, nup, ndn, rmax, nbins, acc)
    assert st == 0, lib.ff_last_error()
    return acc


@pytest.mark.parametrize("nbins", [1, 7, 240, 1024])
@pytest.mark.parametrize("nup,ndn,d", SHAPES, ids=[f"{a}+{b}_{d}d" for a, b, d in SHAPES])
def test_every_slot_equals_numpy(nup, ndn, d, nbins):
    B = 150
    x = walkers(100 + 7 * nup + ndn + d, B, nup + ndn, d)
    # the seeds are chosen so that no sample sits within 1e-9 of a bin edge (checked from numpy alone): the allowed deviation
    # 2 x (number of such samples) is zero and the comparison is exact equality
    assert R.edge_samples(x, nup, RMAX, nbins) == 0
    ref = R.histogram(x, nup, RMAX, nbins)
    got = R.split(run(x, nup, ndn, nbins), nbins)
    assert np.array_equal(got["sum"], ref)
    assert np.array_equal(got["sumsq"], ref ** 2)
    assert (got["calls"], got["walkers"]) == (1, B)
    assert not got["scratch"].any()
    # conservation: every sample of every walker is in exactly one slot of its class
    assert np.array_equal(got["sum"].sum(1), B * R.pair_counts(nup, ndn))


def test_special_walkers():
    nbins, nup, ndn = 12, 2, 1
    inf, nan = np.inf, np.nan
    x = np.array([
        [[0.0, 0.0], [1.0, 0.0], [0.0, 2.0]],          # a particle at the origin -> bin 0
        [[RMAX, 0.0], [0.0, 1e300], [1.0, 1.0]],       # r exactly rmax and r = 1e300 -> overflow
        [[nan, 0.5], [1.0, 0.0], [0.0, 2.0]],          # NaN coordinate: its radius and its two pairs invalid, the rest binned
        [[inf, 0.5], [1.0, 0.0], [0.0, 2.0]],          # inf coordinate: the same
        [[1.5, 0.5], [1.5, 0.5], [0.0, 2.0]],          # coincident up particles -> up-up bin 0
    ])
    got = R.split(run(x, nup, ndn, nbins), nbins)["sum"]
    assert np.array_equal(got, R.histogram(x, nup, RMAX, nbins))
    one = lambda w: R.split(run(x[w:w + 1], nup, ndn, nbins), nbins)["sum"]
    h = one(0)
    assert h[0, 0] == 1 and h[0, 2] == 1 and h[1, 4] == 1          # r = 0, 1, 2 at width 0.5
    h = one(1)
    assert h[0, nbins] == 2 and h[0, nbins + 1] == 0               # rmax and 1e300 are overflow samples, not invalid ones
    assert h[2, nbins] == 1 and h[3, nbins] == 1 and h[3, :nbins].sum() == 1
    for w in (2, 3):
        h = one(w)
        assert h[0, nbins + 1] == 1 and h[2, nbins + 1] == 1 and h[3, nbins + 1] == 1      # radius, up-up pair, its up-down pair
        assert h[0, 2] == 1 and h[1, 4] == 1 and h[3, :nbins].sum() == 1                    # everything else is still binned
        assert h[:, nbins + 1].sum() == 3
    h = one(4)
    assert h[2, 0] == 1


def test_three_calls_accumulate_sum_and_squares():
    nup, ndn, d, nbins, B = 3, 3, 2, 48, 130
    lib = S.lib()
    acc = R.new_buffer(lib, nbins)
    hs = []
    for k in range(3):
        x = walkers(20 + k, B, nup + ndn, d)
        hs.append(R.histogram(x, nup, RMAX, nbins))
        run(x, nup, ndn, nbins, acc=acc)
        assert not R.split(acc, nbins)["scratch"].any()          # every call leaves the scratch (and its ticket) zero
    got = R.split(acc, nbins)
    assert np.array_equal(got["sum"], sum(hs))
    assert np.array_equal(got["sumsq"], sum(h ** 2 for h in hs))
    assert (got["calls"], got["walkers"]) == (3, 3 * B)
    before = acc.copy()
    assert R.accumulate(lib, np.zeros((0, nup + ndn, d)), nup, ndn, RMAX, nbins, acc) == 0      # B = 0: a no-op
    assert np.array_equal(acc, before)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_any_batch_size_and_grid(B):
    """The grid derives from B (one wave per 64 walkers up to a cap the simulator's two compute units reach at 1000): the counts are
    those of numpy at every size, and the walkers of a large batch split over several calls give the same sum."""
    nup, ndn, d, nbins = 3, 3, 2, 240
    x = walkers(5, 1000, nup + ndn, d)[:B]
    assert R.edge_samples(x, nup, RMAX, nbins) == 0
    got = R.split(run(x, nup, ndn, nbins), nbins)
    assert np.array_equal(got["sum"], R.histogram(x, nup, RMAX, nbins))
    assert (got["calls"], got["walkers"]) == (1, B)
    if B == 1000:
        acc = R.new_buffer(S.lib(), nbins)
        for part in (x[:1], x[1:64], x[64:129], x[129:]):
            run(part, nup, ndn, nbins, acc=acc)
        assert np.array_equal(R.split(acc, nbins)["sum"], got["sum"])


@pytest.mark.parametrize("nup,ndn,d,nbins,B", [(3, 3, 2, 240, 2113), (10, 10, 3, 1024, 333), (4, 3, 2, 7, 2049)],
                         ids=["3+3_2d", "10+10_3d", "4+3_2d"])
def test_a_wave_goes_round_the_tile_loop_again(nup, ndn, d, nbins, B):
    """More tiles of 64 walkers than the simulator's grid has waves (2 compute units: at most 4 workgroups of 4 waves, of ONE wave at
    10 + 10 particles in 3-D where the staged rows leave room for no more): a wave stages a second and a third tile over the rows it has
    just read, with a ragged last tile.  Exact equality, as above."""
    x = walkers(300 + nup + d, B, nup + ndn, d)
    assert R.edge_samples(x, nup, RMAX, nbins) == 0
    ref = R.histogram(x, nup, RMAX, nbins)
    got = R.split(run(x, nup, ndn, nbins), nbins)
    assert np.array_equal(got["sum"], ref)
    assert np.array_equal(got["sumsq"], ref ** 2)
    assert (got["calls"], got["walkers"]) == (1, B)
    assert not got["scratch"].any()


def test_refusals_write_nothing():
    lib = S.lib()
    nbins = 16
    x = walkers(1, 8, 25, 4)
    acc = R.new_buffer(lib, nbins)
    acc[:] = 12345
    before = acc.copy()
    xs = x[:, :6, :2]
    cases = [
        (1, dict(x=xs, nup=3, ndn=3, x_null=True)),
        (1, dict(x=xs, nup=3, ndn=3, acc_null=True)),
        (1, dict(x=xs, nup=3, ndn=3, nbins=0)),
        (2, dict(x=xs, nup=3, ndn=3, nbins=1025)),
        (1, dict(x=xs, nup=3, ndn=3, rmax=0.0)),
        (1, dict(x=xs, nup=3, ndn=3, rmax=float("nan"))),
        (1, dict(x=xs, nup=3, ndn=3, rmax=float("inf"))),
        (2, dict(x=x[:, :6, :], nup=3, ndn=3)),                      # d = 4
        (2, dict(x=x[:, :, :2], nup=13, ndn=12)),                    # n = 25
        (2, dict(x=np.zeros((8, 21, 3)), nup=11, ndn=10)),           # n d = 63
    ]
    for status, kw in cases:
        kw = dict(dict(rmax=RMAX, nbins=nbins), **kw)
        st = R.accumulate(lib, kw["x"], kw["nup"], kw["ndn"], kw["rmax"], kw["nbins"], acc, x_null=kw.get("x_null", False),
                          acc_null=kw.get("acc_null", False))
        assert st == status, (kw, st)
        assert lib.ff_last_error().decode().startswith("ff_observe:"), lib.ff_last_error()
        assert np.array_equal(acc, before)
    assert lib.ff_observe_buffer_bytes(0) == 0 and lib.ff_observe_buffer_bytes(1025) == 0
