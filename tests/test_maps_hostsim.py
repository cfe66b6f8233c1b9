"""ff_maps_accumulate (csrc/ff_maps.h) under the host simulator: the kernel source against a numpy restatement of the definitions in
include/fermiflow_maps.h.  CPU only; the two symbols are called through simlib.lib() with ctypes directly.  The simulator is built
without FMA contraction, so every comparison of counts is exact equality."""
import numpy as np
import pytest

from tests import maps_ref as R
from tests.hostsim import simlib as S

EXTENT = 6.0
SHAPES = [(1, 0), (0, 1), (1, 1), (2, 1), (3, 3), (12, 12)]


def walkers(seed, B, n, scale=1.3):
    return np.random.default_rng(seed).standard_normal((B, n, 2)) * scale


def run(x, nup, ndn, nbins, extent=EXTENT, acc=None):
    lib = S.lib()
    acc = R.new_buffer(lib, nbins) if acc is None else acc
    st = R.accumulate(lib, x, nup, ndn, extent, nbins, acc)
    assert st == 0, lib.ff_last_error()
    return acc


@pytest.mark.parametrize("nbins", [1, 2, 7, 128])
@pytest.mark.parametrize("nup,ndn", SHAPES, ids=[f"{a}+{b}" for a, b in SHAPES])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_every_slot_equals_numpy(B, nup, ndn, nbins):
    x = walkers(100 + 7 * nup + ndn, 257, nup + ndn)[:B]
    ref = R.histogram(x, nup, EXTENT, nbins)
    acc = run(x, nup, ndn, nbins)
    got = R.split(acc, nbins)
    assert np.array_equal(got["sum"], ref)
    assert (got["calls"], got["walkers"]) == (1, B)
    # conservation: every sample of every walker is in exactly one slot of its plane
    assert np.array_equal(got["sum"].sum(1), B * R.samples_per_walker(nup, ndn))
    if B == 65:
        run(x, nup, ndn, nbins, acc=acc)          # a second call doubles sum
        got = R.split(acc, nbins)
        assert np.array_equal(got["sum"], 2 * ref) and (got["calls"], got["walkers"]) == (2, 2 * B)


def test_workgroups_go_round_the_tile_loop_again():
    """More tiles of 256 walkers than the simulator's grid has slices (2 compute units: 8 workgroups over 5 planes with samples x 2 bands
    leave ONE slice): every workgroup takes five tiles, the last one ragged."""
    nup, ndn, nbins, B = 2, 1, 128, 1100
    x = walkers(9, B, nup + ndn)
    got = R.split(run(x, nup, ndn, nbins), nbins)
    assert np.array_equal(got["sum"], R.histogram(x, nup, EXTENT, nbins))
    assert (got["calls"], got["walkers"]) == (1, B)


def test_non_finite_coordinates_spoil_only_their_own_samples():
    nbins, nup, ndn = 12, 2, 1
    P = nbins * nbins + 2
    base = np.array([[0.5, 0.25], [1.0, -0.5], [-0.75, 2.0]])
    for bad in (np.nan, np.inf, -np.inf):
        for part in range(3):
            for coord in range(2):
                x = base[None].copy()
                x[0, part, coord] = bad
                h = R.split(run(x, nup, ndn, nbins), nbins)["sum"]
                assert np.array_equal(h, R.histogram(x, nup, EXTENT, nbins))
                inv = h[:, P - 1]
                # the particle's own lab sample, and the four ordered pairs it is part of (as reference or as partner)
                want = np.zeros(6, dtype=np.int64)
                want[0 if part < nup else 1] = 1
                if part < nup:
                    want[2], want[3], want[4] = 2, 1, 1          # uu both ways, ud as reference, du as partner
                else:
                    want[3], want[4] = 2, 2                      # partner of both ups, reference of both ups
                assert np.array_equal(inv, want), (bad, part, coord, inv)
                assert h[:, P - 2].sum() == 0 and h[:, :P - 2].sum() == 9 - want.sum()
    # finite coordinates whose rho overflows: the reference's pairs are invalid, its lab sample is an overflow sample
    x = base[None].copy()
    x[0, 0] = (1e200, 1e200)
    h = R.split(run(x, nup, ndn, nbins), nbins)["sum"]
    assert np.array_equal(h, R.histogram(x, nup, EXTENT, nbins))
    assert h[0, P - 2] == 1 and h[2, P - 1] == 1 and h[3, P - 1] == 1


def test_reference_particle_at_the_origin_takes_the_identity_rotation():
    nbins, L = 8, 4.0
    for origin in ([0.0, 0.0], [1e-170, -1e-170], [-0.0, 0.0]):          # rho == 0 as computed (the squares underflow)
        x = np.array([[origin, [1.5, -2.5]]])
        h = R.split(run(x, 1, 1, nbins, extent=L), nbins)["sum"]
        assert np.array_equal(h, R.histogram(x, 1, L, nbins))
        assert h[3, 5 * nbins + 1] == 1                                  # ud: the partner where it is, (1.5, -2.5) -> cell (5, 1)
        assert h[4, 4 * nbins + 4] == 1                                  # du: the origin stays the origin -> cell (4, 4)


def test_cell_edges_and_the_window_border():
    nbins, L = 8, 4.0                                                    # cells of width 1: edges at the integers
    x = np.array([[[-4.0, -4.0]], [[4.0, 0.0]], [[0.0, 4.0]], [[3.0, -1.0]], [[np.nextafter(4.0, 0.0), np.nextafter(-4.0, -5.0)]],
                  [[-0.0, 0.0]], [[-2.0 ** -50, 0.5]]])               # (4 - 2^-50 is a double: a is just below the edge at 4)
    h = R.split(run(x, 1, 0, nbins, extent=L), nbins)["sum"]
    assert np.array_equal(h, R.histogram(x, 1, L, nbins))
    P = nbins * nbins + 2
    assert h[0, 0] == 1                              # (-L, -L) is in the first cell
    assert h[0, P - 2] == 3                          # x = L, y = L, and y just below -L: outside [-L, L)
    assert h[0, 7 * nbins + 3] == 1                  # a point on two edges belongs to the cell above
    assert h[0, 4 * nbins + 4] == 1                  # -0.0 is 0
    assert h[0, 3 * nbins + 4] == 1                  # one ulp of a below the edge belongs to the cell below
    assert h[0, P - 1] == 0


def test_an_empty_call_is_a_no_op():
    lib = S.lib()
    acc = run(walkers(3, 10, 2), 1, 1, 4)
    before = acc.copy()
    assert R.accumulate(lib, np.zeros((0, 2, 2)), 1, 1, EXTENT, 4, acc) == 0
    assert R.accumulate(lib, np.zeros((0, 2, 2)), 1, 1, EXTENT, 4, acc, x_null=True) == 0
    assert np.array_equal(acc, before)


def test_refusals_write_nothing():
    lib = S.lib()
    nbins = 16
    acc = R.new_buffer(lib, nbins)
    acc[:] = 12345
    before = acc.copy()
    x6, x25 = walkers(1, 8, 6), walkers(1, 8, 25)
    cases = [
        (1, dict(x=x6, nup=3, ndn=3, x_null=True)),
        (1, dict(x=x6, nup=3, ndn=3, acc_null=True)),
        (1, dict(x=x6, nup=3, ndn=3, B=-1)),
        (1, dict(x=x6, nup=-1, ndn=7)),
        (1, dict(x=x6, nup=7, ndn=-1)),
        (1, dict(x=x6, nup=0, ndn=0)),
        (1, dict(x=x6, nup=3, ndn=3, nbins=0)),
        (1, dict(x=x6, nup=3, ndn=3, nbins=-4)),
        (1, dict(x=x6, nup=3, ndn=3, extent=0.0)),
        (1, dict(x=x6, nup=3, ndn=3, extent=-1.0)),
        (1, dict(x=x6, nup=3, ndn=3, extent=float("nan"))),
        (1, dict(x=x6, nup=3, ndn=3, extent=float("inf"))),
        (2, dict(x=x6, nup=3, ndn=3, nbins=129)),
        (2, dict(x=x25, nup=13, ndn=12)),
        (2, dict(x=x25, nup=25, ndn=0)),
    ]
    for status, kw in cases:
        kw = dict(dict(extent=EXTENT, nbins=nbins), **kw)
        st = R.accumulate(lib, kw["x"], kw["nup"], kw["ndn"], kw["extent"], kw["nbins"], acc, B=kw.get("B"), x_null=kw.get("x_null", False),
                          acc_null=kw.get("acc_null", False))
        assert st == status, (kw, st)
        assert lib.ff_last_error().decode().startswith("ff_maps:"), lib.ff_last_error()
        assert np.array_equal(acc, before)
    assert lib.ff_maps_buffer_bytes(0) == 0 and lib.ff_maps_buffer_bytes(129) == 0 and lib.ff_maps_buffer_bytes(-1) == 0
    assert lib.ff_maps_buffer_bytes(128) == 8 * (2 + 6 * (128 * 128 + 2))


def test_sign_convention_known_answer():
    """nup = ndn = 1, L = 4, 64 bins (cells of 1/8).  Particle 0 at radius 1.1 and a random angle phi, particle 1 at radius 1.7 and
    phi + 60 degrees.  In the frame of particle 0 the partner sits at 1.7 (cos 60, sin 60) = (0.85, 1.4722): a = 38.8, b = 43.78;
    in the frame of particle 1 the partner sits at 1.1 (cos 60, -sin 60) = (0.55, -0.9526): a = 36.4, b = 24.38.  Every value is at
    least 0.2 cell from an edge: no rounding reaches it."""
    B, L, nbins = 300, 4.0, 64
    phi = np.random.default_rng(60).uniform(0.0, 2.0 * np.pi, B)
    x = np.empty((B, 2, 2))
    x[:, 0, 0], x[:, 0, 1] = 1.1 * np.cos(phi), 1.1 * np.sin(phi)
    x[:, 1, 0], x[:, 1, 1] = 1.7 * np.cos(phi + np.pi / 3.0), 1.7 * np.sin(phi + np.pi / 3.0)
    h = R.split(run(x, 1, 1, nbins, extent=L), nbins)["sum"]
    assert h[3, 38 * nbins + 43] == B and h[3].sum() == B
    assert h[4, 36 * nbins + 24] == B and h[4].sum() == B
    assert h[2].sum() == 0 and h[5].sum() == 0 and h[0].sum() == B and h[1].sum() == B
