"""Cases of the Philox-fed samplers' ground dispatch (csrc/ff_mcmc.h: ff_mc_is_ground), shared by tests/test_gpu_sampler_ground.py
and its host-simulator twin tests/test_sampler_ground_hostsim.py.

A launch whose orbital tables are the list 0 .. NS-1 in order and that has no per-walker state evaluates the determinant of the
accept test with compile-time degrees; every other launch takes the run-time degrees.  Both must be the chain of the noise-fed
kernel on the materialised stream, bit for bit: walkers, log p and accept counts -- from the stream's own initial walkers
(ff_mcmc_sample), continued from given walkers (ff_mcmc_continue), and whatever batch a walker is in.

A backend provides, on numpy arrays (tables: int32 (states, NS) or None for an absent species; ws: int32 (B,) or None):
  rng_fill(B, n, steps, seed, offset) -> g0, g, u
  noise(nup, ndn, g0, g, u, tu, td, ws) -> x, logp, accept (steps, B)
  sample(B, nup, ndn, steps, seed, offset, tu, td, ws) -> x, logp, count
  cont(x0, nup, ndn, steps, seed, offset, tu, td, ws) -> x, logp, count
"""
import numpy as np

from tests.common import bits_equal, special_starts

STEPS = 20
BATCHES = (1, 7, 130)            # 130 walkers: two lanes per walker cross a 128-thread workgroup, the last workgroup is ragged
SPIN_SHAPES = [(ns, ns) for ns in range(1, 7)]
PAIR_SHAPES = [(ns, 0) for ns in range(2, 7)]      # the shapes launch_mcmc serves with ff_mcmc_pair_kernel<NS, false>
NONGROUND = ("up_last", "down_only", "permuted", "wstate_ground")


def ground_tables(nup, ndn):
    return (np.arange(nup, dtype=np.int32)[None], np.arange(ndn, dtype=np.int32)[None] if ndn else None)


def nonground_tables(kind, nup, ndn, B):
    """Tables one step away from the ground list, and the per-walker states that go with them (or None)."""
    tu, td = ground_tables(nup, ndn)
    tu = tu.copy(); td = None if td is None else td.copy()
    ws = None
    if kind == "up_last":
        tu[0, -1] += 1
    elif kind == "down_only":
        assert ndn, "one species has no down table"
        td[0, -1] += 1
    elif kind == "permuted":
        tu = np.roll(tu, 1, axis=1)
        if td is not None and ndn > 1:
            td = td[:, ::-1].copy()
        assert nup > 1, "a list of one orbital has no other order"
    elif kind == "wstate_ground":
        tu = np.repeat(tu, 3, axis=0)
        td = None if td is None else np.repeat(td, 3, axis=0)
        ws = (np.arange(B) % 3).astype(np.int32)
    else:
        raise ValueError(kind)
    return tu, td, ws


def nonground_cases(shapes):
    """(nup, ndn, kind) for every kind a shape has: one species has no down table, a list of one orbital has one order."""
    return [(nup, ndn, kind) for nup, ndn in shapes for kind in NONGROUND
            if not (kind == "down_only" and ndn == 0) and not (kind == "permuted" and nup == 1)]


def one_chain(K, nup, ndn, B, tu, td, ws, seed, offset):
    """Stream, noise-fed chain, Philox-fed chain and continued chain of B walkers: the three are one chain.  Returns it."""
    n = nup + ndn
    g0, g, u = K.rng_fill(B, n, STEPS, seed, offset)
    x1, lp1, a1 = K.noise(nup, ndn, g0, g, u, tu, td, ws)
    x2, lp2, c2 = K.sample(B, nup, ndn, STEPS, seed, offset, tu, td, ws)
    x3, lp3, c3 = K.cont(g0, nup, ndn, STEPS, seed, offset, tu, td, ws)
    cnt = a1.astype(np.int64).sum(0)
    assert bits_equal(x1, x2) and bits_equal(lp1, lp2) and np.array_equal(cnt, c2), (nup, ndn, B, "sample")
    assert bits_equal(x1, x3) and bits_equal(lp1, lp3) and np.array_equal(cnt, c3), (nup, ndn, B, "continue")
    assert np.isfinite(lp2).all()
    return x2, lp2, c2


def chain_case(K, nup, ndn, kind=None, batches=BATCHES):
    """kind None: the ground launch; else one of NONGROUND.  Every batch, and a walker's result whatever batch it is in."""
    seed, offset = 20260 + 16 * nup + ndn, 11
    out = {}
    for B in batches:
        tu, td, ws = ground_tables(nup, ndn) + (None,) if kind is None else nonground_tables(kind, nup, ndn, B)
        out[B] = one_chain(K, nup, ndn, B, tu, td, ws, seed, offset)
    big = max(batches)
    for B in batches:
        for a, b in zip(out[B], out[big]):
            assert bits_equal(a.astype(np.float64), b[:B].astype(np.float64)), (nup, ndn, kind, B, "batch")
    if kind == "wstate_ground":       # the same orbitals through the run-time degrees: the ground launch's walkers, bit for bit
        tu, td = ground_tables(nup, ndn)
        ref = K.sample(big, nup, ndn, STEPS, seed, offset, tu, td, None)
        for a, b in zip(out[big], ref):
            assert bits_equal(a.astype(np.float64), b.astype(np.float64)), (nup, ndn, "ground launch vs states")
    return out


def special_case(K, nup, ndn, B=35):
    """The special walkers of tests/test_gpu_sampler_edges.py (all particles at the origin, on an axis, far rings, a NaN coordinate,
    coincident particles) on a ground launch: continued chain == noise-fed chain on the stream, the NaN walker never moves, the
    walker at the origin (log p = -inf) accepts its first proposal."""
    n = nup + ndn
    seed, offset = 77 + nup, 5
    x0, _ = special_starts(nup, ndn, B, list(range(16)), seed=nup + ndn)
    tu, td = ground_tables(nup, ndn)
    _, g, u = K.rng_fill(B, n, STEPS, seed, offset)
    x1, lp1, a1 = K.noise(nup, ndn, x0, g, u, tu, td, None)
    x2, lp2, c2 = K.cont(x0, nup, ndn, STEPS, seed, offset, tu, td, None)
    assert bits_equal(x1, x2) and bits_equal(lp1, lp2) and np.array_equal(a1.astype(np.int64).sum(0), c2)
    assert a1[0, 0] == 1 and c2[0] >= 1                                      # origin: p = exp(+inf)
    assert c2[6] == 0 and np.isnan(lp2[6]) and bits_equal(x2[6], x0[6])      # NaN coordinate: never moves
    assert np.isfinite(lp2[16:]).all()
