"""ff_slater_sign and ff_obdm_accumulate (csrc/ff_obdm.h) under the host simulator: the kernel sources against the numpy restatement
of include/fermiflow_obdm.h in tests/obdm_ref.py.  CPU only; the symbols are called through simlib.lib() with ctypes directly."""
import numpy as np
import pytest

from tests import obdm_ref as R
from tests.hostsim import simlib as S

SHAPES = [(1, 0), (0, 1), (1, 1), (2, 1), (3, 3), (6, 5), (12, 12)]
IDS = [f"{a}+{b}" for a, b in SHAPES]
MARGIN, good_walkers = R.MARGIN, R.good_walkers


@pytest.mark.parametrize("nup,ndn", SHAPES, ids=IDS)
def test_sign_equals_numpy(nup, ndn):
    lib = S.lib()
    z = good_walkers(40 + 3 * nup + ndn, 257, nup, ndn)
    ref, margin = R.slater_sign(z, nup, ndn)
    assert (margin > MARGIN).all() and set(np.unique(ref)) <= {-1.0, 1.0}          # a property of the reference alone
    if max(nup, ndn) > 1:
        assert len(np.unique(ref)) == 2
    for B in (1, 63, 64, 65, 257):
        assert np.array_equal(R.sign_call(lib, z[:B], nup, ndn), ref[:B]), B


@pytest.mark.parametrize("nup,ndn", [(2, 1), (3, 3), (6, 5)], ids=["2+1", "3+3", "6+5"])
def test_sign_with_three_states(nup, ndn):
    lib = S.lib()
    rng = np.random.default_rng(9)
    tab_up = np.stack([np.sort(rng.choice(15, nup, replace=False)) for _ in range(3)])
    tab_dn = np.stack([np.sort(rng.choice(15, ndn, replace=False)) for _ in range(3)])
    tab_up[0], tab_dn[0] = np.arange(nup), np.arange(ndn)
    B = 130
    ws = np.sort(rng.integers(0, 3, B))
    assert set(ws) == {0, 1, 2}
    z = good_walkers(77, B, nup, ndn, tab_up, tab_dn, ws)
    ref, margin = R.slater_sign(z, nup, ndn, tab_up, tab_dn, ws)
    assert (margin > MARGIN).all()
    got = R.sign_call(lib, z, nup, ndn, tab_up, tab_dn, ws)
    assert np.array_equal(got, ref)
    # the state matters: the same walkers all in state 0 have other signs
    assert not np.array_equal(R.sign_call(lib, z, nup, ndn, tab_up, tab_dn, np.zeros(B, dtype=np.int32)), ref)


def test_sign_of_coincident_and_non_finite_walkers():
    lib = S.lib()
    z = good_walkers(5, 8, 3, 3)
    ref, _ = R.slater_sign(z, 3, 3)
    z[1, 2] = z[1, 0]                      # two up particles at one point
    z[2, 5] = z[2, 3]                      # two down particles
    z[3, 4] = z[3, 1]                      # an up and a down particle at one point: nothing special
    z[4, 1, 0] = np.nan
    z[5, 4, 1] = np.inf
    got = R.sign_call(lib, z, 3, 3)
    assert got[1] == 0.0 and got[2] == 0.0 and not np.signbit(got[1]) and not np.signbit(got[2])
    assert abs(got[3]) == 1.0
    assert np.isnan(got[4]) and np.isnan(got[5])
    assert np.array_equal(got[[0, 6, 7]], ref[[0, 6, 7]])
    for nup, ndn in ((12, 12), (6, 5)):   # the identity padding of the smaller species leaves an exact zero exact
        w = good_walkers(6, 4, nup, ndn)
        w[0, nup + 1] = w[0, nup]
        w[1, nup - 1] = w[1, 0]
        got = R.sign_call(lib, w, nup, ndn)
        assert got[0] == 0.0 and got[1] == 0.0 and abs(got[2]) == 1.0


def run(inp, nup, ndn, nshells, sigma=1.0, acc=None):
    lib = S.lib()
    acc = R.new_buffer(lib, nshells) if acc is None else acc
    st = R.accumulate(lib, **inp, sigma=sigma, nshells=nshells, nup=nup, ndn=ndn, acc=acc)
    assert st == 0, lib.ff_last_error()
    return acc


def check(acc, inp, nup, ndn, nshells, sigma=1.0, calls=1):
    B = inp["x"].shape[0]
    ref = R.estimate(**inp, sigma=sigma, nshells=nshells, nup=nup, ft=np.longdouble)
    delta = R.term_delta(**inp, sigma=sigma, nshells=nshells, nup=nup)
    got = R.split(acc, nshells)
    assert (got["calls"], got["walkers"], got["ticket"]) == (calls, calls * B, 0)
    assert np.array_equal(got["invalid"], calls * ref["invalid"])
    T = ref["T"].astype(np.float64)
    bound = R.bound(ref, delta)
    err = np.abs(got["sum"] - calls * T)
    print(f"B={B} nshells={nshells}: delta {delta:.3e}, max err {err.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert (err <= calls * bound).all()
    assert np.array_equal(got["sum"], got["sum"].transpose(0, 2, 1))          # symmetric bit for bit
    # sumsq: one block per call, T o T each
    assert (np.abs(got["sumsq"] - calls * T * T) <= calls * (2.0 * np.abs(T) * bound + bound * bound + 4.0 * R.EPS * T * T)).all()
    return got, ref


@pytest.mark.parametrize("nshells", [1, 2, 4, 8])
@pytest.mark.parametrize("nup,ndn", SHAPES, ids=IDS)
def test_accumulate_against_numpy(nup, ndn, nshells):
    full = R.inputs(200 + 5 * nup + ndn, 2 * R.CHUNK + 3, nup, ndn)
    for B in (1, 63, 64, 65, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 3):
        inp = {k: v[:B] for k, v in full.items()}
        acc = run(inp, nup, ndn, nshells)
        got, _ = check(acc, inp, nup, ndn, nshells)
        if B == 65:
            run(inp, nup, ndn, nshells, acc=acc)          # a second call doubles sum and sumsq
            two = R.split(acc, nshells)
            assert np.array_equal(two["sum"], 2.0 * got["sum"]) and np.array_equal(two["sumsq"], 2.0 * got["sumsq"])
            assert (two["calls"], two["walkers"]) == (2, 2 * B) and np.array_equal(two["invalid"], 2 * got["invalid"])


@pytest.mark.parametrize("sigma", [0.7, 1.4])
def test_another_width(sigma):
    inp = R.inputs(31, 100, 3, 3, sigma=sigma)
    check(run(inp, 3, 3, 4, sigma=sigma), inp, 3, 3, 4, sigma=sigma)


def test_more_chunks_than_workgroups():
    """The simulator has 2 compute units: a grid of 8 workgroups.  10 chunks (the last of 5 walkers): two workgroups go round again."""
    nup, ndn, nshells, B = 2, 1, 2, 9 * R.CHUNK + 5
    inp = R.inputs(17, B, nup, ndn)
    acc = run(inp, nup, ndn, nshells)
    check(acc, inp, nup, ndn, nshells)
    again = run(inp, nup, ndn, nshells)
    assert np.array_equal(acc, again)                     # bit for bit, run to run


def test_every_invalid_rule():
    nup, ndn, nshells, B = 2, 1, 2, 5
    base = R.inputs(3, B, nup, ndn)
    base["sign_moved"][:] = np.where(base["sign_moved"] == 0.0, 1.0, base["sign_moved"])
    clean = R.split(run(base, nup, ndn, nshells), nshells)
    assert not clean["invalid"].any()
    cases = [
        ("logp", (1,), np.nan, (2, 1)),                   # the walker's own log-density: every sample of the walker, both species
        ("sign", (1,), np.nan, (2, 1)),
        ("logp_moved", (2, 0), np.nan, (1, 0)),           # one moved walker: that sample only
        ("logp_moved", (0, 2), -np.inf, (0, 0)),          # q = 0: a valid zero
        ("sign_moved", (3, 1), 0.0, (0, 0)),              # likewise
        ("logp_moved", (1, 1), 5000.0, (1, 0)),           # exp overflows: q = inf
        ("logp", (4,), -np.inf, (2, 1)),                  # exp(+inf)
        ("rprime", (2, 1, 0), np.nan, (0, 1)),            # r' of one species: that species' samples of the walker
        ("rprime", (0, 0, 1), np.inf, (2, 0)),
        ("x", (3, 2, 1), np.nan, (0, 1)),                 # a coordinate of the particle itself
        ("x", (3, 0, 0), -np.inf, (1, 0)),
    ]
    for name, idx, value, want in cases:
        inp = {k: v.copy() for k, v in base.items()}
        inp[name][idx] = value
        got, ref = check(run(inp, nup, ndn, nshells), inp, nup, ndn, nshells)
        assert tuple(got["invalid"]) == want, (name, idx, value, got["invalid"])
        assert np.isfinite(got["sum"]).all() and np.isfinite(got["sumsq"]).all()
        if want == (0, 0):
            assert not np.array_equal(got["sum"], clean["sum"])          # the sample is there, with weight zero
    # sign' = 0 with an overflowing exponent is 0 x inf as computed: invalid
    inp = {k: v.copy() for k, v in base.items()}
    inp["sign_moved"][1, 0], inp["logp_moved"][1, 0] = 0.0, 5000.0
    got, _ = check(run(inp, nup, ndn, nshells), inp, nup, ndn, nshells)
    assert tuple(got["invalid"]) == (1, 0)
    # everything at once
    inp = {k: v.copy() for k, v in base.items()}
    for name, idx, value, _ in cases:
        inp[name][idx] = value
    check(run(inp, nup, ndn, nshells), inp, nup, ndn, nshells)


def test_far_walkers_have_zero_orbitals():
    """|r| > 38.6: the Gaussian factor is 0 as computed and the orbital is 0, whatever the polynomials overflow to"""
    inp = R.inputs(8, 3, 1, 1)
    inp["x"][0, 0] = (50.0, -3.0)
    inp["x"][1, 1] = (1e200, 1e200)
    got, ref = check(run(inp, 1, 1, 8), inp, 1, 1, 8)
    assert not got["invalid"].any() and np.isfinite(got["sum"]).all()


@pytest.mark.parametrize("nup,ndn", [(3, 0), (3, 3)], ids=["3+0", "3+3"])
def test_exact_identity_on_zero_flow(nup, ndn):
    """With z = x (no flow) and a single determinant, A_a = sum_i phi_a(x_i) q_i = phi_a(r') for an occupied orbital a -- the expansion
    of the determinant with row i replaced along that row.  So for occupied a and c, sum[a][c] = phi_a(r') phi_c(r') / g(r').
    ff_logprob, ff_slater_sign and ff_obdm_accumulate together, one walker per call."""
    lib = S.lib()
    n, nshells, sigma = nup + ndn, 3, 1.0
    rng = np.random.default_rng(100 + n)
    for walker in range(5):
        x = rng.standard_normal((1, n, 2))
        rp = rng.standard_normal((1, 2, 2)) * sigma
        xm = np.repeat(x, n, axis=0)
        for i in range(n):
            xm[i, i] = rp[0, 0 if i < nup else 1]
        logp, logpm = S.logprob(x, nup, ndn, derivs=False), S.logprob(xm, nup, ndn, derivs=False)
        sg, sgm = R.sign_call(lib, x, nup, ndn), R.sign_call(lib, xm, nup, ndn)
        inp = dict(x=x, rprime=rp, logp=logp, sign=sg, logp_moved=logpm[None], sign_moved=sgm[None])
        got = R.split(run(inp, nup, ndn, nshells, sigma=sigma), nshells)
        assert not got["invalid"].any()
        cond = R.condition(x[0], nup, ndn)
        for s, (lo, ns) in enumerate(((0, nup), (nup, ndn))):
            if not ns:
                assert not got["sum"][s].any()
                continue
            occ = range(ns)
            Phi = R.orbitals(occ, x[0, lo:lo + ns, 0], x[0, lo:lo + ns, 1])             # [particle, orbital]
            at_r = R.orbitals(occ, rp[0, s, 0], rp[0, s, 1])                             # phi_a(r')
            C = R.weights(rp[0, s][None], sigma, nshells)[0, :ns]
            q = np.array([np.linalg.det(np.vstack([Phi[:i], at_r[None], Phi[i + 1:]])) for i in range(ns)]) / np.linalg.det(Phi)
            mass = np.abs(Phi * q[:, None]).sum(0)                                       # sum_i |phi_a(x_i) q_i|
            bound = 64.0 * R.EPS * cond[s] * 0.5 * (np.outer(mass, np.abs(C)) + np.outer(np.abs(C), mass))
            want = 0.5 * (np.outer(at_r, C) + np.outer(C, at_r))
            numpy_own = 0.5 * (np.outer((Phi * q[:, None]).sum(0), C) + np.outer(C, (Phi * q[:, None]).sum(0)))
            assert (np.abs(numpy_own - want) <= bound).all()                             # the seed: numpy itself keeps the bound
            err = np.abs(got["sum"][s][:ns, :ns] - want)
            print(f"walker {walker} species {s}: cond {cond[s]:.1f}, max err / bound {(err / bound).max():.3e}")
            assert (err <= bound).all()


def test_an_empty_call_is_a_no_op():
    lib = S.lib()
    inp = R.inputs(2, 10, 1, 1)
    acc = run(inp, 1, 1, 2)
    before = acc.copy()
    empty = {k: v[:0] for k, v in inp.items()}
    assert R.accumulate(lib, **empty, sigma=1.0, nshells=2, nup=1, ndn=1, acc=acc) == 0
    assert R.accumulate(lib, **empty, sigma=1.0, nshells=2, nup=1, ndn=1, acc=acc, null=("x", "rprime", "logp", "sign", "logp_moved", "sign_moved", "workspace")) == 0
    assert np.array_equal(acc, before)
    out = np.full(3, 5.0)
    assert lib.ff_slater_sign(None, 0, 1, 1, None, None, None, None, None) == 1          # (the tables are checked first)
    tab = np.zeros(1, dtype=np.int32)
    assert lib.ff_slater_sign(None, 0, 1, 1, R._p(tab), R._p(tab), None, None, None) == 0
    assert (out == 5.0).all()


def test_refusals_write_nothing():
    lib = S.lib()
    nshells = 3
    acc = R.new_buffer(lib, nshells)
    acc[:] = 12345
    before = acc.copy()
    i6, i25, i13 = R.inputs(1, 8, 3, 3), R.inputs(1, 8, 13, 12), R.inputs(1, 8, 13, 0)
    cases = [(1, dict(null=(k,))) for k in ("x", "rprime", "logp", "sign", "logp_moved", "sign_moved", "acc", "workspace")]
    cases += [(1, dict(B=-1)), (1, dict(nup=-1, ndn=7)), (1, dict(nup=0, ndn=0)), (1, dict(nshells=0)), (1, dict(nshells=-3)),
              (1, dict(sigma=0.0)), (1, dict(sigma=-1.0)), (1, dict(sigma=float("nan"))), (1, dict(sigma=float("inf"))),
              (2, dict(nshells=9)), (2, dict(inp=i25, nup=13, ndn=12)), (2, dict(inp=i13, nup=13, ndn=0)), (2, dict(B=1 << 31))]
    for status, kw in cases:
        kw = dict(dict(inp=i6, nup=3, ndn=3, nshells=nshells, sigma=1.0, B=None, null=()), **kw)
        st = R.accumulate(lib, **kw["inp"], sigma=kw["sigma"], nshells=kw["nshells"], nup=kw["nup"], ndn=kw["ndn"], acc=acc, B=kw["B"],
                          null=kw["null"], ws=np.zeros(8))
        assert st == status, (kw["null"], kw["B"], kw["nup"], kw["nshells"], kw["sigma"], st)
        assert lib.ff_last_error().decode().startswith("ff_obdm:"), lib.ff_last_error()
        assert np.array_equal(acc, before)
    z, out, tab = np.zeros((4, 6, 2)), np.full(4, 5.0), np.arange(13, dtype=np.int32)
    for status, args in [(1, (4, 3, 3, R._p(tab), R._p(tab), None, None, R._p(out))), (1, (4, 3, 3, R._p(tab), R._p(tab), None, R._p(z), None)),
                         (1, (4, 3, 3, None, R._p(tab), None, R._p(z), R._p(out))), (1, (-1, 3, 3, R._p(tab), R._p(tab), None, R._p(z), R._p(out))),
                         (1, (4, 0, 0, R._p(tab), R._p(tab), None, R._p(z), R._p(out))), (2, (4, 13, 0, R._p(tab), None, None, R._p(z), R._p(out))),
                         (2, (4, 12, 13, R._p(tab), R._p(tab), None, R._p(z), R._p(out)))]:
        assert lib.ff_slater_sign(None, *args) == status, args[:3]
        assert lib.ff_last_error().decode().startswith("ff_obdm:")
    assert (out == 5.0).all()
    for ns in (0, 9, -1):
        assert lib.ff_obdm_buffer_bytes(ns) == 0 and lib.ff_obdm_workspace_bytes(100, ns) == 0
    assert lib.ff_obdm_buffer_bytes(8) == 8 * (5 + 4 * 36 * 36)
    assert lib.ff_obdm_workspace_bytes(-1, 4) == 0 and lib.ff_obdm_workspace_bytes(1 << 31, 4) == 0
    assert lib.ff_obdm_workspace_bytes(0, 4) == 8 * 200 and lib.ff_obdm_workspace_bytes(257, 4) == 8 * 200 * 2
