"""ff_energy_parts_accumulate (csrc/ff_energy_parts.h) under the host simulator: the kernel sources against the numpy restatement of
include/fermiflow_energy.h in tests/energy_ref.py, and the statistical identities of the components on inputs whose law is known exactly.
CPU only; the symbol is called through simlib.lib() with ctypes directly.  Every test prints its largest error-to-bound ratio."""
import numpy as np
import pytest
import torch

from tests import energy_ref as R
from tests.hostsim import simlib as S

SHAPES = [(1, 0, 2), (2, 1, 2), (3, 3, 2), (2, 2, 3), (12, 12, 2)]
IDS = [f"{a}+{b}-{d}d" for a, b, d in SHAPES]
C_ = R.CHUNK
SIZES = (1, 63, 65, C_ - 1, C_, C_ + 1, 2 * C_ + 3)


def run(inp, nup, ndn, Z, acc=None, wstate=None, nstates=0, centre=None, want_parts=True):
    lib = S.lib()
    acc = R.new_buffer(lib, nstates) if acc is None else acc
    po = np.full((inp["x"].shape[0], R.K), 7.0) if want_parts else None
    st = R.accumulate(lib, **inp, nup=nup, ndn=ndn, Z=Z, acc=acc, wstate=wstate, nstates=nstates, centre=centre, parts_out=po)
    assert st == 0, lib.ff_last_error()
    return acc, po


def check(inp, nup, ndn, Z, wstate=None, nstates=0, centre=None):
    acc, po = run(inp, nup, ndn, Z, wstate=wstate, nstates=nstates, centre=centre)
    ref = R.reference(**inp, nup=nup, Z=Z, wstate=wstate, nstates=nstates, centre=centre)
    got = R.split(acc, nstates)
    worst = max(R.compare(got, ref, nstates), R.compare_parts(po, ref))
    return acc, po, got, ref, worst


@pytest.mark.parametrize("Z", [0.0, 2.0])
@pytest.mark.parametrize("nup,ndn,d", SHAPES, ids=IDS)
def test_accumulate_against_numpy(nup, ndn, d, Z):
    full = R.inputs(300 + 7 * nup + ndn + d, SIZES[-1], nup, ndn, d)
    worst = 0.0
    for B in SIZES:
        inp = {k: v[:B] for k, v in full.items()}
        acc, po, got, ref, w = check(inp, nup, ndn, Z)
        worst = max(worst, w)
        assert (got["walkers"], got["invalid"]) == (B, 0)
        if Z == 0.0:
            assert not po[:, 3:].any() and not got["sum"][3:].any() and not got["sum2"][3:].any() and not got["sum2"][:, 3:].any()
        else:
            pairs = (nup * (nup - 1) // 2, nup * ndn, ndn * (ndn - 1) // 2)
            assert [bool(po[:, 3 + k].any()) for k in range(3)] == [p > 0 for p in pairs]
        if B == 65:
            # a second call on the same buffer: one more block, every sum doubled exactly, the ticket back at zero
            run(inp, nup, ndn, Z, acc=acc)
            two = R.split(acc)
            assert (two["calls"], two["walkers"], two["invalid"], two["ticket"]) == (2, 2 * B, 0, 0)
            for name in ("sum", "sum2", "blocksq"):
                assert np.array_equal(two[name], 2.0 * got[name]), name
            worst = max(worst, R.compare(two, ref, calls=2))
    print(f"{nup}+{ndn} d={d} Z={Z}: largest error / bound {worst:.3e}")


def test_more_chunks_than_workgroups_and_two_runs_are_bitwise_equal():
    """The simulator has 2 compute units: a grid of 8 workgroups.  10 chunks (the last of 5 walkers): two workgroups go round again."""
    nup, ndn, d, B = 2, 1, 2, 9 * C_ + 5
    inp = R.inputs(17, B, nup, ndn, d)
    ws = R.states(5, B, 3)
    acc, po, got, ref, worst = check(inp, nup, ndn, 2.0, wstate=ws, nstates=3)
    again, po2 = run(inp, nup, ndn, 2.0, wstate=ws, nstates=3)
    assert np.array_equal(acc, again) and np.array_equal(po, po2)
    print(f"B={B}: largest error / bound {worst:.3e}")


@pytest.mark.parametrize("nstates", [1, 3])
def test_per_state_sums(nstates):
    """An empty middle state (of three) and a state boundary inside a chunk"""
    nup, ndn, d, B = 2, 1, 2, C_ + 40
    inp = R.inputs(23, B, nup, ndn, d)
    ws = R.states(9, B, nstates, empty=(1,) if nstates == 3 else ())
    if nstates == 3:
        edge = int(np.searchsorted(ws, 2))
        assert 0 < edge < B and edge % C_ != 0 and not (ws == 1).any()
    centre = np.array([1.0, 2.0, 3.0, 0.5, 1.5, 0.25])
    worst = 0.0
    for ctr in (None, centre):
        acc, po, got, ref, w = check(inp, nup, ndn, 2.0, wstate=ws, nstates=nstates, centre=ctr)
        worst = max(worst, w)
        assert got["count"].sum() == B and (nstates == 1 or got["count"][1] == 0)
        if nstates == 3:
            assert not got["ssum"][1].any() and got["sumE2"][1] == 0.0
        # the states' sums add up to the whole within their bounds
        assert (np.abs(got["ssum"].astype(R.LD).sum(0) - got["sum"].astype(R.LD)) <= ref["b_ssum"].sum(0) + ref["b_sum"]).all()
        # a second call doubles the per-state words too
        run(inp, nup, ndn, 2.0, acc=acc, wstate=ws, nstates=nstates, centre=ctr)
        two = R.split(acc, nstates)
        assert np.array_equal(two["count"], 2 * got["count"]) and np.array_equal(two["ssum"], 2.0 * got["ssum"]) and np.array_equal(two["sumE2"], 2.0 * got["sumE2"])
    print(f"nstates={nstates}: largest error / bound {worst:.3e}")


def test_every_invalid_rule():
    nup, ndn, d, B = 2, 2, 2, 70
    base = R.inputs(3, B, nup, ndn, d)
    ws = R.states(4, B, 3)
    clean = R.split(run(base, nup, ndn, 2.0, wstate=ws, nstates=3)[0], 3)
    assert clean["invalid"] == 0
    worst = 0.0

    def spoil(inp, ws, what):
        if what == "nan coordinate":
            inp["x"][5, 1, 0] = np.nan
        elif what == "inf coordinate":
            inp["x"][64, 3, 1] = np.inf
        elif what == "nan lap":
            inp["lap"][66] = np.nan
        elif what == "nan grad":
            inp["grad"][7, 0, 1] = np.nan
        elif what == "coincident uu":
            inp["x"][9, 1] = inp["x"][9, 0]
        elif what == "coincident ud":
            inp["x"][10, 2] = inp["x"][10, 0]
        elif what == "state above":
            ws[-1] = 3
        elif what == "state below":
            ws[0] = -1
    kinds = ("nan coordinate", "inf coordinate", "nan lap", "nan grad", "coincident uu", "coincident ud", "state above", "state below")
    for what in kinds + ("all",):
        inp, w = {k: v.copy() for k, v in base.items()}, ws.copy()
        for k in (kinds if what == "all" else (what,)):
            spoil(inp, w, k)
        for Z in (2.0, 0.0):
            acc, po, got, ref, r = check(inp, nup, ndn, Z, wstate=w, nstates=3)
            worst = max(worst, r)
            coincident = sum(k.startswith("coincident") for k in (kinds if what == "all" else (what,)))
            want = (len(kinds) if what == "all" else 1) - (coincident if Z == 0.0 else 0)       # a coincident pair is valid at Z = 0
            assert got["invalid"] == want and got["walkers"] == B - want, (what, Z, got["invalid"])
            assert got["count"].sum() == B - want
            # an invalid walker's row holds what was computed
            if what == "coincident uu" and Z != 0.0:
                assert np.isinf(po[9, 3]) and np.isfinite(po[9, [0, 1, 2, 4, 5]]).all()
            if what == "nan lap":
                assert np.isnan(po[66, 0]) and np.isfinite(po[66, 1:]).all()
            if what == "state above":
                assert np.isfinite(po[-1]).all()
    print(f"largest error / bound {worst:.3e}")


def test_parts_out_null_and_a_centre_change_nothing_they_should_not():
    nup, ndn, d, B = 3, 3, 2, C_ + 9
    inp = R.inputs(31, B, nup, ndn, d)
    with_parts, _ = run(inp, nup, ndn, 2.0)
    without, _ = run(inp, nup, ndn, 2.0, want_parts=False)
    assert np.array_equal(with_parts, without)
    # centre != 0 against centre = 0: the same means within the sum of the two bounds
    c0, m0 = R.parts(**inp, nup=nup, Z=2.0)
    centre = np.asarray(c0.mean(0), dtype=np.float64)
    acc_c, _, got_c, ref_c, w1 = check(inp, nup, ndn, 2.0, centre=centre)
    got_0, ref_0 = R.split(with_parts), R.reference(**inp, nup=nup, Z=2.0)
    lhs = got_c["sum"].astype(R.LD) + R.LD(B) * centre.astype(R.LD)
    assert (np.abs(lhs - got_0["sum"].astype(R.LD)) <= ref_c["b_sum"] + ref_0["b_sum"]).all()
    # about the centre the second moments are the covariance: far smaller than about zero, and so are their bounds
    # (the centre is the mean rounded to a double: what is left of the sums is B times that rounding, and the sums' own)
    assert (np.abs(got_c["sum"]) <= B * R.U * np.abs(centre) + ref_c["b_sum"].astype(np.float64)).all()
    assert ref_c["b_sum2"][2, 2] < ref_0["b_sum2"][2, 2]
    print(f"largest error / bound {w1:.3e}")


def test_an_empty_call_is_a_no_op_and_refusals_write_nothing():
    lib = S.lib()
    inp = R.inputs(2, 10, 1, 1, 2)
    acc, _ = run(inp, 1, 1, 2.0)
    before = acc.copy()
    empty = {k: v[:0] for k, v in inp.items()}
    assert R.accumulate(lib, **empty, nup=1, ndn=1, Z=2.0, acc=acc, d=2) == 0
    assert R.accumulate(lib, **empty, nup=1, ndn=1, Z=2.0, acc=acc, d=2, nstates=4, null=("x", "grad", "lap", "workspace")) == 0
    assert np.array_equal(acc, before)
    acc[:] = 12345
    before = acc.copy()
    i6, big = R.inputs(1, 8, 3, 3, 2), R.inputs(1, 8, 13, 12, 2)
    ws8 = np.zeros(8, dtype=np.int32)
    cases = [(1, dict(null=(k,))) for k in ("x", "grad", "lap", "acc", "workspace")]
    cases += [(1, dict(B=-1)), (1, dict(nup=-1, ndn=7)), (1, dict(nup=0, ndn=0)), (1, dict(d=0)), (1, dict(d=-2)), (1, dict(nstates=-1)),
              (1, dict(nstates=2)), (1, dict(Z=float("nan"))), (1, dict(Z=float("inf"))), (1, dict(Z=-float("inf"))),
              (2, dict(d=1)), (2, dict(d=4)), (2, dict(inp=big, nup=13, ndn=12)), (2, dict(inp=R.inputs(1, 8, 11, 10, 3), nup=11, ndn=10)),
              (2, dict(B=1 << 31)), (2, dict(nstates=R.MAX_STATES + 1, wstate=ws8))]
    for status, kw in cases:
        kw = dict(dict(inp=i6, nup=3, ndn=3, d=None, Z=2.0, B=None, null=(), nstates=0, wstate=None), **kw)
        st = R.accumulate(lib, **kw["inp"], nup=kw["nup"], ndn=kw["ndn"], Z=kw["Z"], acc=acc, wstate=kw["wstate"], nstates=kw["nstates"], B=kw["B"],
                          d=kw["d"], null=kw["null"], ws=np.zeros(64))
        assert st == status, (kw["null"], kw["B"], kw["nup"], kw["d"], kw["Z"], kw["nstates"], st)
        assert lib.ff_last_error().decode().startswith("ff_energy_parts:"), lib.ff_last_error()
        assert np.array_equal(acc, before)
    assert lib.ff_energy_parts_buffer_bytes(0) == 8 * 52 and lib.ff_energy_parts_buffer_bytes(3) == 8 * (52 + 24)
    assert lib.ff_energy_parts_buffer_bytes(-1) == 0 and lib.ff_energy_parts_buffer_bytes(R.MAX_STATES + 1) == 0
    assert lib.ff_energy_parts_buffer_bytes(R.MAX_STATES) == 8 * (52 + 8 * R.MAX_STATES)
    assert lib.ff_energy_parts_workspace_bytes(0, 0) == 8 * 28 and lib.ff_energy_parts_workspace_bytes(257, 0) == 8 * 28 * 2
    assert lib.ff_energy_parts_workspace_bytes(257, 3) == 8 * (28 * 2 + 6 * 257)
    assert lib.ff_energy_parts_workspace_bytes(-1, 0) == 0 and lib.ff_energy_parts_workspace_bytes(1 << 31, 0) == 0 and lib.ff_energy_parts_workspace_bytes(8, -1) == 0


def _loaded(acc, d):
    """the accumulator of the simulated kernel in an EnergyParts on the host: its means() and errors() are what a user reads"""
    from fermiflow_amd import EnergyParts
    obj = EnergyParts(1, 0, 0.0, dim=d)
    st = obj.state_dict()
    st["acc"] = torch.from_numpy(acc.view(np.int64).copy())
    obj.load_state_dict(st)
    return obj


@pytest.mark.parametrize("d", [2, 3])
def test_statistical_identities_of_the_trap_ground_state(d):
    """One particle, x ~ N(0, I / 2), grad = -2 x, lap = -2 d (energy_ref.gaussian_inputs; the seed was chosen once): E = d / 2 for every
    walker within the rounding bound; <T_L>, <T_G> and <V_trap> within 5 of their own reported errors of d / 4; the virial and dT
    within 5 of theirs of 0.  The restatement meets the same 5 sigma first: that is a property of the inputs alone."""
    B = 4096
    inp = R.gaussian_inputs(B, d)
    ref = R.reference(**inp, nup=1, Z=0.0)
    want = {"T_L": d / 4, "T_G": d / 4, "V_trap": d / 4, "virial": 0.0, "dT": 0.0}
    mean, err = R.statistics(ref)
    for name, v in want.items():
        assert err[name] > 0.0 and abs(mean[name] - v) <= 5.0 * err[name], ("restatement", name, mean[name], err[name])
    acc, po, got, _, worst = check(inp, 1, 0, 0.0)
    assert (got["walkers"], got["invalid"]) == (B, 0)
    # E = T_L + V_trap per walker: the two components' bounds and the rounding of this sum
    e = po[:, 0] + po[:, 2]
    b = (ref["b_parts"][:, 0] + ref["b_parts"][:, 2]).astype(np.float64) + R.U * (np.abs(po[:, 0]) + np.abs(po[:, 2]))
    assert (np.abs(e - d / 2) <= b).all()
    obj = _loaded(acc, d)
    m, s = obj.means(), obj.errors()
    for name, v in want.items():
        assert s[name] > 0.0 and abs(m[name] - v) <= 5.0 * s[name], (name, m[name], s[name])
    # the class's means against the restatement's: the bounds of the sums it divides, and the 13 roundings of its own arithmetic (the
    # division, the centre, six products and five additions) on the magnitudes it combines
    comp = np.array([mean[k] for k in R.NAMES])
    for name, a in {**{k: np.eye(R.K)[i] for i, k in enumerate(R.NAMES)}, **R.DERIVED}.items():
        a = np.abs(np.asarray(a, dtype=np.float64))
        tol = float(a @ ref["b_sum"].astype(np.float64)) / B + 13 * R.U * float(a @ np.abs(comp))
        assert abs(m[name] - mean[name]) <= tol, (name, m[name], mean[name], tol)
    assert m["V_ee"] == 0.0 and s["V_ee"] == 0.0
    print(f"d={d}: E = {m['E']!r} +- {s['E']:.3e}")
    print(f"d={d}: largest error / bound {worst:.3e}; " + ", ".join(f"{k} {(m[k] - v) / s[k]:+.2f} sigma" for k, v in want.items()))
