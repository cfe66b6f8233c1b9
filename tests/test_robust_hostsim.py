"""The robust estimator (csrc/ff_robust.h: ff_energy_robust, ff_energy_robust_apply) under the host simulator, against the definitions
restated in tests/robust_ref.py: the CPU twin of tests/test_gpu_robust.py (the same cases, tests/robust_cases.py, at sizes the simulator
runs in seconds).  The simulator's workgroups have 4 threads (hip_shim.h: FF_RBLOCK) -- a "wave" of four lanes for the ballots, longer
serial chains in the sums; the bounds are the device's all the same."""
import ctypes as C

import numpy as np
import pytest

from tests import robust_cases as cases
from tests import robust_ref as R
from tests.hostsim import simlib as S

HDR_WORDS = 8 + 2048      # ticket, selection state and histogram of the workspace: zero between calls


def workspace(N):
    return np.zeros(S.lib().ff_energy_robust_workspace_bytes(N) // 8)


def robust(e, logp, k, shift, ws=None):
    e = S._d(e); logp = None if logp is None else S._d(logp)
    ws = workspace(len(e)) if ws is None else ws
    stat = np.full(R.NSTAT, -7.0)
    S._ck(S.lib().ff_energy_robust(None, len(e), S._p(e), S._p(logp), float(k), S._p(np.array([shift], dtype=np.float64)), S._p(stat), S._p(ws)))
    assert not ws.view(np.uint64)[:HDR_WORDS].any()
    return stat


def apply(e, logp, stat, n_global, finish, z=None, g=None, ws=None):
    e, logp, stat = S._d(e), S._d(logp), np.array(stat, dtype=np.float64)
    ws = workspace(len(e)) if ws is None else ws
    u, s = np.full(len(e), -7.0), np.full(1, -7.0)
    n, d = (z.shape[1], z.shape[2]) if z is not None else (0, 0)
    z, g = (None, None) if z is None else (S._d(z).copy(), S._d(g).copy())
    S._ck(S.lib().ff_energy_robust_apply(None, len(e), n, d, S._p(e), S._p(logp), S._p(stat), int(n_global), int(finish), S._p(u), S._p(z), S._p(g),
                                         S._p(s), S._p(ws)))
    assert not ws.view(np.uint64)[:HDR_WORDS].any()
    return u, s, stat, z, g


class _Sim:
    robust = staticmethod(robust)
    apply = staticmethod(apply)


@pytest.mark.parametrize("B", [1, 2, 3, 255, 1024, 1025, 5000])
def test_sizes(B):
    """odd and even n_v, the segment boundary, five segments"""
    cases.sizes(_Sim, B)


@pytest.mark.parametrize("B", [1, 2, 1025])
def test_all_energies_equal(B):
    cases.all_equal(_Sim, B)


def test_heavy_ties_at_the_median():
    cases.heavy_ties(_Sim, 1025)


def test_signed_zeros_subnormals_and_last_bit_neighbours():
    cases.last_digit(_Sim, 1025)


def test_finite_outliers_are_valid():
    cases.finite_outliers(_Sim, 1025)


def test_every_walker_invalid():
    cases.every_walker_invalid(_Sim, 255)


def test_clip_a_third_and_nobody():
    cases.clip_widths(_Sim, 3001)


def test_padding_behind_the_batch_is_bit_identical():
    cases.padding(_Sim, 1000)


@pytest.mark.parametrize("n,d", [(1, 2), (6, 2), (20, 3)])
def test_apply_sanitises_invalid_rows_only(n, d):
    """M = 2, 12, 60"""
    cases.rows(_Sim, 300, n, d)


def test_one_workspace_serves_twenty_calls():
    """robust and apply share ONE workspace, call after call: bit-identical results, the header back at zero every time"""
    e, lp = R.spoil(*R.energies(2500))
    ws = workspace(2500)
    first = robust(e, lp, 5.0, 29.5, ws=ws)
    u1, s1, st1, _, _ = apply(e, lp, first, 2500, 1, ws=ws)
    for _ in range(20):
        stat = robust(e, lp, 5.0, 29.5, ws=ws)
        u, s, st, _, _ = apply(e, lp, stat, 2500, 1, ws=ws)
        assert cases.bits_equal(stat[:R.VALUE], first[:R.VALUE]) and cases.bits_equal(u, u1) and cases.bits_equal(s, s1) and cases.bits_equal(st, st1)


def test_dyadic_energies_are_exact():
    """e_b = 2.5 + k_b / 64 with sum k_b = 0, k = 1e6: every step is exact, u_b = e_b - 2.5 bit for bit"""
    e = R.dyadic(256)
    lp = np.linspace(-3.0, 3.0, 256)
    stat = robust(e, lp, 1e6, 0.0)
    u, _, _, _, _ = apply(e, lp, stat, 256, 1)
    assert stat[R.NV] == 256 and stat[R.NC] == 0 and stat[R.E] == 2.5 and stat[R.EC] == 2.5
    assert cases.bits_equal(u, e - 2.5)


def test_argument_errors_before_any_launch():
    lib = S.lib()
    p8 = C.c_void_p(8)
    assert lib.ff_energy_robust_workspace_bytes(1) == lib.ff_energy_robust_workspace_bytes(1024) == 8 * (HDR_WORDS + 4)
    assert lib.ff_energy_robust_workspace_bytes(1025) == 8 * (HDR_WORDS + 8)
    assert lib.ff_energy_robust_workspace_bytes(-1) == 0 and lib.ff_energy_robust_workspace_bytes(2**31) == 0
    for k in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ff_energy_robust(None, 4, p8, p8, k, p8, p8, p8) == 1
        assert lib.ff_last_error().decode().startswith("ff_energy_robust:")
    assert lib.ff_energy_robust(None, 0, p8, p8, 5.0, p8, p8, p8) == 1
    assert lib.ff_energy_robust(None, 4, None, p8, 5.0, p8, p8, p8) == 1
    assert lib.ff_energy_robust(None, 4, p8, p8, 5.0, p8, p8, None) == 1
    assert lib.ff_energy_robust(None, 2**31, p8, p8, 5.0, p8, p8, p8) == 2
    ok = (None, 4, 6, 2, p8, p8, p8, 4, 1, p8, p8, p8, p8, p8)

    def call(**kw):
        names = ("stream", "B", "n", "d", "e", "logp", "stat", "n_global", "finish", "u", "z", "g", "sum", "ws")
        return lib.ff_energy_robust_apply(*[kw.get(nm, v) for nm, v in zip(names, ok)])
    assert call(B=-1) == 1 and call(n_global=0) == 1 and call(logp=None) == 1 and call(g=None) == 1 and call(stat=None) == 1
    assert call(n=31) == 2 and call(n=0) == 2 and call(B=2**31) == 2
    assert lib.ff_last_error().decode().startswith("ff_energy_robust_apply:")
