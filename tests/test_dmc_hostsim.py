"""ff_dmc_propose, ff_dmc_accept and ff_dmc_comb (csrc/ff_dmc.h) under the host simulator: the kernel sources against the numpy
restatement of include/fermiflow_dmc.h in tests/dmc_ref.py.  CPU only; the symbols are called through simlib.lib() with ctypes."""
import numpy as np
import pytest

from tests import dmc_ref as R
from tests.common import bits_equal
from tests.hostsim import simlib as S

SHAPES = [(1, 0), (2, 1), (12, 12)]           # n = 1 (one lone particle in the last quad), 3 (an odd tail), 24 (the limit)
IDS = [f"{a}+{b}" for a, b in SHAPES]
SIZES = (1, 255, 257, 513)                    # one lane, a ragged chunk, a second chunk of one walker, a ragged third
ACCEPT_SEED = 11                              # test_accept_*: the restatement's own min |u - p| is checked to exceed 1e-6 with it


# ---- propose
@pytest.mark.parametrize("a", [0.0, 1.0])
@pytest.mark.parametrize("nup,ndn", SHAPES, ids=IDS)
def test_propose_is_bit_exact_on_explicit_noise(nup, ndn, a):
    lib, n = S.lib(), nup + ndn
    rng = np.random.default_rng(100 + n)
    for B in SIZES:
        x, g, xi = rng.standard_normal((B, n, 2)), 3.0 * rng.standard_normal((B, n, 2)), rng.standard_normal((B, n, 2))
        g[0, 0] = 0.0                         # a vanishing drift
        xn, xo = R.call_propose(lib, x, g, 0.02, a, nup, ndn, noise=xi)
        ref = R.propose(x, g, xi, 0.02, a)
        assert bits_equal(xn, ref) and bits_equal(xo, xi), (B, np.abs(xn - ref).max())
        if a == 0.0:
            assert bits_equal(ref, (x + 0.02 * (0.5 * g)) + np.sqrt(0.02) * xi)      # the plain drift


@pytest.mark.parametrize("nup,ndn", SHAPES, ids=IDS)
def test_propose_philox_normals_are_reported_and_shard(nup, ndn):
    lib, n, B = S.lib(), nup + ndn, 257
    rng = np.random.default_rng(7)
    x, g = rng.standard_normal((B, n, 2)), rng.standard_normal((B, n, 2))
    xn, xi = R.call_propose(lib, x, g, 0.01, 1.0, nup, ndn, seed=12345, walker_offset=40, step=3)
    # the normals: finite, not the fill value, about standard, different from walker to walker and from step to step
    assert np.isfinite(xi).all() and abs(xi.mean()) < 5 / np.sqrt(xi.size) and abs(xi.std() - 1) < 0.1
    assert len(np.unique(xi)) > 0.99 * xi.size
    # xi_out is what a second call with noise = xi_out consumes
    again, _ = R.call_propose(lib, x, g, 0.01, 1.0, nup, ndn, noise=xi)
    assert bits_equal(xn, again) and bits_equal(xn, R.propose(x, g, xi, 0.01, 1.0))
    # two shards with their walker offsets are the whole batch; xi_out = NULL changes nothing
    h = 100
    a_, xa = R.call_propose(lib, x[:h], g[:h], 0.01, 1.0, nup, ndn, seed=12345, walker_offset=40, step=3)
    b_, xb = R.call_propose(lib, x[h:], g[h:], 0.01, 1.0, nup, ndn, seed=12345, walker_offset=40 + h, step=3, want_xi=False)
    assert bits_equal(np.concatenate([a_, b_]), xn) and bits_equal(xa, xi[:h]) and xb is None
    other, xs = R.call_propose(lib, x, g, 0.01, 1.0, nup, ndn, seed=12345, walker_offset=40, step=4)
    assert not (xs == xi).any()


# ---- accept
def check_accept(got_state, acc, rec, ref_state, info):
    assert np.array_equal(acc.astype(bool), info["acc"])
    for k in ("x", "logp", "grad", "eloc", "sign"):
        assert bits_equal(got_state[k], ref_state[k]), k
    np.testing.assert_allclose(got_state["w"], ref_state["w"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rec[:6], info["rec"][:6], rtol=1e-12, atol=0)
    assert rec[6:] == info["rec"][6:], (rec[6:], info["rec"][6:])


@pytest.mark.parametrize("a", [0.0, 1.0])
@pytest.mark.parametrize("nup,ndn", SHAPES, ids=IDS)
def test_accept_against_numpy(nup, ndn, a):
    lib, n, tau = S.lib(), nup + ndn, 0.02
    ctrl = [10.2, 10.0, 4.0]
    for B in SIZES:
        s, q, kinds = R.spoiled(ACCEPT_SEED + B, B, n)
        u = np.random.default_rng(ACCEPT_SEED).random(B)
        ref_state, info = R.accept(s, q, u, tau, a, ctrl)
        margin = np.abs(u - info["p"]).min()
        assert margin > 1e-6, (B, margin)             # the restatement's own margin: a rounding of q cannot flip a decision
        got, acc, rec, _ = R.call_accept(lib, s, q, tau, a, ctrl, nup, ndn, u=u)
        check_accept(got, acc, rec, ref_state, info)
        if kinds:
            assert not info["acc"][[kinds[k] for k in ("nan proposal", "zero sign", "flipped sign", "dead nan x", "dead inf eloc",
                                                        "nan grad proposal", "negative w", "inf logp proposal")]].any()
            assert info["acc"][kinds["above clip"]] and info["acc"][kinds["below clip"]]
            assert (got["w"][[5, 6, 10]] == 0.0).all() and rec[8] == 6 and rec[7] >= 2
            # beyond both clip bounds the weight moves by exactly the bound
            for b, edge in ((7, 14.0), (8, 6.0)):
                np.testing.assert_allclose(got["w"][b], s["w"][b] * np.exp(tau * (ctrl[0] - edge)), rtol=1e-12)
            assert np.isfinite(rec[:6]).all()


def test_accept_record_does_not_depend_on_the_grid_and_lands_in_its_slot():
    lib, nup, ndn, B, tau = S.lib(), 2, 1, 5 * R.CHUNK + 9, 0.02
    s, q, _ = R.spoiled(5, B, 3)
    u = np.random.default_rng(6).random(B)
    ctrl = [10.0, 10.0, 3.0]
    runs = [R.call_accept(lib, s, q, tau, 1.0, ctrl, nup, ndn, u=u, groups=g, slot=2, nslots=4) for g in (0, 1, 4)]
    ref_state, info = R.accept(s, q, u, tau, 1.0, ctrl)
    check_accept(runs[0][0], runs[0][1], runs[0][2], ref_state, info)
    for r in runs[1:]:
        assert bits_equal(r[3], runs[0][3]) and all(bits_equal(r[0][k], runs[0][0][k]) for k in r[0])
    trace = runs[0][3]
    assert (trace[:2 * R.REC] == -3.0).all() and (trace[3 * R.REC:] == -3.0).all()      # the other slots are untouched


def test_accept_philox_uniforms_are_the_counters_of_the_header():
    lib, nup, ndn, B, tau = S.lib(), 3, 3, 300, 0.02
    s, q, _ = R.spoiled(8, B, 6)
    ctrl = [10.0, 10.0, 3.0]
    seed, off, step = 0x1234567887654321, 1000, 17
    u = R.accept_uniforms(seed, B, step, off)
    assert ((u >= 0) & (u < 1)).all() and abs(u.mean() - 0.5) < 0.1
    ref_state, info = R.accept(s, q, u, tau, 1.0, ctrl)
    assert np.abs(u - info["p"]).min() > 1e-6
    got, acc, rec, _ = R.call_accept(lib, s, q, tau, 1.0, ctrl, nup, ndn, seed=seed, walker_offset=off, step=step)
    check_accept(got, acc, rec, ref_state, info)
    # two shards make the same decisions
    h = 111
    parts = [R.call_accept(lib, {k: v[sl] for k, v in s.items()}, {k: v[sl] for k, v in q.items()}, tau, 1.0, ctrl, nup, ndn, seed=seed,
                           walker_offset=off + o, step=step) for sl, o in ((slice(0, h), 0), (slice(h, B), h))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), acc)


# ---- comb
def check_comb(lib, state, nup, ndn, u0):
    src, out, info = R.call_comb(lib, state, nup, ndn, u0=u0)
    rs, distinct, copies, flag = R.comb(state["w"], u0)
    assert np.array_equal(src, rs) and list(info) == [distinct, copies, flag, 0], (list(info), distinct, copies, flag)
    for k in ("x", "logp", "grad", "eloc", "sign"):
        assert bits_equal(out[k], np.asarray(state[k])[rs]), k
    assert (out["w"] == 1.0).all()
    return src, info


@pytest.mark.parametrize("B", SIZES + (3 * R.CHUNK,))
def test_comb_against_numpy(B):
    lib, nup, ndn = S.lib(), 2, 1
    s, _ = R.random_state(40 + B, B, 3)
    rng = np.random.default_rng(B)
    for kind in ("random", "wide", "one", "holes", "equal"):
        w = rng.uniform(0.5, 1.5, B)
        if kind == "wide":
            w = np.exp(3.0 * rng.standard_normal(B))
        elif kind == "one":
            w = np.zeros(B); w[B // 2] = 3.0
        elif kind == "holes":
            w[rng.random(B) < 0.3] = 0.0
            w[rng.random(B) < 0.1] = np.nan
            w[rng.random(B) < 0.05] = -2.0
            w[B - 1] = np.inf                                  # (the last walker carries nothing: the clamp's case)
            w[0] = 1.0
        elif kind == "equal":
            w = np.ones(B)
        for u0 in (0.0, rng.random(), 1.0 - 2.0 ** -53):
            src, info = check_comb(lib, dict(s, w=w), nup, ndn, u0)
            assert (np.diff(src) >= 0).all()
            ws = R.cumulative(w)[0]
            assert (ws[src] > 0).all()
            if kind == "one":
                assert (src == B // 2).all() and list(info[:2]) == [1, B]
            if kind == "equal" and u0 < 0.5:
                assert np.array_equal(src, np.arange(B)) and list(info[:2]) == [B, 1]


def test_comb_total_weight_zero_sets_the_flag_and_philox_u0():
    lib, nup, ndn, B = S.lib(), 2, 1, 300
    s, _ = R.random_state(3, B, 3)
    for w in (np.zeros(B), np.full(B, np.nan), -np.ones(B), np.full(B, 1e308)):
        src, info = check_comb(lib, dict(s, w=w), nup, ndn, 0.3)
        assert np.array_equal(src, np.arange(B)) and list(info) == [B, 1, 1, 0]
    w = np.random.default_rng(1).uniform(0.2, 2.0, B)
    seed, step = 987654321987, 41
    u0 = R.comb_uniform(seed, step)
    assert 0.0 <= u0 < 1.0
    src, _, info = R.call_comb(lib, dict(s, w=w), nup, ndn, seed=seed, step=step)
    rs, distinct, copies, flag = R.comb(w, u0)
    assert np.array_equal(src, rs) and list(info) == [distinct, copies, flag, 0]
    assert not np.array_equal(rs, R.comb(w, R.comb_uniform(seed, step + 1))[0])


# ---- one full step with the flow
def test_one_full_step_at_the_synthetic_flow():
    """3 + 3, Z = 2 at the benchmark's synthetic weights, B = 64: propose, local energy and sign of the proposals, accept, comb -- the
    simulated kernels (ff_eloc_nd and ff_slater_sign included) against dmc_ref with the oracle's local energy and the restated sign.
    The accept mask is exact (the restatement's margin min |u - p| is asserted first); w to 1e-6 relative, the local-energy bar."""
    import torch
    import fermiflow_amd as ff
    from oracle import oracle as O
    from tests.obdm_ref import slater_sign
    nup = ndn = 3; B, Z, tau, a = 64, 2.0, 0.01, 1.0
    eta, mu = ff.MLP(1, 50), ff.MLP(1, 50)
    eta.init_gaussian(1); mu.init_gaussian(2)
    with torch.no_grad():
        for m in (eta, mu):
            m.fc2.weight *= 30.0
            m.fc1.weight *= 300.0
    wts = [tuple(t.detach().numpy().reshape(-1) for t in (m.fc1.weight, m.fc1.bias, m.fc2.weight)) for m in (eta, mu)]
    onet, snet = O.Net(*wts), S.Net(*wts, table=True)
    lib = S.lib()

    def oracle_guide(x):
        r = O.eloc(x, nup, ndn, onet, Z, rtol=1e-10, atol=1e-12)
        z = O.cnf_delta_logp(x, onet, t0=0.0, t1=1.0, rtol=1e-10, atol=1e-12)[0]
        return dict(logp=r["logp"], grad=r["grad"], eloc=r["eloc"], sign=slater_sign(z, nup, ndn)[0])

    def sim_guide(x):
        r = S.eloc_nd(x, nup, ndn, snet, Z)
        sign = np.empty(len(x))
        tu, td = S._tabs(nup, ndn, None, None)
        S._ck(lib.ff_slater_sign(None, len(x), nup, ndn, S._p(tu), S._p(td), None, S._p(r["z"]), S._p(sign)))
        return dict(logp=r["logp"], grad=r["grad"], eloc=r["eloc"], sign=sign)

    rng = np.random.default_rng(2)
    x0 = S.cnf_generate(S.mcmc(B, nup, ndn, 100, seed=5)[0], snet)[0]
    xi, u, u0 = rng.standard_normal(x0.shape), rng.random(B), rng.random()
    rs = dict(oracle_guide(x0), x=x0, w=np.ones(B))
    ctrl = [float(rs["eloc"].mean()), float(rs["eloc"].mean()), 0.2 * np.sqrt(6 / tau)]
    rx1 = R.propose(x0, rs["grad"], xi, tau, a)
    rnew, info = R.accept(rs, dict(oracle_guide(rx1), x=rx1), u, tau, a, ctrl)
    margin = np.abs(u - info["p"]).min()
    assert margin > 1e-4 and 0 < info["acc"].sum() and not info["dead"].any()
    rsrc = R.comb(rnew["w"], u0)[0]

    ss = dict(sim_guide(x0), x=x0, w=np.ones(B))
    x1, _ = R.call_propose(lib, x0, ss["grad"], tau, a, nup, ndn, noise=xi)
    np.testing.assert_allclose(x1, rx1, rtol=0, atol=1e-6 * tau)
    snew, acc, rec, _ = R.call_accept(lib, ss, dict(sim_guide(x1), x=x1), tau, a, ctrl, nup, ndn, u=u)
    assert np.array_equal(acc.astype(bool), info["acc"])
    np.testing.assert_allclose(snew["w"], rnew["w"], rtol=1e-6)
    np.testing.assert_allclose(rec[:5], info["rec"][:5], rtol=1e-5)
    assert rec[6:] == info["rec"][6:]
    src, out, cinfo = R.call_comb(lib, snew, nup, ndn, u0=u0)
    assert np.array_equal(src, R.comb(snew["w"], u0)[0]) and cinfo[2] == 0
    assert (src != rsrc).mean() < 0.1      # (the two weight vectors differ by 1e-6: a slot at a boundary may take the neighbour)
    print(f"full step: accepted {info['acc'].sum()} of {B}, margin {margin:.2e}, max |dw| / w {np.abs(snew['w'] / rnew['w'] - 1).max():.2e}")
