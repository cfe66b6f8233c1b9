"""Cases of the ODE kernels at time spans other than (0, 1), shared by tests/test_gpu_spans.py and its host-simulator
twin tests/test_spans_hostsim.py.

Every ODE entry point takes (t0, t1), and the kernels carry the direction and the length of the interval explicitly: ff_stepper::dir
and ::interval, the clip of the last step to tb, ff_open_step's equal steps of |tb - ta|, the clamp fmin(hwarm, interval) of a warm
start.  A sign on h, a 1.0 where the interval is meant or a clamp against the wrong bound is invisible at (0, 1).

Two references per case.  The first is always the oracle called with the span itself.  The second is the autonomous-field identity:
the velocity field does not depend on t and is linear in the fc2 weights, so the flow over (a, b) with weights theta is the flow over
(0, 1) with both fc2 weight vectors multiplied by s = b - a (s < 0: the reversed span); d / d fc2.weight over (a, b) is s times the
scaled model's gradient and every other parameter gradient is equal.  The two sides are not bit-identical (t + h rounds differently):
compared at the bars.

Solves and bars are those of tests/test_gpu_geometry.py, unchanged.  The spans are up to twice as long as the one those bars were
set at, so every reference asserts, on the oracle alone, that its own result at the kernels' tolerances stays within half of each bar
of its result at the oracle's tolerances (the practice of tests/eloc_states_cases.py).  Walkers: seeded standard_normal * 1.2; batches
of 2 G + 3 walkers (G walkers per wave of the call's kernel: a wave ends on a partly filled group), 3 for the wide family; the oracle
on the first min(B, G + 1).  No walker is excluded from a comparison.

Worst errors measured on an MI355X over all spans, shapes and both radial modes (235 device cases; docs/LOG.md has the full list):
  flow x / z / dlogp (absolute)            3.7e-10 / 1.2e-10 / 4.9e-10, round trip 8.8e-10, identity 4.4e-11     bar 1e-8
  E_loc, lap (relative per walker)         2.2e-9, 7.7e-11; identity 9.1e-11, 2.1e-10                            bar 3e-8
  grad, glogp0 (relative to the largest)   4.1e-11, 2.3e-11; identity 1.1e-10                                    bar 5e-9
  adjoint gx, gp (relative to the largest) 1.3e-10, 4.5e-10; identity 4.7e-11                                    bar 5e-8
  autograd through generate / delta_logp   d/dtheta 7.7e-10 / 5.2e-10 (oracle), 8.5e-10 / 5.3e-10 (RK4)          bar 5e-8
  GSVMC sweeps                             x 7.2e-11, E_loc 6.6e-10, E 1.2e-10, theta-gradient 9.3e-10           bars as above
  empty interval                           E_loc / sum of orbital energies - 1: 1.6e-15                          bar 1e-10

A backend K provides, on numpy arrays (h: a handle of K.net; warm: h_init, h_scale, uniform, equal, max_steps):
  plan(call, n, d) -> (family, walkers per group) of native.PLAN_CALLS[call]
  net(s, table) -> handle of weights(golden, s) with the radial table or direct evaluation
  generate(h, z, t0, t1, order=None, **warm) -> x, walker_cost, walker_h_out, stats
  delta_logp(h, x, t0, t1) -> z, dlogp, stats
  eloc(h, x, nup, ndn, Z, t0, t1, **warm) -> dict(eloc, grad, lap, logp, z, dlogp, glogp0, stats, hout)   (64-bit sensitivities)
  adjoint(h, y, a_z, a_d, t0, t1, **warm) -> gx, gp, stats
  gp_reproducible: two identical adjoint launches return the same gp bit for bit
"""
import numpy as np

from oracle import oracle as O
from tests.common import bits_equal, net_arrays
from tests.test_gpu_geometry import AT, BAR_ELOC, BAR_FLOW, BAR_GP, BAR_GRAD, OAT, ORT, RT      # noqa: F401  (shared, unchanged)

SPANS = [(0.25, 1.75), (1.0, 0.0), (2.0, 0.5), (0.1, 0.7)]
CONTROL = (0.0, 1.0)
ALL_SPANS = SPANS + [CONTROL]
DYADIC = SPANS[:3]                 # t0 a dyadic number: t0 +- 2^-20 is exact
EMPTY = (0.5, 0.5)
SLOT_SPANS = [(1.0, 0.0), (0.25, 1.75)]

FLOW_SHAPES = [(3, 2), (6, 2), (2, 3), (13, 2), (5, 3)]            # narrow kernels at G = 10, 5, 10; the wide family in 2-D and 3-D
ELOC_SHAPES = [(2, 1, 2), (3, 3, 2), (4, 3, 2), (4, 4, 2), (1, 1, 3), (7, 6, 2)]   # columns, mfma, rows, split, 3-D rows, wide
ADJ_SHAPES = [(6, 2, True), (6, 2, False), (2, 3, True), (13, 2, True)]           # tabulated, direct, 3-D, wide
NARROW_FLOW = FLOW_SHAPES[:3]
Z_COULOMB = 1.0
H0 = 2.0 ** -20
H_UNITS = 50                       # hidden units of both nets of the benchmark's flow

WORST = {}                         # quantity -> worst error seen in this process (printed by report())


def sid(span):
    return f"{span[0]:g}-{span[1]:g}"


def weights(golden, s=1.0, use_mu=True):
    """(eta, mu) of the benchmark's flow with both fc2 weight vectors multiplied by s (use_mu = False: no one-body net, mu = None)"""
    eta, mu = net_arrays(golden["g5_gsvmc"], "z2_nt_")
    return (eta[0], eta[1], eta[2] * s), ((mu[0], mu[1], mu[2] * s) if use_mu else None)


def onet(golden, s=1.0, use_mu=True):
    return O.Net(*weights(golden, s, use_mu))


def walkers(n, d, B):
    return np.random.default_rng(1000 * n + d).standard_normal((B, n, d)) * 1.2


def batch(K, call, n, d):
    fam, G = K.plan(call, n, d)
    B = 3 if fam == "wide" else 2 * G + 3
    return fam, G, B, min(B, G + 1)


def rel_max(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def note(**errs):
    for k, v in errs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)


def report(path):
    print(f"SPANS MAX {path}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def scale_gp(gp, s):
    """the gradient over (a, b) from the gradient of the model over (0, 1) with fc2 scaled by s: d / d fc2.weight times s"""
    g = np.array(gp, dtype=np.float64).reshape(-1, 3, H_UNITS)      # [eta(, mu)][w1, b1, w2][H]
    g[:, 2] *= s
    return g.reshape(-1)


# ---- references: the oracle with the span itself, computed once per case; conditioning is decided by the oracle alone -----------------
_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _half(name, own, bar, what):
    assert own < bar / 2, (f"{what}: the oracle's own truncation error in {name} at the kernels' tolerances is {own:.2e}, beyond half of "
                           f"the bar {bar:.0e}: tighten this case's solve or choose another seed")


def ref_generate(golden, z, span):
    def make():
        net = onet(golden)
        x, _ = O.cnf_generate(z, net, span[0], span[1], ORT, OAT)
        own, _ = O.cnf_generate(z, net, span[0], span[1], RT, AT)
        _half("x", float(np.abs(own - x).max()), BAR_FLOW, ("generate", z.shape, span))
        return x
    return _cached(("gen", z.tobytes(), span), make)


def ref_delta_logp(golden, x, span, check=True):
    def make():
        net = onet(golden)
        z, dl, _ = O.cnf_delta_logp(x, net, span[0], span[1], ORT, OAT)
        if check:
            zo, dlo, _ = O.cnf_delta_logp(x, net, span[0], span[1], RT, AT)
            _half("z", float(np.abs(zo - z).max()), BAR_FLOW, ("delta_logp", x.shape, span))
            _half("dlogp", float(np.abs(dlo - dl).max()), BAR_FLOW, ("delta_logp", x.shape, span))
        return z, dl
    return _cached(("dl", x.tobytes(), span, check), make)


def eloc_errors(g, ref):
    """the figures of tests/test_gpu_geometry.py's local-energy check"""
    return dict(eloc=float((np.abs(g["eloc"] - ref["eloc"]) / np.abs(ref["eloc"])).max()),
                lap=float((np.abs(g["lap"] - ref["lap"]) / np.maximum(np.abs(ref["lap"]), 1.0)).max()),
                grad=rel_max(g["grad"], ref["grad"]), glogp0=rel_max(g["glogp0"], ref["glogp0"]),
                logp=float(np.abs(g["logp"] - ref["logp"]).max()),
                z=float(np.abs(g["z"] - ref["z"]).max()), dlogp=float(np.abs(g["dlogp"] - ref["dlogp"]).max()))


ELOC_BARS = dict(eloc=BAR_ELOC, lap=BAR_ELOC, grad=BAR_GRAD, glogp0=BAR_GRAD, logp=BAR_FLOW, z=BAR_FLOW, dlogp=BAR_FLOW)


def _oracle_eloc(golden, x, nup, ndn, span, Z, rtol, atol, tab_up=None, wstate=None):
    d = x.shape[2]
    net = onet(golden)
    kw = dict(tab_up=tab_up, wstate=wstate) if tab_up is not None else {}
    ref = dict((O.eloc if d == 2 else O.eloc3d)(x, nup, ndn, net, Z, t0=span[0], t1=span[1], rtol=rtol, atol=atol, **kw))
    ref["z"], ref["dlogp"], _ = O.cnf_delta_logp(x, net, span[0], span[1], rtol, atol)
    ref["glogp0"] = (O.logprob if d == 2 else O.logprob3d)(ref["z"], nup, ndn, **kw)[1]
    return ref


def ref_eloc(golden, x, nup, ndn, span, Z=Z_COULOMB, tab_up=None, wstate=None):
    def make():
        ref = _oracle_eloc(golden, x, nup, ndn, span, Z, ORT, OAT, tab_up, wstate)
        own = eloc_errors(_oracle_eloc(golden, x, nup, ndn, span, Z, RT, AT, tab_up, wstate), ref)
        for k, v in own.items():
            _half(k, v, ELOC_BARS[k], ("eloc", nup, ndn, x.shape, span))
        return ref
    return _cached(("eloc", x.tobytes(), nup, ndn, span, Z, None if wstate is None else np.asarray(wstate).tobytes()), make)


def ref_adjoint(golden, y, a_z, a_d, span, use_mu=True):
    def make():
        net = onet(golden, 1.0, use_mu)
        gx, gp, _ = O.cnf_adjoint(y, np.zeros(len(y)), a_z, a_d, net, span[0], span[1], ORT, OAT)
        gxo, gpo, _ = O.cnf_adjoint(y, np.zeros(len(y)), a_z, a_d, net, span[0], span[1], RT, AT)
        _half("gx", rel_max(gxo, gx), BAR_GP, ("adjoint", y.shape, span))
        _half("gp", rel_max(gpo, gp), BAR_GP, ("adjoint", y.shape, span))
        return gx, gp
    return _cached(("adj", y.tobytes(), a_z.tobytes(), a_d.tobytes(), span, use_mu), make)


def seeds(n, d, B):
    rng = np.random.default_rng(77 + 10 * n + d)
    return rng.standard_normal((B, n, d)) / B, rng.standard_normal(B) / B


# ---- 1. plain solves against the oracle and the identity --------------------------------------------------------------------------
def flow_case(K, golden, n, d, table, span):
    """cnf_generate and cnf_delta_logp over the span against the oracle, against the scaled model over (0, 1), and the round trip"""
    fam, G, B, S = batch(K, "flow" if table else "flow_fb", n, d)
    a, b = span
    net, unit = K.net(1.0, table), K.net(b - a, table)
    z = walkers(n, d, B)
    x, cost, hout, st = K.generate(net, z, a, b)
    assert st[3] == 0 and np.isfinite(x).all() and (cost >= 0).all(), st[:4]
    assert (hout > 0).all() and (hout <= abs(b - a)).all(), hout
    e_x = float(np.abs(x[:S] - ref_generate(golden, z[:S], span)).max())
    x1, _, _, s1 = K.generate(unit, z, 0.0, 1.0)
    assert s1[3] == 0
    i_x = float(np.abs(x - x1).max())
    zb, dl, st = K.delta_logp(net, x, a, b)
    assert st[3] == 0
    ref_delta_logp(golden, ref_generate(golden, z[:S], span), span)      # (conditioning: on the oracle's own x)
    zo, dlo = ref_delta_logp(golden, x[:S], span, check=False)
    e_z, e_d = float(np.abs(zb[:S] - zo).max()), float(np.abs(dl[:S] - dlo).max())
    z1, d1, s1 = K.delta_logp(unit, x, 0.0, 1.0)
    assert s1[3] == 0
    i_z, i_d = float(np.abs(zb - z1).max()), float(np.abs(dl - d1).max())
    back = float(np.abs(zb - z).max())
    print(f"SPANS flow {n}x{d} {fam} table={table} {sid(span)} B={B}: oracle x {e_x:.2e} z {e_z:.2e} dlogp {e_d:.2e}; identity x {i_x:.2e} "
          f"z {i_z:.2e} dlogp {i_d:.2e}; round trip {back:.2e} (bar {BAR_FLOW:.0e})")
    note(flow_x=e_x, flow_z=e_z, flow_dlogp=e_d, identity_flow=max(i_x, i_z, i_d), round_trip=back)
    assert max(e_x, e_z, e_d) < BAR_FLOW, (e_x, e_z, e_d)
    assert max(i_x, i_z, i_d) < BAR_FLOW, (i_x, i_z, i_d)
    # x is within the bar of the exact flow of z, zb within the bar of the exact preimage of x: the round trip is held to the same bar
    assert back < BAR_FLOW, back


def eloc_case(K, golden, nup, ndn, d, table, span):
    n = nup + ndn
    fam, G, B, S = batch(K, "eloc" if table else "eloc_fb", n, d)
    a, b = span
    x = walkers(n, d, B)
    r = K.eloc(K.net(1.0, table), x, nup, ndn, Z_COULOMB, a, b)
    assert r["stats"][3] == 0, r["stats"][:4]
    assert (r["hout"] > 0).all() and (r["hout"] <= abs(b - a)).all(), r["hout"]
    e = eloc_errors({k: v[:S] for k, v in r.items() if k in ELOC_BARS}, ref_eloc(golden, x[:S], nup, ndn, span))
    r1 = K.eloc(K.net(b - a, table), x, nup, ndn, Z_COULOMB, 0.0, 1.0)
    assert r1["stats"][3] == 0
    i = eloc_errors(r, r1)
    print(f"SPANS eloc {nup}+{ndn} {d}d {fam} table={table} {sid(span)} B={B}: oracle " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          "; identity " + " ".join(f"{k} {v:.2e}" for k, v in i.items()))
    note(**{"eloc_" + k: v for k, v in e.items()}, **{"identity_eloc_" + k: v for k, v in i.items()})
    for k in ELOC_BARS:
        assert e[k] < ELOC_BARS[k], ("oracle", k, e[k])
        assert i[k] < ELOC_BARS[k], ("identity", k, i[k])


def adjoint_case(K, golden, n, d, table, span):
    """need_gx = True, random seeds a_z, a_d.  gx of the first S walkers of the full batch against the oracle; the sub-batch of S
    walkers gives the same gx bit for bit and the parameter gradient that the oracle's solve of S has."""
    fam, G, B, S = batch(K, "adjoint" if table else "adj_fb", n, d)
    a, b = span
    net, unit = K.net(1.0, table), K.net(b - a, table)
    y = walkers(n, d, B)
    a_z, a_d = seeds(n, d, B)
    gx, gp, st = K.adjoint(net, y, a_z, a_d, a, b)
    assert st[3] == 0 and np.isfinite(gx).all() and np.isfinite(gp).all(), st[:4]
    gxs, gps, st = K.adjoint(net, y[:S], a_z[:S], a_d[:S], a, b)
    assert st[3] == 0 and bits_equal(gxs, gx[:S])
    gxo, gpo = ref_adjoint(golden, y[:S], a_z[:S], a_d[:S], span)
    e_gx, e_gp = rel_max(gxs, gxo), rel_max(gps, gpo)
    gx1, gp1, s1 = K.adjoint(unit, y, a_z, a_d, 0.0, 1.0)
    assert s1[3] == 0
    i_gx, i_gp = rel_max(gx, gx1), rel_max(gp, scale_gp(gp1, b - a))
    print(f"SPANS adjoint {n}x{d} {fam} table={table} {sid(span)} B={B}: oracle gx {e_gx:.2e} gp {e_gp:.2e}; identity gx {i_gx:.2e} gp {i_gp:.2e} "
          f"(bar {BAR_GP:.0e})")
    note(adjoint_gx=e_gx, adjoint_gp=e_gp, identity_adjoint=max(i_gx, i_gp))
    assert max(e_gx, e_gp) < BAR_GP, (e_gx, e_gp)
    assert max(i_gx, i_gp) < BAR_GP, (i_gx, i_gp)


# ---- 2. batch and order independence ------------------------------------------------------------------------------------------------
def slots_case(K, golden, n, d, span):
    """x, walker_cost and walker_h_out of a walker are bit-identical in the reversed batch, under an explicit walker_order and in the
    sub-batch of G + 1; a step size is a magnitude whatever the direction: 0 < walker_h_out <= |b - a|."""
    fam, G, B, S = batch(K, "flow", n, d)
    a, b = span
    net = K.net(1.0, True)
    z = walkers(n, d, B)
    x, cost, hout, st = K.generate(net, z, a, b)
    assert st[3] == 0 and (hout > 0).all() and (hout <= abs(b - a)).all(), (st[:4], hout)
    xr, cr, hr, _ = K.generate(net, np.ascontiguousarray(z[::-1]), a, b)
    assert bits_equal(xr[::-1], x) and np.array_equal(cr[::-1], cost) and bits_equal(hr[::-1], hout), (n, d, span, "reversed")
    order = np.ascontiguousarray(np.random.default_rng(B).permutation(B), dtype=np.int32)
    xo, co, ho, _ = K.generate(net, z, a, b, order=order)
    assert bits_equal(xo, x) and np.array_equal(co, cost) and bits_equal(ho, hout), (n, d, span, "order")
    xs, cs, hs, _ = K.generate(net, z[:S], a, b)
    assert bits_equal(xs, x[:S]) and np.array_equal(cs, cost[:S]) and bits_equal(hs, hout[:S]), (n, d, span, "sub-batch")


# ---- 3. opening steps -----------------------------------------------------------------------------------------------------------
def _given_steps(B):
    """per-walker steps 2^-20 (1 + k / 8): dyadic, so that t0 +- step is exact at a dyadic t0"""
    return H0 * (1.0 + (np.arange(B) % 8) / 8.0)


def _same_step(hout, given, span):
    if span in DYADIC or span == CONTROL:
        return bits_equal(hout, given)
    # t0 is no dyadic number: (t0 +- h) - t0 rounds at ulp(t0) / 2 per operation
    return bool((np.abs(hout - given) <= 2.0 * np.spacing(max(abs(span[0]), abs(span[1])))).all())


def open_flow_case(K, golden, n, d, span):
    """walker_h_init per walker and with walker_h_uniform, max_steps = 1: one step of the given size is attempted, accepted (2^-20 is far
    below what the tolerance asks for) and reported in walker_h_out -- the given step, in both directions."""
    fam, G, B, S = batch(K, "flow", n, d)
    a, b = span
    net = K.net(1.0, True)
    z = walkers(n, d, B)
    hw = _given_steps(B)
    one_u = K.generate(net, z, a, b, h_init=np.array([H0]), uniform=True, max_steps=1)
    assert _same_step(one_u[2], np.full(B, H0), span), (n, d, span, one_u[2])
    one_w = K.generate(net, z, a, b, h_init=hw, max_steps=1)
    assert _same_step(one_w[2], hw, span), (n, d, span, one_w[2], hw)
    assert one_u[3][3] != 0 and one_w[3][3] != 0          # (the interval is not done after one such step: reported as failed)
    # the warm-started solve is the solve: within the bar of the oracle
    xw, _, hwo, sw = K.generate(net, z, a, b, h_init=hw)
    assert sw[3] == 0 and (hwo >= hw).all() and (hwo <= abs(b - a)).all()
    err = float(np.abs(xw[:S] - ref_generate(golden, z[:S], span)).max())
    note(flow_x_warm=err)
    assert err < BAR_FLOW, err


def open_eloc_case(K, golden, nup, ndn, span):
    n, d = nup + ndn, 2
    fam, G, B, S = batch(K, "eloc", n, d)
    a, b = span
    net = K.net(1.0, True)
    x = walkers(n, d, B)
    hw = _given_steps(B)
    one_u = K.eloc(net, x, nup, ndn, Z_COULOMB, a, b, h_init=np.array([H0]), uniform=True, max_steps=1)
    assert _same_step(one_u["hout"], np.full(B, H0), span), (fam, span, one_u["hout"])
    one_w = K.eloc(net, x, nup, ndn, Z_COULOMB, a, b, h_init=hw, max_steps=1)
    assert _same_step(one_w["hout"], hw, span), (fam, span, one_w["hout"], hw)
    assert one_u["stats"][3] != 0 and one_w["stats"][3] != 0
    r = K.eloc(net, x, nup, ndn, Z_COULOMB, a, b, h_init=hw)
    assert r["stats"][3] == 0 and (r["hout"] >= hw).all() and (r["hout"] <= abs(b - a)).all()
    e = eloc_errors({k: v[:S] for k, v in r.items() if k in ELOC_BARS}, ref_eloc(golden, x[:S], nup, ndn, span))
    note(**{"eloc_" + k + "_warm": v for k, v in e.items()})
    for k in ELOC_BARS:
        assert e[k] < ELOC_BARS[k], (k, e[k])


def equal_case(K, golden, span):
    """walker_h_equal = True with walker_h_scale = 1.1 on the flow and the adjoint (6 particles in two dimensions) is, bit for bit in
    results and stats[:4], the same call given |b - a| / ceil(|b - a| / (1.1 h) - 1e-9) explicitly with scale 1.0 (ff_open_step)."""
    n, d = 6, 2
    fam, G, B, S = batch(K, "flow", n, d)
    a, b = span
    L = abs(b - a)
    net = K.net(1.0, True)
    z = walkers(n, d, B)
    x, _, hg, st = K.generate(net, z, a, b)
    assert st[3] == 0 and (hg > 0).all() and (hg <= L).all()
    hs = hg * 1.1
    hr = np.where(hs < L, L / np.ceil(L / np.minimum(hs, L) - 1e-9), hs)
    assert ((hs < L) & (hr < hs)).any(), "no walker's step is rounded: the case checks nothing"
    fe = K.generate(net, z, a, b, h_init=hg, h_scale=1.1, equal=True)
    fr = K.generate(net, z, a, b, h_init=hr, h_scale=1.0)
    assert fe[3][3] == 0 and bits_equal(fe[0], fr[0]) and np.array_equal(fe[1], fr[1]) and bits_equal(fe[2], fr[2]), (span, "flow")
    assert np.array_equal(fe[3][:4], fr[3][:4]), (fe[3][:4], fr[3][:4])
    assert float(np.abs(fe[0][:S] - ref_generate(golden, z[:S], span)).max()) < BAR_FLOW
    a_z, a_d = seeds(n, d, B)
    ae = K.adjoint(net, z, a_z, a_d, a, b, h_init=hg, h_scale=1.1, equal=True)
    ar = K.adjoint(net, z, a_z, a_d, a, b, h_init=hr, h_scale=1.0)
    # (the simulator's host threads deposit a launch's parameter gradient in no fixed order: to rounding there, bit for bit on the device)
    same_gp = bits_equal(ae[1], ar[1]) if K.gp_reproducible else rel_max(ae[1], ar[1]) < 1e-12
    assert ae[2][3] == 0 and bits_equal(ae[0], ar[0]) and same_gp, (span, "adjoint")
    assert np.array_equal(ae[2][:4], ar[2][:4]), (ae[2][:4], ar[2][:4])
    cold = K.adjoint(net, z, a_z, a_d, a, b)
    assert rel_max(ae[0], cold[0]) < BAR_GP and rel_max(ae[1], cold[1]) < BAR_GP      # (two solves at the same tolerance)


def clamp_case(K, golden, span):
    """walker_h_init larger than the interval is clamped to it: the solves succeed, no accepted step is longer than |b - a|, and the
    results are the solve's (flow and local energy against the oracle, the adjoint against its own cold start)."""
    a, b = span
    L = abs(b - a)
    net = K.net(1.0, True)
    fam, G, B, S = batch(K, "flow", 6, 2)
    z = walkers(6, 2, B)
    big = np.full(B, 10.0 * L)
    x, _, hout, st = K.generate(net, z, a, b, h_init=big)
    assert st[3] == 0 and (hout > 0).all() and (hout <= L).all(), (st[:4], hout)
    assert float(np.abs(x[:S] - ref_generate(golden, z[:S], span)).max()) < BAR_FLOW
    a_z, a_d = seeds(6, 2, B)
    gx, gp, st = K.adjoint(net, z, a_z, a_d, a, b, h_init=big)
    cold = K.adjoint(net, z, a_z, a_d, a, b)
    assert st[3] == 0 and rel_max(gx, cold[0]) < BAR_GP and rel_max(gp, cold[1]) < BAR_GP
    fam, G, B, S = batch(K, "eloc", 6, 2)
    xs = walkers(6, 2, B)
    r = K.eloc(net, xs, 3, 3, Z_COULOMB, a, b, h_init=np.full(B, 10.0 * L))
    assert r["stats"][3] == 0 and (r["hout"] > 0).all() and (r["hout"] <= L).all(), (r["stats"][:4], r["hout"])
    e = eloc_errors({k: v[:S] for k, v in r.items() if k in ELOC_BARS}, ref_eloc(golden, xs[:S], 3, 3, span))
    for k in ELOC_BARS:
        assert e[k] < ELOC_BARS[k], (k, e[k])


# ---- 4. the empty interval ----------------------------------------------------------------------------------------------------------
EMPTY_ELOC = [(2, 1, 2, 4.0), (3, 3, 2, 10.0), (1, 1, 3, 3.0)]      # (nup, ndn, d, the sum of the orbital energies)
EMPTY_CANCEL = 1e4       # largest (|lap| + |grad|^2) / E of the walkers, asserted on the oracle's log p0
EMPTY_RTOL = 1e-10       # fp64 rounding 1.1e-16 x that cancellation x 100 operations' worth of accumulation


def empty_flow_case(K, golden, n, d, table):
    fam, G, B, S = batch(K, "flow" if table else "flow_fb", n, d)
    a, b = EMPTY
    net = K.net(1.0, table)
    z = walkers(n, d, B)
    x, _, _, st = K.generate(net, z, a, b)
    assert st[3] == 0 and bits_equal(x, z), (n, d, table, st[:4])
    zb, dl, st = K.delta_logp(net, z, a, b)
    assert st[3] == 0 and bits_equal(zb, z) and bits_equal(dl, np.zeros(B)), (n, d, table, st[:4], dl)
    a_z, a_d = seeds(n, d, B)
    gx, gp, st = K.adjoint(net, z, a_z, a_d, a, b)
    assert st[3] == 0 and bits_equal(gx, a_z) and not gp.any(), (n, d, table, st[:4], np.abs(gp).max())


def empty_eloc_case(K, golden, nup, ndn, d, E, table):
    """Z = 0 and no flow: the walkers sample the oscillator's ground determinant, whose local energy is the sum of its orbital
    energies at every point; log p and its gradient are those of O.logprob at rounding."""
    n = nup + ndn
    fam, G, B, S = batch(K, "eloc" if table else "eloc_fb", n, d)
    a, b = EMPTY
    x = walkers(n, d, B)
    lp, g, lap = (O.logprob if d == 2 else O.logprob3d)(x, nup, ndn)
    cancel = float(((np.abs(lap) + (g * g).reshape(B, -1).sum(1)) / E).max())
    assert cancel < EMPTY_CANCEL, ("a walker near a node of the determinant: choose another seed", cancel)
    r = K.eloc(K.net(1.0, table), x, nup, ndn, 0.0, a, b)
    assert r["stats"][3] == 0, r["stats"][:4]
    assert bits_equal(r["z"], x) and bits_equal(r["dlogp"], np.zeros(B))
    e_e = float(np.abs(r["eloc"] / E - 1.0).max())
    e_l, e_g, e_0 = float(np.abs(r["logp"] - lp).max()), rel_max(r["grad"], g), rel_max(r["glogp0"], g)
    print(f"SPANS empty eloc {nup}+{ndn} {d}d {fam} table={table}: E_loc / {E:g} - 1 {e_e:.2e}  logp {e_l:.2e} grad {e_g:.2e} glogp0 {e_0:.2e} "
          f"(cancellation {cancel:.1e})")
    note(empty_eloc=e_e, empty_logp=e_l, empty_grad=max(e_g, e_0))
    assert e_e < EMPTY_RTOL and e_l < EMPTY_RTOL * max(1.0, float(np.abs(lp).max())) and max(e_g, e_0) < EMPTY_RTOL, (e_e, e_l, e_g, e_0)


# ---- 5. a reference of the autograd wrappers that shares nothing with the oracle's hand-derived adjoint -------------------------------
RK4_STEPS = 128


def rk4_reference(golden, use_mu, span, z=None, c=None, x=None, cz=None, cd=None, steps=RK4_STEPS):
    """torch fp64 on the CPU: the plain restatement of the velocity field (v_plain of tests/test_gpu_parity.py
    test_autograd_through_backflow_and_mlp), fixed-step RK4, autograd through it.
    z, c given: x = flow of z over (a, b), loss sum(c x) -> (x, d loss / d z, d loss / d theta in Backflow.parameters() order).
    x, cz, cd given: (z, Delta) = flow of (x, 0) under (v, -div v) from b to a (the divergence by autograd, one coordinate at a time),
    loss sum(cz z) + sum(cd Delta) -> (z, Delta, d loss / d x, d loss / d theta).
    128 steps: measured on the CPU against the oracle at 1e-10 / 1e-12 over SPANS and (0, 1), at 3 x 2 and 2 x 3, with and without a
    one-body net (rk4_vs_oracle), states and gradients of both directions agree within 3.6e-11 (gradients relative to their largest
    entry); with 64 steps the parameter gradient of generate is within 2.1e-10, with 32 within 2.1e-9.  A tenth of BAR_GP is 5e-9;
    tests/test_spans_hostsim.py asserts it at the span where the figure is largest."""
    import torch
    eta, mu = weights(golden, 1.0, use_mu)
    P = [torch.tensor(np.asarray(w, dtype=np.float64).reshape(-1), requires_grad=True) for w in (eta + (mu if mu is not None else ()))]
    y0 = torch.tensor(z if z is not None else x, requires_grad=True)
    n = y0.shape[1]
    eye = torch.eye(n, dtype=torch.float64)

    def mlp(w, r):
        return (torch.sigmoid(r * w[0] + w[1]) * w[2]).sum(-1, keepdim=True)

    def v(xx):
        rij = xx[:, :, None] - xx[:, None]
        dij = (rij + eye[..., None]).norm(dim=-1, keepdim=True)
        out = ((mlp(P[:3], dij) * rij) * (1 - eye)[..., None]).sum(dim=-2)
        return out + mlp(P[3:], xx.norm(dim=-1, keepdim=True)) * xx if mu is not None else out

    def f(state):
        if z is not None:
            return (v(state[0]),)
        vx = v(state[0])
        flat = vx.flatten(1)
        div = sum(torch.autograd.grad(flat[:, i].sum(), state[0], create_graph=True)[0].flatten(1)[:, i] for i in range(flat.shape[1]))
        return vx, -div

    a, b = span if z is not None else (span[1], span[0])
    h = (b - a) / steps
    state = (y0,) if z is not None else (y0, torch.zeros(len(y0), dtype=torch.float64))
    for _ in range(steps):
        k1 = f(state)
        k2 = f(tuple(s + 0.5 * h * k for s, k in zip(state, k1)))
        k3 = f(tuple(s + 0.5 * h * k for s, k in zip(state, k2)))
        k4 = f(tuple(s + h * k for s, k in zip(state, k3)))
        state = tuple(s + (h / 6.0) * (p + 2 * q + 2 * r + t) for s, p, q, r, t in zip(state, k1, k2, k3, k4))
    loss = (torch.tensor(c) * state[0]).sum() if z is not None else (torch.tensor(cz) * state[0]).sum() + (torch.tensor(cd) * state[1]).sum()
    g = torch.autograd.grad(loss, [y0] + P)
    return tuple(s.detach().numpy() for s in state) + (g[0].numpy(), np.concatenate([t.numpy() for t in g[1:]]))


AUTOGRAD_SHAPES = [(3, 2), (2, 3)]
AUTOGRAD_B = 23                    # 2 G + 3 at both shapes


def autograd_inputs(n, d):
    """walkers and the coefficients of the losses sum(c x) and sum(cz z) + sum(cd Delta)"""
    rng = np.random.default_rng(500 + 10 * n + d)
    B = AUTOGRAD_B
    return walkers(n, d, B), rng.standard_normal((B, n, d)) / B, rng.standard_normal((B, n, d)) / B, rng.standard_normal(B) / B


def rk4_vs_oracle(golden, n, d, use_mu, span):
    """the two references of case 5 against each other, on the CPU: (generate, delta_logp) worst relative gradient difference"""
    z, c, cz, cd = autograd_inputs(n, d)
    net = onet(golden, 1.0, use_mu)
    xo, _ = O.cnf_generate(z, net, span[0], span[1], ORT, OAT)
    gzo, gpo, _ = O.cnf_adjoint(xo, np.zeros(len(z)), c, np.zeros(len(z)), net, span[1], span[0], ORT, OAT)
    x, gz, gp = rk4_reference(golden, use_mu, span, z=z, c=c)
    e_gen = max(rel_max(gz, gzo), rel_max(gp, gpo), float(np.abs(x - xo).max()))
    zo, dlo, _ = O.cnf_delta_logp(z, net, span[0], span[1], ORT, OAT)
    gxo, gpo, _ = O.cnf_adjoint(zo, dlo, cz, cd, net, span[0], span[1], ORT, OAT)
    zb, dl, gx, gp = rk4_reference(golden, use_mu, span, x=z, cz=cz, cd=cd)
    e_dl = max(rel_max(gx, gxo), rel_max(gp, gpo), float(np.abs(zb - zo).max()), float(np.abs(dl - dlo).max()))
    return e_gen, e_dl
