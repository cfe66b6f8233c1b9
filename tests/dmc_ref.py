"""TEST-ONLY: a numpy restatement of include/fermiflow_dmc.h -- the limited drift, the proposal, the Green's-function accept step with
its weights and record, the comb -- and of the driver loop of fermiflow_amd.DMC, written from the header alone; Philox4x32-10 and the
uniforms of csrc/ff_rng.h restated for the counters the header names; closed-form wave functions for the known-answer tests; and ctypes
callers of the three entry points on numpy buffers (the host simulator's library, or the real one for its refusals).
The same orders of summation as the header: plain IEEE doubles, no fused multiply-add anywhere."""
import ctypes as C
import math

import numpy as np

REC, CHUNK, U_SLOT, SEGW = 9, 256, 64, 32
M32 = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10 (csrc/ff_rng.h): key = seed, counter = (walker lo, walker hi, step, slot)
def philox(seed, walker, step, slot):
    walker = np.atleast_1d(np.asarray(walker, dtype=np.uint64))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    c0, c1 = walker & M32, walker >> np.uint64(32)
    c2 = np.full_like(c0, np.uint64(step)); c3 = np.full_like(c0, np.uint64(slot))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def uniform(seed, walker, step, slot):
    """ff_uniform: 53 bits of the block's first two words, in [0, 1)"""
    c0, c1, _, _ = philox(seed, walker, step, slot)
    return (((c0 << np.uint64(32)) | c1) >> np.uint64(11)).astype(np.float64) * 1.1102230246251565e-16


def accept_uniforms(seed, B, step, walker_offset=0):
    return uniform(seed, np.arange(B, dtype=np.uint64) + np.uint64(walker_offset), step, U_SLOT)


def comb_uniform(seed, step):
    return float(uniform(seed, np.uint64(1) << np.uint64(63), step, 0)[0])


# ---- the contract
def drift(g, tau, a):
    """the limited drift of every particle: g (..., n, 2) -> (..., n, 2)"""
    c = (2.0 * a) * tau
    vx, vy = 0.5 * g[..., 0], 0.5 * g[..., 1]
    v2 = vx * vx + vy * vy
    s = 2.0 / (1.0 + np.sqrt(1.0 + c * v2))
    return np.stack([vx * s, vy * s], axis=-1)


def propose(x, grad, xi, tau, a):
    with np.errstate(all="ignore"):
        return (x + tau * drift(grad, tau, a)) + math.sqrt(tau) * xi


def ordered_sum(v, op=np.add):
    """v (B,) summed as the header states: chunks of 256, in a chunk eight segments of 32 in walker order, the segments in order, the
    chunks in order (absent walkers add zeros)"""
    v = np.asarray(v, dtype=np.float64)
    nch = max(1, -(-len(v) // CHUNK))
    p = np.zeros(nch * CHUNK); p[:len(v)] = v
    p = p.reshape(nch, CHUNK // SEGW, SEGW)
    seg = np.zeros(p.shape[:2])
    for k in range(SEGW):
        seg = op(seg, p[:, :, k])
    ch = seg[:, 0].copy()
    for s in range(1, seg.shape[1]):
        ch = op(ch, seg[:, s])
    tot = 0.0
    for c in range(nch):
        tot = op(tot, ch[c])
    return float(tot)


def accept(state, prop, u, tau, a, ctrl):
    """state, prop: dicts x, logp, grad, eloc, sign (state also w).  Returns (new state, info): info has the mask `acc`, p, q, the flags
    dead / invalid / crossed and the record `rec` (six doubles, three integers)."""
    x, lp, g, e, sg, w = (np.asarray(state[k], dtype=np.float64) for k in ("x", "logp", "grad", "eloc", "sign", "w"))
    x1, lp1, g1, e1, sg1 = (np.asarray(prop[k], dtype=np.float64) for k in ("x", "logp", "grad", "eloc", "sign"))
    B, n = x.shape[0], x.shape[1]
    e_t, e_ref, c = (float(v) for v in ctrl)
    fin = np.isfinite
    with np.errstate(all="ignore"):
        alive = fin(lp) & fin(e) & fin(sg) & fin(w) & (w >= 0) & fin(x).all((1, 2)) & fin(g).all((1, 2))
        valid = fin(lp1) & fin(e1) & fin(sg1) & fin(x1).all((1, 2)) & fin(g1).all((1, 2))
        b0, b1 = drift(g, tau, a), drift(g1, tau, a)
        sf, sb = np.zeros(B), np.zeros(B)
        for i in range(n):
            dx, dy = (x1[:, i, 0] - x[:, i, 0]) - tau * b0[:, i, 0], (x1[:, i, 1] - x[:, i, 1]) - tau * b0[:, i, 1]
            sf = sf + (dx * dx + dy * dy)
            ex, ey = (x[:, i, 0] - x1[:, i, 0]) - tau * b1[:, i, 0], (x[:, i, 1] - x1[:, i, 1]) - tau * b1[:, i, 1]
            sb = sb + (ex * ex + ey * ey)
        two_tau = 2.0 * tau
        lf, lb = -(sf / two_tau), -(sb / two_tau)
        q = ((lp1 - lp) + lb) - lf
        invalid = alive & ~valid
        crossed = alive & valid & ~(sg1 * sg > 0)
        go = alive & valid & ~crossed
        p = np.where(go, np.where(q >= 0, 1.0, np.where(q < 0, np.exp(np.where(q < 0, q, 0.0)), 0.0)), 0.0)
        acc = alive & (u < p)
        e_now = np.where(acc, e1, e)
        clip = lambda v: np.minimum(np.maximum(v, e_ref - c), e_ref + c)
        mid = 0.5 * (clip(e) + clip(e_now))
        wn = np.where(alive, w * np.exp(tau * (e_t - mid)), 0.0)
        we = np.where(alive, wn * e_now, 0.0)
        we2 = np.where(alive, we * e_now, 0.0)
    new = {}
    for k, old, nw in (("x", x, x1), ("logp", lp, lp1), ("grad", g, g1), ("eloc", e, e1), ("sign", sg, sg1)):
        m = acc.reshape((B,) + (1,) * (old.ndim - 1))
        new[k] = np.where(m, nw, old)
    new["w"] = wn
    rec = [ordered_sum(wn), ordered_sum(we), ordered_sum(we2), ordered_sum(wn * wn), ordered_sum(p), ordered_sum(wn, np.maximum),
           int(acc.sum()), int(crossed.sum()), int((invalid | ~alive).sum())]
    return new, dict(acc=acc, p=p, q=q, dead=~alive, invalid=invalid, crossed=crossed, rec=rec)


def cumulative(w):
    """(ws, cum, W, jlast) in the header's association"""
    w = np.asarray(w, dtype=np.float64)
    B = len(w)
    with np.errstate(all="ignore"):
        ws = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    nch = -(-B // CHUNK)
    loc = np.concatenate([np.cumsum(ws[c * CHUNK:(c + 1) * CHUNK]) for c in range(nch)])      # (cumsum adds left to right)
    T = np.array([loc[min(B, (c + 1) * CHUNK) - 1] for c in range(nch)])
    P = np.zeros(nch)
    for c in range(1, nch):
        P[c] = P[c - 1] + T[c - 1]
    cum = P[np.arange(B) // CHUNK] + loc
    pos = np.nonzero(ws > 0)[0]
    return ws, cum, float(cum[-1]), int(pos[-1]) if len(pos) else -1


def comb(w, u0):
    """(src int32 (B), distinct, largest copy count, flag)"""
    B = len(w)
    ws, cum, W, jlast = cumulative(w)
    if not (W > 0 and np.isfinite(W)):
        return np.arange(B, dtype=np.int32), B, 1, 1
    t = (np.arange(B, dtype=np.float64) + u0) * (W / float(B))
    src = np.minimum(np.searchsorted(cum, t, side="right"), jlast).astype(np.int32)
    return src, len(np.unique(src)), int(np.bincount(src).max()), 0


# ---- closed-form guides (zero flow): dicts logp, grad, eloc, sign of walkers x (B, n, 2)
def two_electrons(Z=1.0):
    """1 + 1 in the trap, psi = exp(-(r1^2 + r2^2) / 2): E_loc = 2 + Z / r12, nodeless"""
    def f(x):
        r12 = np.sqrt(((x[:, 0] - x[:, 1]) ** 2).sum(-1))
        with np.errstate(all="ignore"):
            return dict(logp=-(x ** 2).sum((1, 2)), grad=-2.0 * x, eloc=2.0 + Z / r12, sign=np.ones(len(x)))
    return f


def _det3(p):
    """D = det [1, x_i, y_i] of three particles p (B, 3, 2), and its gradient (B, 3, 2); D is harmonic"""
    x1, y1, x2, y2, x3, y3 = p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1], p[:, 2, 0], p[:, 2, 1]
    D = (x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1)
    dD = np.stack([np.stack([y2 - y3, x3 - x2], -1), np.stack([y3 - y1, x1 - x3], -1), np.stack([y1 - y2, x2 - x1], -1)], 1)
    return D, dD


def three_plus_three(x):
    """3 + 3 free fermions in the trap (Z = 0), the ground state: psi = D_up D_dn exp(-r^2 / 2), E_loc = 10 for every walker.  The
    energy is EVALUATED, -lap / 4 - |grad|^2 / 8 + r^2 / 2 of log p = 2 ln|psi|, not set."""
    g, lap, sign = -2.0 * x, np.full(len(x), -2.0 * 12), np.ones(len(x))
    for off in (0, 3):
        D, dD = _det3(x[:, off:off + 3])
        g[:, off:off + 3] += 2.0 * dD / D[:, None, None]
        lap = lap - 2.0 * (dD ** 2).sum((1, 2)) / D ** 2
        sign = sign * np.sign(D)
    r2 = (x ** 2).sum((1, 2))
    logp = -r2 + sum(2.0 * np.log(np.abs(_det3(x[:, o:o + 3])[0])) for o in (0, 3))
    return dict(logp=logp, grad=g, eloc=-0.25 * lap - 0.125 * (g ** 2).sum((1, 2)) + 0.5 * r2, sign=sign)


# ---- the driver loop of fermiflow_amd.DMC, on the host with numpy's generator
def run(guide, x0, tau, nblocks, steps_per_block, equilibrate=0, drift_limit=1.0, ecut=0.2, seed=0, comb_on=True, trace=None):
    """Blocks of steps: propose, guide(x'), accept, comb; after a block E_ref = E_T = (sum sum w e) / (sum sum w) over the measured steps so
    far (over the block itself while equilibrating).  Returns a dict like DMC.result(); trace: a list that receives every step's record."""
    rng = np.random.default_rng(seed)
    x0 = np.asarray(x0, dtype=np.float64)
    B, n = x0.shape[0], x0.shape[1]
    st = dict(guide(x0), x=x0.copy(), w=np.ones(B))
    e_vmc = float(st["eloc"].mean())
    ctrl = [e_vmc, e_vmc, ecut * math.sqrt(n / tau)]
    blocks, tot, step = [], np.zeros(2), 0
    diag = dict(acc=0, crossed=0, invalid=0, esf=0.0, distinct=0.0, steps=0)
    for blk in range(equilibrate + nblocks):
        bsum = np.zeros(2)
        for _ in range(steps_per_block):
            x1 = propose(st["x"], st["grad"], rng.standard_normal(x0.shape), tau, drift_limit)
            st, info = accept(st, dict(guide(x1), x=x1), rng.random(B), tau, drift_limit, ctrl)
            r = info["rec"]
            if trace is not None:
                trace.append(r)
            bsum += r[0], r[1]
            if blk >= equilibrate:
                diag["acc"] += r[6]; diag["crossed"] += r[7]; diag["invalid"] += r[8]; diag["steps"] += 1
                diag["esf"] += r[0] ** 2 / (B * r[3])
            if comb_on:
                src, distinct, _, flag = comb(st["w"], rng.random())
                if flag:
                    raise FloatingPointError("the population's total weight is zero or not finite")
                st = {k: v[src] for k, v in st.items()}
                st["w"] = np.ones(B)
                if blk >= equilibrate:
                    diag["distinct"] += distinct
            step += 1
        if blk >= equilibrate:
            blocks.append(bsum[1] / bsum[0])
            tot += bsum
            ctrl[0] = ctrl[1] = tot[1] / tot[0]
        else:
            ctrl[0] = ctrl[1] = bsum[1] / bsum[0]
    blocks = np.array(blocks)
    ns = max(diag["steps"], 1)
    return dict(E=float(tot[1] / tot[0]) if len(blocks) else float("nan"),
                E_err=float(blocks.std(ddof=1) / math.sqrt(len(blocks))) if len(blocks) > 1 else float("nan"), E_vmc=e_vmc,
                acceptance=diag["acc"] / (ns * B), crossing=diag["crossed"] / (ns * B), invalid=diag["invalid"], esf=diag["esf"] / ns,
                distinct=diag["distinct"] / ns, blocks=blocks, walkers=st["x"])


# ---- the three entry points on numpy buffers (lib: the host simulator's, or any library for a refusal)
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _d(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def call_propose(lib, x, grad, tau, a, nup, ndn, noise=None, seed=0, walker_offset=0, step=0, want_xi=True):
    x, grad, noise = _d(x), _d(grad), _d(noise)
    xn, xi = np.full_like(x, 7.0), (np.full_like(x, 7.0) if want_xi else None)
    st = lib.ff_dmc_propose(None, x.shape[0], nup, ndn, 2, tau, a, _p(x), _p(grad), _p(noise), seed, walker_offset, step, _p(xn), _p(xi))
    assert st == 0, lib.ff_last_error()
    return xn, xi


def call_accept(lib, state, prop, tau, a, ctrl, nup, ndn, u=None, seed=0, walker_offset=0, step=0, groups=0, slot=0, nslots=1):
    """-> (new state, accepted uint8 (B), the record as [six floats, three ints], the whole trace as float64 words)"""
    s = {k: _d(state[k]).copy() for k in ("x", "logp", "grad", "eloc", "sign", "w")}
    q = {k: _d(prop[k]) for k in ("x", "logp", "grad", "eloc", "sign")}
    B = s["x"].shape[0]
    u, ctrl = _d(u), _d(ctrl)
    rec = np.full(nslots * REC, -3.0)
    acc = np.full(B, 9, dtype=np.uint8)
    ws = np.zeros(lib.ff_dmc_accept_workspace_bytes(B) // 8)
    ws[1:] = 5.5      # (only the ticket need be zero)
    st = lib.ff_dmc_accept(None, B, nup, ndn, 2, tau, a, *[_p(s[k]) for k in ("x", "logp", "grad", "eloc", "sign", "w")],
                           *[_p(q[k]) for k in ("x", "logp", "grad", "eloc", "sign")], _p(u), seed, walker_offset, step, _p(ctrl), _p(rec), slot,
                           _p(acc), groups, _p(ws))
    assert st == 0, lib.ff_last_error()
    assert ws.view(np.int64)[0] == 0
    r = rec[slot * REC:(slot + 1) * REC]
    return s, acc, list(r[:6]) + [int(v) for v in r[6:].view(np.int64)], rec


def call_comb(lib, state, nup, ndn, u0=None, seed=0, step=0):
    """-> (src, gathered state with w, info int32 [4])"""
    s = {k: _d(state[k]) for k in ("x", "logp", "grad", "eloc", "sign")}
    w = _d(state["w"]).copy()
    B = len(w)
    o = {k: np.full_like(v, 7.0) for k, v in s.items()}
    src, info = np.full(B, -1, dtype=np.int32), np.full(4, -1, dtype=np.int32)
    ws = np.zeros(lib.ff_dmc_comb_workspace_bytes(B) // 8)
    ws[1:] = 5.5
    u0 = None if u0 is None else np.array([u0], dtype=np.float64)
    st = lib.ff_dmc_comb(None, B, nup, ndn, 2, _p(w), *[_p(s[k]) for k in ("x", "logp", "grad", "eloc", "sign")], _p(u0), seed, step, _p(src),
                         *[_p(o[k]) for k in ("x", "logp", "grad", "eloc", "sign")], _p(info), _p(ws))
    assert st == 0, lib.ff_last_error()
    assert ws.view(np.int64)[0] == 0
    o["w"] = w
    return src, o, info


def random_state(seed, B, n, spread=1.0):
    """a seeded state and proposal with every field finite, signs +-1 and local energies around 10 with a tail beyond any clip"""
    rng = np.random.default_rng(seed)

    def one():
        return dict(x=rng.standard_normal((B, n, 2)), logp=rng.standard_normal(B) * spread, grad=rng.standard_normal((B, n, 2)) * 2.0,
                    eloc=10.0 + rng.standard_normal(B) * 3.0, sign=rng.choice([-1.0, 1.0], B))
    s, q = one(), one()
    s["w"] = rng.uniform(0.5, 1.5, B)
    q["x"] = s["x"] + 0.2 * rng.standard_normal((B, n, 2))
    q["sign"] = np.where(rng.random(B) < 0.9, s["sign"], -s["sign"])
    return s, q


def spoiled(seed, B, n):
    """random_state with one walker of every special kind (B >= 16): returns state, proposal, {kind: walker}"""
    s, q = random_state(seed, B, n)
    kinds = {}
    if B >= 16:
        kinds = {"nan proposal": 2, "zero sign": 3, "flipped sign": 4, "dead nan x": 5, "dead inf eloc": 6, "above clip": 7, "below clip": 8,
                 "nan grad proposal": 9, "negative w": 10, "inf logp proposal": 11}
        q["x"][2, n - 1, 1] = np.nan
        q["sign"][3] = 0.0
        q["sign"][4] = -s["sign"][4]
        s["x"][5, 0, 0] = np.nan
        s["eloc"][6] = np.inf
        s["eloc"][7], q["eloc"][7] = 1e3, 2e3
        s["eloc"][8], q["eloc"][8] = -1e3, -2e3
        q["grad"][9, 0, 0] = np.nan
        s["w"][10] = -1.0
        q["logp"][11] = np.inf
        for b in (7, 8):                                  # these two move: same sign, a proposal far more probable
            q["sign"][b] = s["sign"][b]; q["logp"][b] = s["logp"][b] + 500.0
    return s, q, kinds
