"""TEST-ONLY: the cases of tests/test_gpu_eloc_states.py and tests/test_eloc_states_hostsim.py, stated once over a backend K (the device
through fermiflow_amd.native, or the host simulator through tests/hostsim/simlib.py), so that a CPU run has checked them before a GPU
sees them.

They pin the six pieces of code that finish a local energy -- each decodes the orbital degrees of a walker's Slater determinants and
builds the Slater rows of z(t0) in its own way -- at excited orbital sets and with one set per walker (tab_up / tab_dn of NST rows and
a sorted walker_state, what BetaVMC passes):
  F1  the epilogue of the matrix-core kernel (csrc/ff_eloc_mfma.h), nup == ndn <= 3 in d = 2;
  F2  ff_eloc_slater_fixed_kernel<1..4> + ff_eloc_contract_kernel (csrc/ff_cnf_fwd.hip), equal or single determinants up to size 4;
  F3  ff_slater_rows_launch<2> (csrc/ff_ho3d.hip) + the contract kernel, larger or unequal determinants;
  F4  ff_eloc_finish3d, d = 3;
  F5  the fused finish of the one-walker-per-workgroup kernels (csrc/ff_wide.hip), ff_ode.compact_finish;
  F6  the same instantiation as the heavy-walker route beside F1 (launch_routed, csrc/ff_cnf_fwd.hip).

Checks per case (run_case / run_looping / run_routed):
  1. against the oracle at 1e-11 / 1e-13 with the same tables and states (the kernel at 1e-9 / 1e-11): E_loc relative per walker, grad
     and glogp0 absolute, lap relative to 1 + |lap|, logp and dlogp absolute, z absolute (the same solver and tolerance as what is behind
     grad: G_ATOL); no failed walker, everything finite;
  2. every output of a walker bit for bit the same in every batch it appears in and under an explicit walker order;
  3. the state is honoured: walkers of state != 0 differ from the same walkers run with walker_state = 0 by more than 1e-3 relative in
     logp or E_loc, and a table with shuffled rows (walker_state remapped, walkers sorted again) gives every walker the same bits;
  4. ground equivalence: walker_state = 0 with the NST-row table, walker_state = None with its first row alone, and the plain ground
     table give the same bits (no finish path documents another operation order for run-time degrees: csrc/ff_slater.h).

The local-energy kernel of a process is chosen once (FF_ELOC_KERNEL), so the cases that force the matrix-core kernel run in a child:
    FF_ELOC_KERNEL=mfma python -m tests.eloc_states_cases gpu|sim CASE

Backend:  name;  net(eta, mu, table) -> handle;  plan(n, d) -> family of the local-energy call;  cus() -> compute units of the plan;
eloc(handle, x, nup, ndn, tu, td, ws, order=None, compact=False, two_pass=False, wide=False, route=None) -> dict of numpy arrays (eloc,
grad, lap, logp, z, dlogp, glogp0, stats); tu / td: None = the ground set; wide: ff_set_kernel_family(1) around the call; route:
(walker_class, heavy_class)."""
import os
import sys

import numpy as np

KEYS = ("eloc", "grad", "lap", "logp", "z", "dlogp", "glogp0")
# the bars of tests/eloc_mfma_cases.py for this comparison (kernel 1e-9 / 1e-11 against oracle 1e-11 / 1e-13), and the log p bar of
# test_betavmc_two_spin_species_vs_oracle
E_RTOL, G_ATOL, L_TOL, LOGP_ATOL = 1e-7, 1e-7, 1e-6, 1e-6
MARGIN = 1e-3          # relative determinant margin (tests/obdm_ref.py slater_sign) every compared walker keeps at the oracle's z(t0)
NST = 5                # orbital sets per species: row 0 the ground set, the others sorted random subsets
POOL = 9
# sorted, every state present, three distinct states among the four walkers of the first wave of the matrix-core kernel
WS = np.array([0, 1, 2, 2, 3, 3, 4, 4, 4], dtype=np.int32)
assert (np.diff(WS) >= 0).all() and set(WS) == set(range(NST)) and any(len(set(WS[i:i + 4])) >= 3 for i in range(0, POOL, 4))
Z = 2.0
FULL = "mt:3+4+5+9o,md:3+4+5+9o,nt:3+4+5+9o,nd:3+4+5+9o"      # at most 12 coordinates
ONE = "mt:3+4+5+9o"                                             # beyond: one-body net and radial table only (the oracle's time)

# name -> (path, nup, ndn, d, how, family of the device's plan at this shape).  how: "mfma" = child with FF_ELOC_KERNEL=mfma (the
# family is then the forced one: the shapes are on the list FF_ELOC_MFMA of csrc/ff_plan.h), "auto", "two_pass" (ff_eloc_sensitivities
# + ff_eloc_finish), "compact" (ff_ode.compact_finish), "wide" (compact, with ff_set_kernel_family(1): the shape's own plan is narrow)
CASES = {
    "F1-1+1": ("F1", 1, 1, 2, "mfma", "columns"), "F1-2+2": ("F1", 2, 2, 2, "mfma", "mfma"), "F1-3+3": ("F1", 3, 3, 2, "mfma", "mfma"),
    "F1-2+2-auto": ("F1", 2, 2, 2, "auto", "mfma"), "F1-3+3-auto": ("F1", 3, 3, 2, "auto", "mfma"),
    "F2-1+0": ("F2", 1, 0, 2, "auto", "rows"), "F2-2+0": ("F2", 2, 0, 2, "auto", "columns"), "F2-2+2": ("F2", 2, 2, 2, "two_pass", "mfma"),
    "F2-3+3": ("F2", 3, 3, 2, "two_pass", "mfma"), "F2-4+0": ("F2", 4, 0, 2, "auto", "mfma"), "F2-4+4": ("F2", 4, 4, 2, "auto", "split"),
    "F3-5+0": ("F3", 5, 0, 2, "auto", "mfma"), "F3-4+2": ("F3", 4, 2, 2, "auto", "mfma"), "F3-3+2": ("F3", 3, 2, 2, "auto", "mfma"),
    "F3-6+5": ("F3", 6, 5, 2, "auto", "wide"),
    "F4-2+1": ("F4", 2, 1, 3, "auto", "rows"), "F4-2+2": ("F4", 2, 2, 3, "auto", "rows"), "F4-5+4": ("F4", 5, 4, 3, "auto", "wide"),
    "F5-3+3": ("F5", 3, 3, 2, "wide", "mfma"), "F5-4+3": ("F5", 4, 3, 2, "wide", "rows"), "F5-7+6": ("F5", 7, 6, 2, "compact", "wide"),
    "F5-2+2-3d": ("F5", 2, 2, 3, "wide", "rows"), "F5-5+4-3d": ("F5", 5, 4, 3, "compact", "wide"),
}
# What the simulator runs of a case (default: SIM_PLAN, with checks 3 and 4 on the whole pool).  plan: see parse_plan; xb: batch of
# checks 3 and 4 (0: not run); sel: these pool walkers alone, as one batch, against the oracle (check 1 only).  Every simulated lane is
# a host thread and every exchange a barrier: a workgroup of the one-walker-per-workgroup kernels takes 1 to 4 s per walker, a wave of
# the matrix-core kernel 0.1 to 1 s, and several times that beside the other simulator tests.  So the matrix-core cases take five
# walkers (a full wave with three states and one with idle slots), the shapes beyond 20 coordinates two walkers of two excited states
# (one of them the set with a top-shell orbital: one batch, so check 2 is the device's there), the forced wide shapes one batch each
# -- 3+3 the nine walkers that make its grid loop -- and checks 3 and 4 run on F5 once per decode (3+3 for HO2D, 2+2 for HO3D).  The in-process "auto" twins of F1 are the device's alone: the simulator's
# plan has no matrix-core kernel (FF_MFMA_FROM=99), so they would repeat F2-2+2 / F2-3+3.
SIM = {
    "F1-1+1": dict(plan="mt:5o,nd:3", xb=4), "F1-2+2": dict(plan="mt:5o", xb=4), "F1-3+3": dict(plan="mt:5", xb=4),
    "F1-2+2-auto": None, "F1-3+3-auto": None, "F2-4+4": dict(plan="mt:5o", xb=4),
    "F3-6+5": dict(sel=(1, 6)), "F4-5+4": dict(sel=(1, 6)), "F5-7+6": dict(sel=(1, 6)), "F5-5+4-3d": dict(sel=(1, 6)),
    "F5-3+3": dict(plan="mt:9", xb=3), "F5-4+3": dict(plan="mt:5", xb=0), "F5-2+2-3d": dict(plan="mt:3", xb=3),
}
SIM_PLAN = "mt:5o,nd:9"      # the simulator's default up to 12 coordinates: 3 of the 20 launches (both nets, both radial paths)
SIM_FAMILY = {"mfma": "columns"}      # the simulator's plan where the device's names the matrix-core kernel


def sim_cases():
    return [c for c in CASES if SIM.get(c, {}) is not None]


def top_shell(d):
    """first orbital index of the top shell of the orbital lists: degree 7 of the 36 HO2D orbitals, shell 5 of the first 56 HO3D ones"""
    return 28 if d == 2 else 35


def tables(nup, ndn, d, name=None):
    """(tab_up, tab_dn): NST distinct rows per species, row 0 the ground set, the last row of the first species with an orbital of the
    top shell; None for an empty species"""
    rng = np.random.default_rng(TABLE_SEEDS.get(name, 7000 + 100 * nup + 10 * ndn + d))
    norb, top = (36, 28) if d == 2 else (56, 35)

    def one(k, force_top):
        if k == 0:
            return None
        rows = [np.arange(k)]
        while len(rows) < NST:
            row = np.sort(rng.choice(norb, k, replace=False))
            if force_top and len(rows) == NST - 1 and row[-1] < top:
                row[-1] = rng.integers(top, norb)
            if not any((row == r).all() for r in rows):
                rows.append(row)
        return np.array(rows, dtype=np.int32)
    tu, td = one(nup, True), one(ndn, nup == 0)
    assert max(int(t.max()) for t in (tu, td) if t is not None) >= top, "no orbital of the top shell"
    assert all((np.diff(t, axis=1) > 0).all() and (t[0] == np.arange(t.shape[1])).all() for t in (tu, td) if t is not None)
    return tu, td


# walker seeds: default_rng(1000 + 10 n + d) unless the conditions of reference() asked for another one (found on the CPU with the oracle
# alone: the first of 1000 + 10 n + d + 100 j that meets them for every compared walker); for 7+6 and 6+5 with another table seed, and for
# the nine particles in d = 3 another net: the default seed's flow contracts by e^-2 per coordinate, which drives every walker to a node
SEEDS = {"F1-2+2": 4942, "F1-2+2-auto": 4942, "F2-2+2": 4942, "F1-3+3": 1362, "F1-3+3-auto": 1362, "F2-3+3": 1362, "F5-3+3": 1362,
         "F2-2+0": 1222, "F2-4+0": 1442, "F2-4+4": 1682, "F3-5+0": 1652, "F3-4+2": 1162, "F3-3+2": 2752, "F3-6+5": 23412, "F4-2+2": 1543,
         "F5-2+2-3d": 1543, "F4-5+4": 1393, "F5-5+4-3d": 1393, "F5-4+3": 2372, "F5-7+6": 6932, "F6-2+2-sim": 1442, "F6-3+3-sim": 1062, "F6-2+2": 4642, "F6-3+3": 2562,
         "F5-6+6-loop": 3022, "F5-6+6-loop-sim": 1322}      # (the looping case: for the batch of 256 compute units, and for the simulator's)
TABLE_SEEDS = {"F5-7+6": 16, "F3-6+5": 5}
NET_SEEDS = {"F4-5+4": 171, "F5-5+4-3d": 171, "F5-6+6-loop": 191, "F5-6+6-loop-sim": 191}


def inputs(name, nup, ndn, d, B=POOL):
    """Seeded weights (ten and six hidden units, the scales of tests/eloc_mfma_cases.py inputs) and B walkers, normal x 1.2"""
    n = nup + ndn
    rng = np.random.default_rng(NET_SEEDS.get(name, 100 + 7 * n + d))
    eta = [rng.normal(size=10) * 0.5, rng.normal(size=10) * 0.3, rng.normal(size=10) * 0.06]
    mu = [rng.normal(size=6) * 0.5, rng.normal(size=6) * 0.3, rng.normal(size=6) * 0.06]
    x = np.random.default_rng(SEEDS.get(name, 1000 + 10 * n + d)).normal(size=(B, n, d)) * 1.2
    order = np.random.default_rng(n).permutation(POOL).astype(np.int32)
    return eta, mu, x, order


def margin(z, nup, ndn, d, tu, td, ws):
    """smallest |det| / prod(row norms) over the species of every walker, under its own orbital set (d = 2: obdm_ref.slater_sign; d = 3:
    the same quantity from the oracle's HO3D orbitals)"""
    if d == 2:
        from tests.obdm_ref import slater_sign
        return slater_sign(z, nup, ndn, tu, td, ws)[1]
    from oracle import oracle as O
    out = np.full(len(z), np.inf)
    for ns, off, tab in ((nup, 0, tu), (ndn, nup, td)):
        for b in range(len(z) if ns else 0):
            row = (np.arange(ns) if tab is None else np.asarray(tab).reshape(-1, ns)[0 if ws is None else ws[b]])
            Phi = O.orbitals3d(row, z[b, off:off + ns]).T
            out[b] = min(out[b], abs(np.linalg.det(Phi / np.linalg.norm(Phi, axis=1, keepdims=True))))
    return out


def _oracle(x, nup, ndn, d, eta, mu, tu, td, ws, rtol, atol):
    from oracle import oracle as O
    net = O.Net(eta, mu)
    ref = dict((O.eloc if d == 2 else O.eloc3d)(x, nup, ndn, net, Z, rtol=rtol, atol=atol, tab_up=tu, tab_dn=td, wstate=ws))
    ref["z"], ref["dlogp"], _ = O.cnf_delta_logp(x, net, rtol=rtol, atol=atol)
    ref["glogp0"] = (O.logprob if d == 2 else O.logprob3d)(ref["z"], nup, ndn, tab_up=tu, tab_dn=td, wstate=ws)[1]
    return ref


def reference(x, nup, ndn, d, eta, mu, tu, td, ws):
    """The oracle's outputs for the walkers x at 1e-11 / 1e-13 (E_loc, grad, lap, logp; z(t0) and Delta of the flow; grad log p0 at
    z(t0)).  Conditioning is decided by the reference alone and asserted here for every walker: the margin of its determinants at
    z(t0), and the oracle's own figures at the kernel's tolerances (1e-9 / 1e-11) within half of every bar -- the bars on grad and
    glogp0 are absolute, and an excited set's gradient amplifies the solver's error in z(t0) by the Hessian of log p0.  (Both
    conditions read the oracle only.  A seed is never chosen from what a kernel returns.)"""
    ref = _oracle(x, nup, ndn, d, eta, mu, tu, td, ws, 1e-11, 1e-13)
    m = margin(ref["z"], nup, ndn, d, tu, td, ws)
    assert (m > MARGIN).all(), ("a walker near a node of its determinant: choose another seed", m)
    own = errors(_oracle(x, nup, ndn, d, eta, mu, tu, td, ws, 1e-9, 1e-11), ref)
    assert all(v < BARS[k] / 2 for k, v in own.items()), ("ill-conditioned for the reference at the kernel's tolerances: choose another seed", own)
    return ref


def parse_plan(plan):
    out = []
    for item in plan.split(","):
        tag, bs = item.split(":")
        assert len(tag) == 2 and tag[0] in "mn" and tag[1] in "td", item
        out.append((tag[0] == "m", tag[1] == "t", tuple((int(b.rstrip("o")), b.endswith("o")) for b in bs.split("+"))))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, keys=KEYS):
    return [k for k in keys if not (_bits(a[k]) == _bits(b[k])).all()]


def errors(r, ref):
    """the figures of check 1"""
    return dict(eloc=float(np.abs(r["eloc"] / ref["eloc"] - 1.0).max()), grad=float(np.abs(r["grad"] - ref["grad"]).max()),
                glogp0=float(np.abs(r["glogp0"] - ref["glogp0"]).max()),
                lap=float((np.abs(r["lap"] - ref["lap"]) / (1.0 + np.abs(ref["lap"]))).max()),
                logp=float(np.abs(r["logp"] - ref["logp"]).max()), dlogp=float(np.abs(r["dlogp"] - ref["dlogp"]).max()),
                z=float(np.abs(r["z"] - ref["z"]).max()))


BARS = dict(eloc=E_RTOL, grad=G_ATOL, glogp0=G_ATOL, lap=L_TOL, logp=LOGP_ATOL, dlogp=LOGP_ATOL, z=G_ATOL)


def check_oracle(tag, r, ref, worst):
    e = errors(r, ref)
    print(f"ELOCSTATES {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  stats {[int(v) for v in r['stats'][:4]]}")
    for k, v in e.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert int(r["stats"][3]) == 0, (tag, "a walker failed")
    assert all(np.isfinite(r[k]).all() for k in KEYS), tag
    for k, v in e.items():
        assert v < BARS[k], (tag, k, v, BARS[k])


def report(name, path, worst):
    print(f"ELOCSTATES MAX {path} {name}: " + "  ".join(f"{k} {v:.2e} (bar {BARS[k]:.0e})" for k, v in worst.items()))


def take(ref, idx):
    return {k: v[idx] for k, v in ref.items() if k in KEYS}


def permuted(tu, td, ws, seed):
    """Tables with their rows shuffled, walker_state remapped, and the order that sorts the walkers again"""
    rng = np.random.default_rng(seed)
    p = rng.permutation(NST)
    while p[0] == 0:                          # (the ground set leaves row 0)
        p = rng.permutation(NST)
    inv = np.argsort(p)                       # new row p[s] = old row s
    ws2 = p[ws].astype(np.int32)
    srt = np.argsort(ws2, kind="stable")
    return (tu[inv] if tu is not None else None, td[inv] if td is not None else None, ws2[srt], srt)


def check_family(K, name):
    path, nup, ndn, d, how, fam = CASES[name]
    n = nup + ndn
    got = K.plan(n, d)
    assert got == (SIM_FAMILY.get(fam, fam) if K.name == "sim" else fam), (name, got, fam)
    if how == "mfma":
        # forced in this process, and instantiated at the shape (FF_ELOC_MFMA, csrc/ff_plan.h).  The plan above is the DEFAULT routing
        # of the shape ("columns" at 1+1): ff_kernel_plan does not see FF_ELOC_KERNEL.  That the forced kernel ran is shown by
        # forced_kernel_ran below, from the bits.
        assert os.environ.get("FF_ELOC_KERNEL") == "mfma" and d == 2 and 2 <= n <= 6, name
    elif path == "F1":
        assert got == "mfma" and os.environ.get("FF_ELOC_KERNEL") is None, name
    else:
        assert os.environ.get("FF_ELOC_KERNEL") is None, name
    if how in ("wide", "compact"):      # ff_wide_shape (csrc/ff_plan.h); "wide" forces the family, "compact" finds it in the plan
        assert n <= 24 and n * d <= 60 and (how == "wide") == (got != "wide"), name


def run_case(K, name):
    path, nup, ndn, d, how, _ = CASES[name]
    check_family(K, name)
    sim = (SIM.get(name) or {}) if K.name == "sim" else {}
    n = nup + ndn
    eta, mu, x, order = inputs(name, nup, ndn, d)
    tu, td = tables(nup, ndn, d, name)
    kw = dict(compact=how in ("wide", "compact"), two_pass=how == "two_pass", wide=how == "wide")
    run = lambda net, idx, tabs, ws, od=None: K.eloc(net, x[idx], nup, ndn, tabs[0], tabs[1], ws, order=od, **kw)
    refs, first, worst = {}, {}, {}
    sel = sim.get("sel")
    plan = parse_plan(sim.get("plan", (SIM_PLAN if K.name == "sim" else FULL) if n * d <= 12 else ONE)) if sel is None else [(True, True, ())]
    for use_mu, table, batches in plan:
        m = mu if use_mu else None
        if use_mu not in refs:      # one reference per net, shared by every batch
            refs[use_mu] = reference(x, nup, ndn, d, eta, m, tu, td, WS)
        ref = refs[use_mu]
        net = K.net(eta, m, table)
        tag = f"{name} {'one-body net' if use_mu else 'no one-body net'} {'table' if table else 'direct'}"
        runs = [(np.arange(B), None) for B, _ in batches] + [(np.arange(B), order[order < B].copy()) for B, o in batches if o]
        if sel is not None:
            runs = [(np.array(sel), None)]
        for idx, od in runs:
            r = run(net, idx, (tu, td), WS[idx], od)
            check_oracle(f"{tag} B={len(idx)}{' ordered' if od is not None else ''}", r, take(ref, idx), worst)
            # check 2: a walker's numbers depend on nothing but itself and its state
            for j, i in enumerate(idx):
                got = {k: _bits(r[k][j]).copy() for k in KEYS}
                want = first.setdefault((use_mu, table, int(i)), got)
                for k in KEYS:
                    assert (got[k] == want[k]).all(), (tag, len(idx), "ordered" if od is not None else "", i, k)
    report(name, path, worst)
    xb = sim.get("xb", 0 if sel is not None else POOL)
    if not xb:
        return
    use_mu, table, _ = plan[0]
    net = K.net(eta, mu if use_mu else None, table)
    idx, ws = np.arange(xb), WS[:xb]
    base = run(net, idx, (tu, td), ws)
    assert all((_bits(base[k][i]) == first[(use_mu, table, int(i))][k]).all() for i in idx if (use_mu, table, int(i)) in first for k in KEYS), name
    # check 3: the state is honoured, not defaulted
    zero = run(net, idx, (tu, td), np.zeros(xb, dtype=np.int32))
    ex = ws != 0
    diff = np.maximum(np.abs(base["logp"] - zero["logp"]) / np.abs(base["logp"]), np.abs(base["eloc"] - zero["eloc"]) / np.abs(base["eloc"]))
    assert ex.any() and (diff[ex] > 1e-3).all(), (name, diff)
    assert not _same(take(base, ~ex), take(zero, ~ex)), name
    tu2, td2, ws2, srt = permuted(tu, td, ws, n + d)
    perm = K.eloc(net, x[idx][srt], nup, ndn, tu2, td2, ws2, **kw)
    assert not _same(perm, take(base, srt)), (name, "shuffled table rows", _same(perm, take(base, srt)))
    # check 4: ground equivalence
    one_row = run(net, idx, (tu[:1] if tu is not None else None, td[:1] if td is not None else None), None)
    plain = run(net, idx, (None, None), None)
    assert not _same(zero, one_row) and not _same(zero, plain), (name, _same(zero, one_row), _same(zero, plain))
    print(f"ELOCSTATES {name}: state honoured (smallest relative change against state 0: {diff[ex].min():.1e}), shuffled rows and the "
          f"three ground runs bit-identical at B={xb}")


# ---------------------------------------------------------------------------------------------------------------- F5, the special cases
def run_common_table(K):
    """F5 at 4+3 with walker_state = None and ONE non-ground orbital set for every walker: the "decoded once per kernel" branch of
    csrc/ff_wide.hip.  Against the oracle, and bit for bit the run with the NST-row table and every walker in that row's state."""
    nup, ndn, d = 4, 3, 2
    eta, mu, x, order = inputs("F5-4+3-common", nup, ndn, d)
    tu, td = tables(nup, ndn, d, "F5-4+3-common")
    row = NST - 1                      # the set with the top-shell orbital
    assert tu[row].max() >= top_shell(d)
    B = 3 if K.name == "sim" else POOL
    x = x[:B]
    ws = np.full(B, row, dtype=np.int32)
    ref = reference(x, nup, ndn, d, eta, mu, tu, td, ws)
    net = K.net(eta, mu, True)
    assert K.plan(nup + ndn, d) != "wide"
    worst = {}
    r = K.eloc(net, x, nup, ndn, tu[row:row + 1], td[row:row + 1], None, compact=True, wide=True)
    check_oracle(f"F5-4+3-common B={B}", r, ref, worst)
    report("F5-4+3-common", "F5", worst)
    rs = K.eloc(net, x, nup, ndn, tu, td, ws, compact=True, wide=True)
    assert not _same(r, rs), _same(r, rs)
    ro = K.eloc(net, x, nup, ndn, tu[row:row + 1], td[row:row + 1], None, compact=True, wide=True, order=order[order < B].copy())
    assert not _same(r, ro), _same(r, ro)
    ground = K.eloc(net, x, nup, ndn, None, None, None, compact=True, wide=True)
    assert (np.abs(ground["logp"] - r["logp"]) > 1e-3 * np.abs(r["logp"])).all()


def looping_setup(cus, sim):
    """(B, walker_state, order of work, probe set) of the looping case at `cus` compute units"""
    from tests.common import assert_loops, kernel_families, looping_batch, probe_set
    n, d = 12, 2
    fams = kernel_families("eloc", n, d, cus, hostsim=sim)
    assert list(fams) == ["eloc_wide"], fams
    B = looping_batch(fams)
    assert_loops(fams, B)
    ws = ((np.arange(B) * NST) // B).astype(np.int32)
    assert set(ws) == set(range(NST)) and (np.diff(ws) >= 0).all()
    # the order of work: stride through the batch so that consecutive queue tickets are walkers of different states
    stride = B // NST + 1
    order = np.array(sorted(range(B), key=lambda b: (b % stride, b)), dtype=np.int32)
    assert sorted(order) == list(range(B)) and (ws[order[1:]] != ws[order[:-1]]).mean() > 0.5
    if sim:
        # nine walkers on four workgroups there: fewer workgroups than states, so whatever the queue hands out, some workgroup finishes
        # walkers of two states.  (On the device there are more workgroups than states and the queue decides who meets whom: the
        # alternating order makes a workgroup's next ticket a different state four times out of five, which is likely, not certain,
        # to mix states in a workgroup; the guaranteed seam is the simulator's.)  The oracle and the small batch take the two ends.
        g, r = fams["eloc_wide"]
        assert r // g < NST, fams
        return B, ws, order, np.array([0, B - 1])
    S = set(probe_set(B, fams, seed=n * d, nrand=0, edge_rounds=1).tolist()) | {int(np.flatnonzero(ws == s)[0]) for s in range(1, NST)}
    return B, ws, order, np.array(sorted(S))


def run_looping(K):
    """F5 at 6+6, compact, with a walker order so that the persistent grid takes the work queue, at a batch that gives every workgroup
    at least two walkers (tests/common.py looping_batch).  The queue hands a workgroup whatever walker comes next, and the order
    interleaves the states, so every workgroup meets walkers of different states one after the other.  The oracle runs on a probe set
    at the seams; the probe walkers alone, as a small batch with their own states, give the bits of the full launch."""
    nup, ndn, d = 6, 6, 2
    sim = K.name == "sim"
    B, ws, order, S = looping_setup(K.cus(), sim)
    eta, mu, x, _ = inputs("F5-6+6-loop" + ("-sim" if sim else ""), nup, ndn, d, B=B)
    tu, td = tables(nup, ndn, d, "F5-6+6-loop")
    ref = reference(x[S], nup, ndn, d, eta, mu, tu, td, ws[S])
    net = K.net(eta, mu, True)
    worst = {}
    full = K.eloc(net, x, nup, ndn, tu, td, ws, compact=True, order=order)
    assert int(full["stats"][3]) == 0 and all(np.isfinite(full[k]).all() for k in KEYS)
    sub = K.eloc(net, x[S], nup, ndn, tu, td, ws[S], compact=True)
    check_oracle(f"F5-6+6-loop B={B} |S|={len(S)}", sub, ref, worst)
    report("F5-6+6-loop", "F5", worst)
    assert not _same(take(full, S), sub), _same(take(full, S), sub)
    zero = K.eloc(net, x[S], nup, ndn, tu, td, np.zeros(len(S), dtype=np.int32), compact=True)
    ex = ws[S] != 0
    assert (np.abs(sub["logp"] - zero["logp"])[ex] > 1e-3 * np.abs(sub["logp"])[ex]).all()


# ---------------------------------------------------------------------------------------------------------------- F6
ROUTED_B = 2 * 1024 + 5
ROUTED_B_SIM = 13
HEAVY_CLASS = 12


def routed_setup(sim=False):
    """(B, walker_state, heavy walkers, light probes, walker_class, all probes sorted) of the routed cases.  The device: 2053 walkers,
    eight of class 20, among them two pairs b, b + 1024 in different states (the heavy kernel's 1024 workgroups stride over the batch,
    so one workgroup finishes both).  The simulator: 13 walkers, five of class 20, one per state -- a launch of 2053 is 514 simulated
    waves of the matrix-core kernel, minutes per shape; the heavy kernel still starts its 1024 workgroups, strides over the batch
    and skips the light walkers, but no workgroup of it meets two walkers (that seam is F5's in the simulator, and the device's here)."""
    B = ROUTED_B_SIM if sim else ROUTED_B
    ws = ((np.arange(B) * NST) // B).astype(np.int32)
    if sim:
        heavy, light = np.array([1, 4, 6, 9, 12]), np.array([0, 5, 11])
    else:
        heavy = np.array([3, 3 + 1024, 700, 700 + 1024, 411, 1500, 2047, 2052])
        assert ws[3] != ws[3 + 1024] and ws[700] != ws[700 + 1024]
        light = np.array([0, 1, 2, 4, 5, 699, 701, 1023, 1024, 1028, 2048, 2051])
    assert len(set(ws[heavy])) == NST
    wclass = np.zeros(B, dtype=np.int32)
    wclass[heavy] = 20
    return B, ws, heavy, light, wclass, np.sort(np.concatenate([heavy, light]))


def run_routed(K, nup, ndn):
    """F6: the heavy-walker route beside the matrix-core kernel (launch_routed).  walker_class is written by hand (routed_setup): class 20
    for the chosen walkers, 0 elsewhere.  The oracle runs on the heavy walkers (they integrate at 0.3 x the tolerances: the same bars)
    and on the light probes; the probes alone, with their own states and classes, give the bits of the full launch; without the route
    (heavy_class = -1) the light walkers keep their bits and the heavy ones do not; with walker_state = 0 the heavy walkers of every
    other state change."""
    d = 2
    n = nup + ndn
    sim = K.name == "sim"
    name = f"F6-{nup}+{ndn}"
    assert K.plan(n, d) == ("columns" if sim else "mfma") and nup == ndn
    if sim:      # (the plan of the simulator's build has no matrix-core kernel: forced in this process)
        assert os.environ.get("FF_ELOC_KERNEL") == "mfma"
    B, ws, heavy, light, wclass, S = routed_setup(sim)
    eta, mu, x, _ = inputs(name + ("-sim" if sim else ""), nup, ndn, d, B=B)
    tu, td = tables(nup, ndn, d, name)
    ref = reference(x[S], nup, ndn, d, eta, mu, tu, td, ws[S])
    net = K.net(eta, mu, True)
    full = K.eloc(net, x, nup, ndn, tu, td, ws, route=(wclass, HEAVY_CLASS))
    assert int(full["stats"][3]) == 0 and all(np.isfinite(full[k]).all() for k in KEYS)
    worst = {}
    check_oracle(f"{name} B={B} heavy", dict(take(full, heavy), stats=full["stats"]), take(ref, np.searchsorted(S, heavy)), worst)
    check_oracle(f"{name} B={B} light probes", dict(take(full, light), stats=full["stats"]), take(ref, np.searchsorted(S, light)), worst)
    report(name, "F6", worst)
    sub = K.eloc(net, x[S], nup, ndn, tu, td, ws[S], route=(wclass[S].copy(), HEAVY_CLASS))
    assert len(S) < B and not _same(take(full, S), sub), _same(take(full, S), sub)
    # the route was taken: without it the light walkers keep their bits, the heavy ones (0.3 x the tolerances on the route) do not
    plain = K.eloc(net, x[S], nup, ndn, tu, td, ws[S], route=(wclass[S].copy(), -1))
    hs, ls = np.isin(S, heavy), ~np.isin(S, heavy)
    assert not _same(take(plain, ls), take(sub, ls)) and (_bits(plain["eloc"][hs]) != _bits(sub["eloc"][hs])).all()
    zero = K.eloc(net, x[S], nup, ndn, tu, td, np.zeros(len(S), dtype=np.int32), route=(wclass[S].copy(), HEAVY_CLASS))
    ex = hs & (ws[S] != 0)
    assert ex.sum() >= NST - 1 and (np.abs(sub["logp"] - zero["logp"])[ex] > 1e-3 * np.abs(sub["logp"])[ex]).all()


# ---------------------------------------------------------------------------------------------------------------- ff_logprob
LOGPROB_SHAPES = [(1, 0, 2), (2, 2, 2), (4, 0, 2), (4, 4, 2), (5, 3, 2), (12, 12, 2), (2, 2, 3), (5, 4, 3)]
LOGPROB_B = 130


def run_logprob(K, nup, ndn, d):
    """ff_logprob / ff_logprob3d with derivatives under walker_state against the oracle (the bars of test_slater_fwd_bwd_laplacian);
    the walkers keep the margin condition themselves (they are the arguments of the determinants here)"""
    from oracle import oracle as O
    n, B = nup + ndn, LOGPROB_B
    tu, td = tables(nup, ndn, d)
    ws = ((np.arange(B) * NST) // B).astype(np.int32)
    rng = np.random.default_rng(2000 + 10 * n + d)
    x = rng.normal(size=(B, n, d)) * 1.2
    for _ in range(3000):      # chosen with the reference alone: candidates drawn in order, the near-singular ones passed over
        bad = np.flatnonzero(~(margin(x, nup, ndn, d, tu, td, ws) > MARGIN))
        if not len(bad):
            break
        x[bad] = rng.normal(size=(len(bad), n, d)) * 1.2
    assert (margin(x, nup, ndn, d, tu, td, ws) > MARGIN).all()
    lp, g, lap = K.logprob(x, nup, ndn, tu, td, ws)
    lpo, go, lapo = (O.logprob if d == 2 else O.logprob3d)(x, nup, ndn, tab_up=tu, tab_dn=td, wstate=ws)
    print(f"ELOCSTATES logprob {nup}+{ndn} d={d}: logp abs {np.abs(lp - lpo).max():.2e} (bar 1e-11)  grad {(np.abs(g - go) / (1.0 + np.abs(go))).max():.2e} "
          f"of 1 + |grad| (bar 1e-9)  lap {(np.abs(lap - lapo) / (1e3 + np.abs(lapo))).max():.2e} of 1e3 + |lap| (bar 1e-9)")
    np.testing.assert_allclose(lp, lpo, rtol=0, atol=1e-11)
    np.testing.assert_allclose(g, go, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(lap, lapo, rtol=1e-9, atol=1e-6)
    lp0 = K.logprob(x, nup, ndn, tu, td, np.zeros(B, dtype=np.int32))[0]
    assert (np.abs(lp - lp0)[ws != 0] > 1e-3 * np.abs(lp)[ws != 0]).mean() > 0.9      # the state is honoured


# ---------------------------------------------------------------------------------------------------------------- backends
def gpu_backend():
    import torch
    from fermiflow_amd import native
    from tests.common import N, T, cu_count, make_flow
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    tab = lambda t, k: None if k == 0 else native.orbital_table(list(range(k)) if t is None else np.asarray(t).tolist(), dev)

    class K:
        name = "gpu"

        @staticmethod
        def net(eta, mu, table):
            return make_flow(eta, mu, dev).v_wrapper.v.net(radial="table" if table else "exact")

        @staticmethod
        def plan(n, d):
            return native.kernel_plan("eloc", n, d, cu_count())[0]

        @staticmethod
        def cus():
            return cu_count()

        @staticmethod
        def eloc(net, x, nup, ndn, tu, td, ws, order=None, compact=False, two_pass=False, wide=False, route=None):
            i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(dev) if a is not None else None
            kw = dict(walker_class=i32(route[0]), heavy_class=int(route[1]), sens_tol=1.0, sens_tol_class=0) if route is not None else {}
            prev = native.set_kernel_family(1) if wide else None
            try:
                r = native.eloc(tab(tu, nup), tab(td, ndn), nup, ndn, net, T(x, dev), 0.0, 1.0, 1e-9, 1e-11, Z, True, walker_state=i32(ws),
                                want_stats=True, walker_order=i32(order), compact=compact, two_pass=two_pass, **kw)
                torch.cuda.synchronize()
            finally:
                if wide:
                    native.set_kernel_family(prev)
            return {k: N(v) for k, v in r.items()}

        @staticmethod
        def logprob(x, nup, ndn, tu, td, ws):
            fn = native.logprob if x.shape[2] == 2 else native.logprob3d
            return tuple(N(v) for v in fn(tab(tu, nup), tab(td, ndn), nup, ndn, T(x, dev),
                                          walker_state=torch.as_tensor(ws, dtype=torch.int32).to(dev), derivs=True))
    return K


def sim_backend():
    from fermiflow_amd import native
    from tests.hostsim import simlib as S
    nets = {}

    class K:
        name = "sim"

        @staticmethod
        def net(eta, mu, table):      # (a simulated build of the radial table takes seconds: one per set of weights)
            key = (b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in list(eta) + list(mu or [])), mu is None, table)
            if key not in nets:
                nets[key] = S.Net(eta, mu, table=table)
            return nets[key]

        @staticmethod
        def plan(n, d):
            return native.PLAN_FAMILIES[S.kernel_plan(native.PLAN_CALLS.index("eloc"), n, d, 2)[0]]

        @staticmethod
        def cus():
            return 2

        @staticmethod
        def eloc(net, x, nup, ndn, tu, td, ws, order=None, compact=False, two_pass=False, wide=False, route=None):
            prev = S.lib().ff_set_kernel_family(1) if wide else None
            if route is not None:
                S.warm(wclass=np.ascontiguousarray(route[0], dtype=np.int32), sens_tol=1.0, sens_class=0, heavy_class=int(route[1]))
            try:
                return S.eloc_nd(x, nup, ndn, net, Z, rtol=1e-9, atol=1e-11, tab_up=tu, tab_dn=td, wstate=ws, compact=compact, order=order,
                                 two_pass=two_pass)
            finally:
                S.warm()
                if wide:
                    S.lib().ff_set_kernel_family(prev)

        @staticmethod
        def logprob(x, nup, ndn, tu, td, ws):
            return (S.logprob if x.shape[2] == 2 else S.logprob3d)(x, nup, ndn, tab_up=tu, tab_dn=td, wstate=ws)
    return K


def run_named(K, name):
    if name.startswith("F6-"):
        run_routed(K, *(int(v) for v in name[3:].split("+")))
    elif name == "F5-6+6-loop":
        run_looping(K)
    elif name == "F5-4+3-common":
        run_common_table(K)
    else:
        run_case(K, name)


def digest(K, name):
    """SHA-256 of the outputs of ONE launch of a case (five walkers, one-body net, radial table): what the kernel of this process gives"""
    import hashlib
    _, nup, ndn, d, how, _ = CASES[name]
    eta, mu, x, _ = inputs(name, nup, ndn, d)
    tu, td = tables(nup, ndn, d, name)
    r = K.eloc(K.net(eta, mu, True), x[:5], nup, ndn, tu, td, WS[:5])
    assert int(r["stats"][3]) == 0
    return hashlib.sha256(b"".join(_bits(r[k]).tobytes() for k in KEYS)).hexdigest()


def run_child(backend, name, timeout=600, kernel="mfma", what="case"):
    """The case (or, what="digest", the digest of one launch of it) in a child process with FF_ELOC_KERNEL=kernel; its report is
    printed, a failed assertion in it fails the caller; returns the digest line's value"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "tests.eloc_states_cases", backend, name, what], cwd=root,
                       env=dict(os.environ, FF_ELOC_KERNEL=kernel), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode()
    print(out)
    assert p.returncode == 0, out[-4000:]
    assert out.strip().splitlines()[-1] == "ELOCSTATES done", out[-2000:]
    dg = [l.split()[-1] for l in out.splitlines() if l.startswith("ELOCSTATES DIGEST")]
    return dg[-1] if dg else None


def forced_kernel_ran(backend, name, timeout=600):
    """The case in a child forced to the matrix-core kernel, and the proof that this kernel ran.  ff_kernel_plan reports the default
    routing whatever FF_ELOC_KERNEL says, so the plan cannot show it; the arithmetic can: one launch of the case gives the same bits
    twice in the matrix-core child, and other bits in a child forced to the column sweep (instantiated at every shape of F1:
    FF_ELOC_COLUMNS, csrc/ff_plan.h)."""
    a = run_child(backend, name, timeout, "mfma", "case")
    c = run_child(backend, name, timeout, "columns", "digest")
    assert a is not None and c is not None and a != c, (name, a, c)


if __name__ == "__main__":
    K_ = gpu_backend() if sys.argv[1] == "gpu" else sim_backend()
    if len(sys.argv) > 3 and sys.argv[3] == "digest":
        print("ELOCSTATES DIGEST", digest(K_, sys.argv[2]))
    else:
        run_named(K_, sys.argv[2])
        if sys.argv[2] in CASES:
            dg = digest(K_, sys.argv[2])
            assert dg == digest(K_, sys.argv[2]), "the launch does not reproduce its own bits"
            print("ELOCSTATES DIGEST", dg)
    print("ELOCSTATES done")
