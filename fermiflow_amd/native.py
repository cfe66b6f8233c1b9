"""Tensor-level wrappers over the C ABI (include/fermiflow.h).  Every function takes/returns fp64 CUDA
tensors, enqueues on torch's current stream and never synchronises."""
import ctypes as C
import os

import torch

from . import _lib as L


_TABLES = {}   # (orbital indices, device) -> device table; a host->device copy is a synchronisation point, so tables
               # are uploaded once (they are a few integers that never change for a model)


def orbital_table(idx, device):
    """int32 device table [n_states, n_spin] from a (list of) orbital index list(s); cached per device."""
    t = torch.as_tensor(idx, dtype=torch.int32)
    if t.dim() == 1:
        t = t[None]
    key = (tuple(t.shape), tuple(t.reshape(-1).tolist()), str(torch.device(device)))
    tab = _TABLES.get(key)
    if tab is None:
        if len(_TABLES) > 256:
            _TABLES.clear()
        tab = _TABLES[key] = t.contiguous().to(device)
    return tab


def set_kernel_family(family):
    """ff_set_kernel_family: 0 = by particle number (default), 1 = one walker per workgroup for every particle number.
    Returns the previous setting."""
    return int(L.lib().ff_set_kernel_family(int(family)))


PLAN_CALLS = ("flow", "flow_fb", "eloc", "eloc_fb", "adjoint", "adj_fb")                                   # FF_CALL_* (include/fermiflow.h)
PLAN_FAMILIES = (None, "columns", "split", "rows", "mfma", "wide", "narrow", "tabulated", "direct")      # FF_FAMILY_*


def kernel_plan(call, n, dim, cus=256):
    """ff_kernel_plan: (family, walkers per group, walkers per round of the grid at `cus` compute units; 0: the grid never loops) of
    the kernel the library's default routing gives `call` (one of PLAN_CALLS; "_fb": the direct kernel behind the table kernel) at
    n particles in `dim` dimensions.  A pure function of its arguments: no GPU needed.  NotImplementedError for a shape no kernel serves."""
    out = L.FFKernelPlanInfo()
    L.check(L.lib().ff_kernel_plan(PLAN_CALLS.index(call), int(n), int(dim), int(cus), C.byref(out)), "ff_kernel_plan")
    return PLAN_FAMILIES[out.family], int(out.group), int(out.round)


def set_sens_precision(bits):
    """ff_set_sens_precision: 64 (default) or 32 = single-precision sensitivity matrices in the matrix-core local-energy kernel
    (11 particles and more).  Returns the previous setting."""
    return int(L.lib().ff_set_sens_precision(int(bits)))


def _state(ws):
    return None if ws is None else L.dev(ws, torch.int32, "walker_state")


def slater_fwd(table, x, walker_state=None):
    x = L.dev(x, name="x")
    B, n = x.shape[0], x.shape[1]
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    L.check(L.lib().ff_slater_logabsdet_fwd(L.stream(), B, n, L.ptr(table), L.ptr(_state(walker_state)), L.ptr(x), L.ptr(out)), "ff_slater_logabsdet_fwd")
    return out


def slater_bwd(table, x, grad_out, walker_state=None):
    x = L.dev(x, name="x"); go = L.dev(grad_out, name="grad_out")
    B, n = x.shape[0], x.shape[1]
    gx = torch.empty_like(x)
    L.check(L.lib().ff_slater_logabsdet_bwd(L.stream(), B, n, L.ptr(table), L.ptr(_state(walker_state)), L.ptr(x),
                                            L.ptr(go), L.ptr(gx)), "ff_slater_logabsdet_bwd")
    return gx


def logprob(tab_up, tab_dn, nup, ndn, x, walker_state=None, derivs=False):
    x = L.dev(x, name="x")
    B = x.shape[0]
    logp = torch.empty(B, dtype=torch.float64, device=x.device)
    grad = torch.empty_like(x) if derivs else None
    lap = torch.empty(B, dtype=torch.float64, device=x.device) if derivs else None
    L.check(L.lib().ff_logprob(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)),
                               L.ptr(x), L.ptr(logp), L.ptr(grad), L.ptr(lap)), "ff_logprob")
    return (logp, grad, lap) if derivs else logp


def mcmc_sample(tab_up, tab_dn, nup, ndn, B, steps, tau, seed, device, walker_offset=0, walker_state=None):
    n = nup + ndn
    x = torch.empty(B, n, 2, dtype=torch.float64, device=device)
    logp = torch.empty(B, dtype=torch.float64, device=device)
    cnt = torch.empty(B, dtype=torch.int32, device=device)
    L.check(L.lib().ff_mcmc_sample(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), int(steps), tau,
                                   int(seed) & (2**64 - 1), int(walker_offset), L.ptr(x), L.ptr(logp), L.ptr(cnt)), "ff_mcmc_sample")
    return x, logp, cnt


def mcmc_continue(tab_up, tab_dn, nup, ndn, x_init, steps, tau, seed, walker_offset=0, walker_state=None):
    """ff_mcmc_continue: `steps` more Metropolis steps from the walkers x_init (B,n,2)."""
    x0 = L.dev(x_init, name="x_init")
    B = x0.shape[0]
    x = torch.empty_like(x0)
    logp = torch.empty(B, dtype=torch.float64, device=x0.device)
    cnt = torch.empty(B, dtype=torch.int32, device=x0.device)
    L.check(L.lib().ff_mcmc_continue(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), int(steps), tau,
                                     int(seed) & (2**64 - 1), int(walker_offset), L.ptr(x0), L.ptr(x), L.ptr(logp), L.ptr(cnt)), "ff_mcmc_continue")
    return x, logp, cnt


def mcmc_sample_noise(tab_up, tab_dn, nup, ndn, g0, g, u, tau=0.1, walker_state=None):
    g0, g, u = L.dev(g0, name="g0"), L.dev(g, name="g"), L.dev(u, name="u")
    B, steps = g0.shape[0], g.shape[0]
    x = torch.empty_like(g0)
    logp = torch.empty(B, dtype=torch.float64, device=g0.device)
    acc = torch.empty(steps, B, dtype=torch.uint8, device=g0.device)
    L.check(L.lib().ff_mcmc_sample_noise(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), int(steps), tau, L.ptr(g0),
                                         L.ptr(g), L.ptr(u), L.ptr(x), L.ptr(logp), L.ptr(acc)), "ff_mcmc_sample_noise")
    return x, logp, acc


def rng_fill(B, n, steps, seed, device, walker_offset=0, dim=2):
    """the noise ff_mcmc_sample (dim = 2) / ff_mcmc_sample3d (dim = 3) consume for these walkers, materialised"""
    g0 = torch.empty(B, n, dim, dtype=torch.float64, device=device)
    g = torch.empty(steps, B, n, dim, dtype=torch.float64, device=device)
    u = torch.empty(steps, B, dtype=torch.float64, device=device)
    fn, name = (L.lib().ff_rng_fill, "ff_rng_fill") if dim == 2 else (L.lib().ff_rng_fill3d, "ff_rng_fill3d")
    L.check(fn(L.stream(), B, n, int(steps), int(seed) & (2**64 - 1), int(walker_offset), L.ptr(g0), L.ptr(g), L.ptr(u)), name)
    return g0, g, u


def mlp_eval(w1, b1, w2, r, need_grad=True):
    r = L.dev(r, name="r")
    w1, b1, w2 = L.dev(w1.reshape(-1)), L.dev(b1), L.dev(w2.reshape(-1))
    val = torch.empty_like(r)
    dval = torch.empty_like(r) if need_grad else None
    L.check(L.lib().ff_mlp_eval(L.stream(), r.numel(), b1.numel(), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(r), L.ptr(val), L.ptr(dval)), "ff_mlp_eval")
    return val, dval


def mlp_eval_nd(w1, b1, w2, x, need_val=True, need_grad=False):
    """ff_mlp_eval_nd: x (N, D_in) -> val (N), grad (N, D_in)."""
    x = L.dev(x, name="x")
    N, Din = x.shape
    w1, b1, w2 = L.dev(w1.reshape(-1, Din)), L.dev(b1), L.dev(w2.reshape(-1))
    val = torch.empty(N, dtype=torch.float64, device=x.device) if need_val else None
    grad = torch.empty_like(x) if need_grad else None
    L.check(L.lib().ff_mlp_eval_nd(L.stream(), N, int(Din), b1.numel(), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(x), L.ptr(val), L.ptr(grad)), "ff_mlp_eval_nd")
    return val, grad


def backflow_vjp(net, x, w=None, need_gdiv=False):
    """ff_backflow_vjp: ((dv/dx)^T w or None, grad_x div v or None)."""
    x = L.dev(x, name="x")
    B, n, d = x.shape
    w = L.dev(w, name="w") if w is not None else None
    Aw = torch.empty_like(x) if w is not None else None
    gd = torch.empty_like(x) if need_gdiv else None
    L.check(L.lib().ff_backflow_vjp(L.stream(), B, n, d, net.ref(), L.ptr(x), L.ptr(w), L.ptr(Aw), L.ptr(gd)), "ff_backflow_vjp")
    return Aw, gd


def backflow_v_div(net, x, need_v=True, need_div=True):
    x = L.dev(x, name="x")
    B, n, d = x.shape
    v = torch.empty_like(x) if need_v else None
    div = torch.empty(B, dtype=torch.float64, device=x.device) if need_div else None
    L.check(L.lib().ff_backflow_v_div(L.stream(), B, n, d, net.ref(), L.ptr(x), L.ptr(v), L.ptr(div)), "ff_backflow_v_div")
    return v, div


def potential(x, Z, use_ho):
    x = L.dev(x, name="x")
    B, n, d = x.shape
    V = torch.empty(B, dtype=torch.float64, device=x.device)
    L.check(L.lib().ff_potential(L.stream(), B, n, d, Z, int(bool(use_ho)), L.ptr(x), L.ptr(V)), "ff_potential")
    return V


def _stats(device, want):
    # [0..3] stats, [8..] diagnostic stamps (FF_STAMPS builds; FF_STATS_WORDS makes room for their per-workgroup trace)
    return torch.zeros(int(os.environ.get("FF_STATS_WORDS", "32")), dtype=torch.int32, device=device) if want else None


def cnf_generate(net, z, t0, t1, rtol, atol, want_stats=False, walker_cost=None, walker_order=None, **warm):
    z = L.dev(z, name="z")
    B, n, d = z.shape
    x = torch.empty_like(z)
    st = _stats(z.device, want_stats)
    o = L.ode(t0, t1, rtol, atol, walker_cost=walker_cost, walker_order=walker_order, **warm)
    L.check(L.lib().ff_cnf_generate(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(z), L.ptr(x), L.ptr(st)), "ff_cnf_generate")
    return (x, st) if want_stats else x


def cnf_generate_frames(net, z, nframes, t0, t1, rtol, atol, walker_cost=None, walker_order=None, **warm):
    """ff_cnf_generate_frames: (frames (nframes, B, n, d) at torch.linspace(t0, t1, nframes) with frames[0] = z, stats) --
    one integration that lands on every frame time (csrc/ff_ode.h, ff_frame_stepper)."""
    z = L.dev(z, name="z")
    B, n, d = z.shape
    nframes = int(nframes)
    frames = torch.empty((max(nframes, 1), B, n, d), dtype=torch.float64, device=z.device)
    st = _stats(z.device, True)
    o = L.ode(t0, t1, rtol, atol, walker_cost=walker_cost, walker_order=walker_order, **warm)
    L.check(L.lib().ff_cnf_generate_frames(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(z), nframes, L.ptr(frames), L.ptr(st)), "ff_cnf_generate_frames")
    return frames, st


def cnf_delta_logp(net, x, t0, t1, rtol, atol, want_stats=False, walker_cost=None, walker_order=None, **warm):
    x = L.dev(x, name="x")
    B, n, d = x.shape
    z = torch.empty_like(x)
    dl = torch.empty(B, dtype=torch.float64, device=x.device)
    st = _stats(x.device, want_stats)
    o = L.ode(t0, t1, rtol, atol, walker_cost=walker_cost, walker_order=walker_order, **warm)
    L.check(L.lib().ff_cnf_delta_logp(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(x), L.ptr(z), L.ptr(dl), L.ptr(st)), "ff_cnf_delta_logp")
    return (z, dl, st) if want_stats else (z, dl)


def cnf_adjoint(net, y_start, a_z, a_d, t_from, t_to, rtol, atol, need_gx=True, want_stats=False, walker_cost=None,
                walker_order=None, energy=None, **warm):
    """Adjoint sweep from t_from (where y_start, a_z, a_d are given) to t_to.
    energy = (eloc (B,), e_mean device tensor, scale[, mean_index int32 (B,)]): ff_cnf_adjoint_energy -- a_z is glogp0
    (B,n,d) and the kernel forms the seeds w_b * glogp0[b], -w_b with w_b = (eloc[b] - e_mean[mean_index[b] or 0]) * scale
    itself (a_d is ignored)."""
    y = L.dev(y_start, name="y_start"); a_z = L.dev(a_z, name="a_z")
    if energy is None:
        a_d = L.dev(a_d, name="a_d")
    B, n, d = y.shape
    gx = torch.empty_like(y) if need_gx else None
    gp = torch.empty(net.nparams, dtype=torch.float64, device=y.device)
    nbytes = L.lib().ff_cnf_adjoint_workspace_bytes(B, n, d, net.He, net.Hm)
    ws = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=y.device)
    st = _stats(y.device, want_stats)
    o = L.ode(t_from, t_to, rtol, atol, walker_cost=walker_cost, walker_order=walker_order, **warm)
    if energy is not None:
        e = L.dev(energy[0], name="eloc")
        mi = L.dev(energy[3], torch.int32, "mean_index") if len(energy) > 3 and energy[3] is not None else None
        em = L.dev(energy[1].reshape(-1) if mi is not None else energy[1].reshape(-1)[:1], name="e_mean")
        L.check(L.lib().ff_cnf_adjoint_energy(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(y), L.ptr(a_z), L.ptr(e), L.ptr(em),
                                              L.ptr(mi), energy[2], L.ptr(gx), L.ptr(gp), L.ptr(ws), L.ptr(st)), "ff_cnf_adjoint_energy")
    else:
        L.check(L.lib().ff_cnf_adjoint(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(y), L.ptr(a_z), L.ptr(a_d),
                                       L.ptr(gx), L.ptr(gp), L.ptr(ws), L.ptr(st)), "ff_cnf_adjoint")
    return (gx, gp, st) if want_stats else (gx, gp)


def cnf_adjoint_scores(net, z_t0, glogp0, t_from, t_to, rtol, atol, want_stats=False, walker_order=None, **warm):
    """ff_cnf_adjoint_scores: the per-walker log-derivatives (B, 3He+3Hm) of walkers whose flow ends in z_t0 with
    glogp0 = grad_z logp0(z_t0) (both as native.eloc returns them).  NotImplementedError outside the narrow adjoint's shapes."""
    z = L.dev(z_t0, name="z_t0"); g0 = L.dev(glogp0, name="glogp0")
    B, n, d = z.shape
    scores = torch.empty((B, net.nparams), dtype=torch.float64, device=z.device)
    st = _stats(z.device, want_stats)
    o = L.ode(t_from, t_to, rtol, atol, walker_order=walker_order, **warm)
    L.check(L.lib().ff_cnf_adjoint_scores(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(z), L.ptr(g0), L.ptr(scores), None,      # (no workspace: include/fermiflow.h)
                                          L.ptr(st)), "ff_cnf_adjoint_scores")
    return (scores, st) if want_stats else scores


def _cached_ws(cache, cap, alloc, device, sizes, nbytes):
    """(key, workspace): the fp64 workspace `cache` holds for (device, the current stream of device, *sizes) -- a workspace belongs to
    the stream its calls run on --, made by `alloc` (torch.zeros / torch.empty) from the size query `nbytes` (a callable) on a miss;
    a cache that has grown past `cap` entries is emptied first."""
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream), *sizes)
    ws = cache.get(key)
    if ws is None:
        if len(cache) > cap:
            cache.clear()
        ws = cache[key] = alloc(max(1, nbytes() // 8), dtype=torch.float64, device=device)
    return key, ws


_SR_WS = {}      # (device, stream, B, P[, nstates]) -> workspace of ff_sr_moments / ff_sr_state_* (partial tiles; written in full by every call)


def sr_moments(scores, eloc, e_mean):
    """ff_sr_moments: the raw sums [S_raw (P*P) | o_sum (P) | g_sum (P) | sum(e - E) | B] of scores (B, P) -- all-reduce them,
    then sr_finish.  e_mean: device tensor whose first element is E."""
    scores = L.dev(scores, name="scores"); e = L.dev(eloc, name="eloc"); em = L.dev(e_mean.reshape(-1)[:1], name="e_mean")
    B, P = scores.shape
    ws = _cached_ws(_SR_WS, 16, torch.empty, scores.device, (B, P), lambda: L.lib().ff_sr_moments_workspace_bytes(B, P))[1]
    sums = torch.empty(P * P + 2 * P + 2, dtype=torch.float64, device=scores.device)
    L.check(L.lib().ff_sr_moments(L.stream(), B, P, L.ptr(scores), L.ptr(e), L.ptr(em), L.ptr(sums), L.ptr(ws)), "ff_sr_moments")
    return sums


def sr_finish(sums, P):
    """ff_sr_finish: (fisher (P, P), obar (P), grad (P)) from the (all-reduced) sums of sr_moments."""
    sums = L.dev(sums, name="sums")
    P = int(P)
    f = dict(dtype=torch.float64, device=sums.device)
    fisher, obar, grad = torch.empty((P, P), **f), torch.empty(P, **f), torch.empty(P, **f)
    L.check(L.lib().ff_sr_finish(L.stream(), P, L.ptr(sums), L.ptr(fisher), L.ptr(obar), L.ptr(grad)), "ff_sr_finish")
    return fisher, obar, grad


def sr_state_moments(scores, eloc, walker_state, mean_e, nstates):
    """ff_sr_state_moments: the raw sums [S_raw (P*P) | o_state (nstates*P) | g_sum (P) | c_state (nstates)] of scores (B, P) whose
    walkers are in the many-body states walker_state (int32, SORTED ascending); g_sum = sum_b O_b (eloc[b] - mean_e[state_b]) --
    all-reduce them, then sr_state_finish."""
    scores = L.dev(scores, name="scores"); e = L.dev(eloc, name="eloc"); me = L.dev(mean_e, name="mean_e")
    st = L.dev(walker_state, torch.int32, "walker_state")
    B, P = scores.shape
    ns = int(nstates)
    ws = _sr_state_ws(scores.device, B, P, ns)
    sums = torch.empty(P * P + ns * P + P + ns, dtype=torch.float64, device=scores.device)
    L.check(L.lib().ff_sr_state_moments(L.stream(), B, P, ns, L.ptr(scores), L.ptr(e), L.ptr(st), L.ptr(me), L.ptr(sums), L.ptr(ws)), "ff_sr_state_moments")
    return sums


def _sr_state_ws(device, B, P, nstates):
    return _cached_ws(_SR_WS, 16, torch.empty, device, (B, P, nstates), lambda: L.lib().ff_sr_state_moments_workspace_bytes(B, P, nstates))[1]


def sr_state_finish(sums, P, nstates):
    """ff_sr_state_finish: (fisher (P, P), obar_state (nstates, P), grad (P)) from the (all-reduced) sums of sr_state_moments."""
    sums = L.dev(sums, name="sums")
    P, ns = int(P), int(nstates)
    f = dict(dtype=torch.float64, device=sums.device)
    fisher, obar, grad = torch.empty((P, P), **f), torch.empty((ns, P), **f), torch.empty(P, **f)
    ws = _sr_state_ws(sums.device, 0, P, ns)      # (the finish needs no more than the query gives for an empty batch)
    L.check(L.lib().ff_sr_state_finish(L.stream(), P, ns, L.ptr(sums), L.ptr(fisher), L.ptr(obar), L.ptr(grad), L.ptr(ws)), "ff_sr_state_finish")
    return fisher, obar, grad


COMPACT_WORKSPACE_BYTES = 32 << 30     # eloc(compact=None): beyond this many bytes of full workspace, ask for the compact one


def eloc(tab_up, tab_dn, nup, ndn, net, x, t0, t1, rtol, atol, Z, use_ho, walker_state=None, want_stats=False,
         pass1_events=None, walker_cost=None, walker_order=None, two_pass=False, compact=None, **warm):
    """ff_eloc.  pass1_events: optional (start, end) torch.cuda.Event pair recorded around the sensitivity pass
    (bench.py times the dominant kernel with it).  two_pass: ff_eloc_sensitivities + ff_eloc_finish as separate calls with the
    sensitivities in the workspace between them (the path every kernel without a fused finish takes anyway).
    compact: ff_ode::compact_finish -- the one-walker-per-workgroup kernels finish their walkers themselves and the workspace
    beyond 24 coordinates is z(t0) | Delta only; slower by 6-8 % (include/fermiflow.h), so the default (None) asks for it only when
    the full workspace would pass COMPACT_WORKSPACE_BYTES."""
    x = L.dev(x, name="x")
    B, n, d = x.shape[0], nup + ndn, x.shape[2]
    f = dict(dtype=torch.float64, device=x.device)
    M = n * d
    full_bytes = L.lib().ff_eloc_workspace_bytes(B, n, d)
    if compact is None:
        compact = M > 24 and full_bytes > COMPACT_WORKSPACE_BYTES
    if two_pass and compact:
        raise ValueError("two_pass keeps the sensitivities in the workspace: not with compact=True")
    compact_layout = bool(compact) and M > 24       # ff_eloc_nd beyond 24 coordinates: z(t0) | Delta only (include/fermiflow.h)
    nbytes = L.lib().ff_eloc_nd_workspace_bytes(B, n, d, int(bool(compact))) if not two_pass else full_bytes
    ws = torch.empty(max(1, nbytes // 8), **f)
    # z(t0) and Delta stay where the sensitivity pass leaves them: views of the workspace (its documented head, include/fermiflow.h)
    # instead of two device-to-device copies per sweep
    dl0 = B * M if compact_layout else B * (M * M + 4 * M)
    out = dict(logp=torch.empty(B, **f), grad=torch.empty_like(x), lap=torch.empty(B, **f), V=torch.empty(B, **f),
               eloc=torch.empty(B, **f), z=ws[:B * M].view(B, n, d), dlogp=ws[dl0:dl0 + B],
               glogp0=torch.empty_like(x))
    st = _stats(x.device, want_stats)
    o = L.ode(t0, t1, rtol, atol, walker_cost=walker_cost, walker_order=walker_order, compact_finish=bool(compact), **warm)
    if pass1_events is not None:
        pass1_events[0].record()
    if not two_pass:
        # one call: the library fuses the finish into the sensitivity kernel where that kernel implements it (then the second
        # event of pass1_events closes the whole pass)
        L.check(L.lib().ff_eloc_nd(L.stream(), B, nup, ndn, int(d), L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), net.ref(), C.byref(o), Z,
                                   int(bool(use_ho)), L.ptr(x), L.ptr(out["logp"]), L.ptr(out["grad"]), L.ptr(out["lap"]), L.ptr(out["V"]), L.ptr(out["eloc"]),
                                   None, None, L.ptr(out["glogp0"]), L.ptr(ws), L.ptr(st)), "ff_eloc_nd")
        if pass1_events is not None:
            pass1_events[1].record()
    else:
        L.check(L.lib().ff_eloc_sensitivities(L.stream(), B, n, d, net.ref(), C.byref(o), L.ptr(x), L.ptr(ws), L.ptr(st)), "ff_eloc_sensitivities")
        if pass1_events is not None:
            pass1_events[1].record()
        finish = L.lib().ff_eloc_finish3d if d == 3 else L.lib().ff_eloc_finish      # d = 3: HO3D orbital tables (csrc/ff_ho3d.hip)
        L.check(finish(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), Z, int(bool(use_ho)), L.ptr(x), L.ptr(ws),
                       L.ptr(out["logp"]), L.ptr(out["grad"]), L.ptr(out["lap"]), L.ptr(out["V"]), L.ptr(out["eloc"]), None, None, L.ptr(out["glogp0"])),
                "ff_eloc_finish")
    if want_stats:
        out["stats"] = st
    return out


def walker_order(cost, hval=None):
    """ff_walker_order: int32 permutation, most expensive walkers first (cost: int32 per-walker step counts).
    hval (float64, B): ff_walker_order_mean -- returns (order, 1-element tensor mean(hval)) from the same two launches."""
    cost = cost.contiguous()
    if cost.dtype != torch.int32 or not cost.is_cuda:
        raise ValueError("cost must be an int32 device tensor")
    order = torch.empty_like(cost)
    ws = torch.empty(max(1, (L.lib().ff_walker_order_workspace_bytes(cost.numel()) + 7) // 8), dtype=torch.float64, device=cost.device)
    if hval is None:
        L.check(L.lib().ff_walker_order(L.stream(), cost.numel(), L.ptr(cost), L.ptr(order), L.ptr(ws)), "ff_walker_order")
        return order
    hval = L.dev(hval, name="hval")
    hmean = torch.empty(1, dtype=torch.float64, device=cost.device)
    L.check(L.lib().ff_walker_order_mean(L.stream(), cost.numel(), L.ptr(cost), L.ptr(order), L.ptr(ws), L.ptr(hval), L.ptr(hmean)), "ff_walker_order_mean")
    return order, hmean


def walker_schedule(cost, hval, scale_in, scale_out, prev=None, interval=0.0, counts=None, shrink_at=0.0):
    """ff_walker_schedule: (order, mean(hval) as a 1-element tensor, hs) with hs[b] = hval[b] * scale_in[cost[b]] -- the step every walker's
    local-energy pass opens with; scale_out receives the table updated from the previous pass prev = (cost, hs, he) (None: copied)."""
    cost = cost.contiguous()
    if cost.dtype != torch.int32 or not cost.is_cuda:
        raise ValueError("cost must be an int32 device tensor")
    hval = L.dev(hval, name="hval")
    order = torch.empty_like(cost)
    hs = torch.empty_like(hval)
    hmean = torch.empty(1, dtype=torch.float64, device=cost.device)
    ws = torch.empty(max(1, (L.lib().ff_walker_order_workspace_bytes(cost.numel()) + 7) // 8), dtype=torch.float64, device=cost.device)
    pc, ph, pe = prev if prev is not None else (None, None, None)
    if prev is not None and not (pc.numel() == ph.numel() == pe.numel() == cost.numel()):
        raise ValueError("walker_schedule: the previous pass must have this call's batch size")
    if counts is not None and not (counts.numel() == SCALE_COUNTS and counts.dtype == torch.float64 and counts.is_contiguous()
                                   and counts.is_cuda and counts.device == cost.device):
        raise ValueError(f"walker_schedule: counts must be the {SCALE_COUNTS} doubles of scale_counts, contiguous, on the walkers' device")
    L.check(L.lib().ff_walker_schedule(L.stream(), cost.numel(), L.ptr(cost), L.ptr(order), L.ptr(ws), L.ptr(hval), L.ptr(hmean), L.ptr(scale_in),
                                       L.ptr(scale_out), L.ptr(pc), L.ptr(ph), L.ptr(pe), L.ptr(counts), abs(float(interval)), L.ptr(hs), shrink_at),
            "ff_walker_schedule")
    return order, hmean, hs


SCALE_COUNTS = 128      # doubles of ff_scale_counts / ff_walker_schedule's prev_counts (include/fermiflow.h)


def scale_counts(cost, hs, he, interval=0.0):
    """ff_scale_counts: 128 doubles [walkers by cost class | of them, first step rejected | planned for >= 3 equal steps of `interval` | of
    those, accepted a step of the plan one shorter] of a local-energy pass (this rank's shard)"""
    counts = torch.zeros(SCALE_COUNTS, dtype=torch.float64, device=cost.device)
    L.check(L.lib().ff_scale_counts(L.stream(), cost.numel(), L.ptr(cost), L.ptr(hs), L.ptr(he), abs(float(interval)), L.ptr(counts)), "ff_scale_counts")
    return counts


def reduce_moments(e, shift=0.0, shift_dev=None, shift_dev_scale=1.0, out=None):
    """tensor [sum(e - shift), sum((e - shift)^2)] on the device; shift_dev: optional 1-element device tensor, then
    shift = shift_dev[0] * shift_dev_scale (no host round trip for the mean); out: where to write the two sums."""
    e = L.dev(e, name="e")
    out = torch.empty(2, dtype=torch.float64, device=e.device) if out is None else out
    if shift_dev is not None:
        shift_dev = L.dev(shift_dev.reshape(1), name="shift_dev")
    L.check(L.lib().ff_reduce_moments(L.stream(), e.numel(), L.ptr(e), shift, L.ptr(shift_dev), shift_dev_scale, L.ptr(out)), "ff_reduce_moments")
    return out


def adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step):
    """ff_adam_step: one Adam update of the given fp64 device tensors (lists of equal length) in one launch."""
    n = len(params)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    sizes = (C.c_int64 * n)(*[p.numel() for p in params])
    L.check(L.lib().ff_adam_step(L.stream(), n, sizes, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq), lr, beta1, beta2,
                                 eps, weight_decay, int(step)), "ff_adam_step")


def stream_delay(microseconds):
    """ff_stream_delay on the current stream."""
    L.check(L.lib().ff_stream_delay(L.stream(), microseconds), "ff_stream_delay")


def reduce_energy(e, logp, shift_dev):
    """ff_reduce_energy: tensor [sum(e - c), sum((e - c)^2), sum(logp), sum(logp (e - c))], c = shift_dev[0] (device)."""
    e = L.dev(e, name="e"); logp = L.dev(logp, name="logp"); shift_dev = L.dev(shift_dev.reshape(1), name="shift_dev")
    out = torch.empty(4, dtype=torch.float64, device=e.device)
    L.check(L.lib().ff_reduce_energy(L.stream(), e.numel(), L.ptr(e), L.ptr(logp), L.ptr(shift_dev), L.ptr(out)), "ff_reduce_energy")
    return out


_EST_WS = {}      # (device, stream, B) -> zero-initialised workspace of ff_energy_estimate (its counter is left at zero by every call)


def energy_estimate(e, logp, shift_dev, n_global):
    """ff_energy_estimate: (sums4, est3) in one launch; n_global = 0: sums4 only (est3 is None) -- all-reduce it, then energy_finish."""
    e = L.dev(e, name="e"); logp = L.dev(logp, name="logp"); shift_dev = L.dev(shift_dev.reshape(1), name="shift_dev")
    B = e.numel()
    # the workspace (last-workgroup counter + per-segment partials) is the caller's per call STREAM (include/fermiflow.h): two sweeps on
    # different streams of one device must not share it
    key, ws = _cached_ws(_EST_WS, 64, torch.zeros, e.device, (B,), lambda: L.lib().ff_energy_estimate_workspace_bytes(B))
    sums = torch.empty(4, dtype=torch.float64, device=e.device)
    est = torch.empty(3, dtype=torch.float64, device=e.device) if n_global else None
    try:
        L.check(L.lib().ff_energy_estimate(L.stream(), B, L.ptr(e), L.ptr(logp), L.ptr(shift_dev), int(n_global), L.ptr(sums), L.ptr(est),
                                           L.ptr(ws)), "ff_energy_estimate")
    except Exception:
        _EST_WS.pop(key, None)      # a launch that did not run to its end may have left the counter non-zero: never reuse this workspace
        raise
    return sums, est


def energy_finish(sums4, shift_dev, n_global):
    """ff_energy_finish: tensor [E, sum((e - E)^2), mean(logp (e - E))] from the (all-reduced) sums of reduce_energy."""
    sums4 = L.dev(sums4, name="sums4"); shift_dev = L.dev(shift_dev.reshape(1), name="shift_dev")
    out = torch.empty(3, dtype=torch.float64, device=sums4.device)
    L.check(L.lib().ff_energy_finish(L.stream(), L.ptr(sums4), L.ptr(shift_dev), int(n_global), L.ptr(out)), "ff_energy_finish")
    return out


_ROB_WS = {}      # (device, stream, N) -> zero-initialised workspace of ff_energy_robust / _apply (tickets, selection state and histogram are
                  # left at zero by every call)
ROBUST_STAT = ("n_valid", "E_median", "E_width", "lo", "hi", "E", "E_ss", "E_clipped", "n_clipped", "value")      # stat, include/fermiflow_robust.h


def energy_robust(e, logp, k, shift_dev):
    """ff_energy_robust on a whole batch: stat (10 doubles, ROBUST_STAT; [9] is written by energy_robust_apply).  logp = None: a walker is
    valid where e is finite (the gathered energies of a data-parallel run, invalid walkers marked NaN)."""
    e = L.dev(e, name="e"); shift_dev = L.dev(shift_dev.reshape(1), name="shift_dev")
    logp = L.dev(logp, name="logp") if logp is not None else None
    k = float(k)
    N = e.numel()
    key, ws = _cached_ws(_ROB_WS, 64, torch.zeros, e.device, (N,), lambda: L.lib().ff_energy_robust_workspace_bytes(N))
    stat = torch.empty(L.ROBUST_NSTAT, dtype=torch.float64, device=e.device)
    try:
        L.check(L.lib().ff_energy_robust(L.stream(), N, L.ptr(e), L.ptr(logp), k, L.ptr(shift_dev), L.ptr(stat), L.ptr(ws)), "ff_energy_robust")
    except Exception:
        _ROB_WS.pop(key, None)      # a call that did not run to its end may have left a ticket or the histogram non-zero: never reuse it
        raise
    return stat


def energy_robust_apply(e, logp, stat, n_global, finish=True, z=None, glogp0=None):
    """ff_energy_robust_apply on this rank's shard: (u, sum_out (1,)).  Overwrites IN PLACE the rows of invalid walkers in z / glogp0
    (both or neither) with the documented finite configuration / zeros; finish: stat[9] = sum_out / n_v in the same launch (single rank)."""
    e = L.dev(e, name="e"); logp = L.dev(logp, name="logp"); stat = L.dev(stat, name="stat")
    B = e.numel()
    n = d = 0
    if z is not None:
        z = L.dev(z, name="z"); glogp0 = L.dev(glogp0, name="glogp0")
        if not (z.dim() == 3 and z.shape[0] == B and glogp0.shape == z.shape):
            raise ValueError("energy_robust_apply: z and glogp0 must both be (B, n, d)")
        n, d = z.shape[1], z.shape[2]
    key, ws = _cached_ws(_ROB_WS, 64, torch.zeros, e.device, (B,), lambda: L.lib().ff_energy_robust_workspace_bytes(B))
    u = torch.empty(B, dtype=torch.float64, device=e.device)
    s = torch.empty(1, dtype=torch.float64, device=e.device)
    try:
        L.check(L.lib().ff_energy_robust_apply(L.stream(), B, n, d, L.ptr(e), L.ptr(logp), L.ptr(stat), int(n_global), int(bool(finish)), L.ptr(u),
                                               L.ptr(z), L.ptr(glogp0), L.ptr(s), L.ptr(ws)), "ff_energy_robust_apply")
    except Exception:
        _ROB_WS.pop(key, None)
        raise
    return u, s


def beta_buffer(nstates, device):
    """buffer of ff_beta_state_partials / ff_beta_finish: [0:2] moments of E_loc, [2:] partial per-state sums."""
    return torch.empty(L.lib().ff_beta_buffer_doubles(int(nstates)), dtype=torch.float64, device=device)


def beta_state_partials(e, logp, walker_state, nstates, buf):
    e = L.dev(e, name="e"); logp = L.dev(logp, name="logp"); ws = L.dev(walker_state, torch.int32, "walker_state")
    L.check(L.lib().ff_beta_state_partials(L.stream(), e.numel(), int(nstates), L.ptr(ws), L.ptr(e), L.ptr(logp), L.ptr(buf)), "ff_beta_state_partials")


def beta_finish(buf, shift_dev, logits, beta, n_global):
    """ff_beta_finish: (est8, gphi, mean_e, logp_all) from the all-reduced buffer."""
    logits = L.dev(logits, name="logits"); shift_dev = L.dev(shift_dev.reshape(1), name="shift_dev")
    ns = logits.numel()
    f = dict(dtype=torch.float64, device=buf.device)
    est, gphi, mean_e, lpa = torch.empty(8, **f), torch.empty(ns, **f), torch.empty(ns, **f), torch.empty(ns, **f)
    L.check(L.lib().ff_beta_finish(L.stream(), L.ptr(buf), L.ptr(shift_dev), L.ptr(logits), ns, beta, int(n_global),
                                   L.ptr(est), L.ptr(gphi), L.ptr(mean_e), L.ptr(lpa)), "ff_beta_finish")
    return est, gphi, mean_e, lpa


# ---- one-body density matrix (include/fermiflow_obdm.h, csrc/ff_obdm.h) ---------------------------------
def slater_sign(tab_up, tab_dn, nup, ndn, z, walker_state=None):
    """ff_slater_sign: (B,) the sign of det Phi_up(z) det Phi_dn(z) under the walker's state, in {-1, 0, +1}; NaN for a walker with a
    coordinate that is not finite."""
    z = L.dev(z, name="z")
    B = z.shape[0]
    out = torch.empty(B, dtype=torch.float64, device=z.device)
    L.check(L.lib().ff_slater_sign(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), L.ptr(z), L.ptr(out)),
            "ff_slater_sign")
    return out


def obdm_accumulate(nup, ndn, x, rprime, logp, sign, logp_moved, sign_moved, sigma, nshells, acc, workspace):
    """ff_obdm_accumulate: one call = one block of the accumulator `acc` (int64 words, include/fermiflow_obdm.h); `workspace`: fp64
    scratch of at least ff_obdm_workspace_bytes(B, nshells) bytes."""
    x = L.dev(x, name="x")
    B, n = x.shape[0], nup + ndn
    t = [L.dev(v, name=k) for k, v in (("rprime", rprime), ("logp", logp), ("sign", sign), ("logp_moved", logp_moved), ("sign_moved", sign_moved))]
    for v, shape, k in zip([x] + t, ((B, n, 2), (B, 2, 2), (B,), (B,), (B, n), (B, n)), ("x", "rprime", "logp", "sign", "logp_moved", "sign_moved")):
        if tuple(v.shape) != shape:
            raise ValueError(f"obdm_accumulate: {k} must be {shape}, got {tuple(v.shape)}")
    need = L.lib().ff_obdm_workspace_bytes(B, int(nshells))
    if need and workspace.numel() * 8 < need:
        raise ValueError(f"obdm_accumulate: workspace of {workspace.numel() * 8} bytes, {need} needed")
    L.check(L.lib().ff_obdm_accumulate(L.stream(), B, nup, ndn, L.ptr(x), *[L.ptr(v) for v in t], float(sigma), int(nshells),
                                       L.ptr(L.dev(acc, torch.int64, "acc")), L.ptr(L.dev(workspace, name="workspace"))), "ff_obdm_accumulate")


# ---- energy components (include/fermiflow_energy.h, csrc/ff_energy_parts.h) -----------------------------
def energy_parts_accumulate(nup, ndn, Z, x, grad, lap, walker_state, nstates, centre, parts_out, acc, workspace):
    """ff_energy_parts_accumulate: one call = one block of the accumulator `acc` (int64 words, include/fermiflow_energy.h).  x, grad
    (B, n, d) and lap (B) as eloc() leaves them; walker_state: sorted int32 (B) with nstates > 0, else None; centre: 6 doubles on the
    device or None; parts_out: (B, 6) or None; `workspace`: fp64 scratch of at least ff_energy_parts_workspace_bytes(B, nstates) bytes."""
    x = L.dev(x, name="x")
    B, n, d = x.shape[0], nup + ndn, x.shape[2]
    grad, lap = L.dev(grad, name="grad"), L.dev(lap, name="lap")
    for v, shape, k in ((x, (B, n, d), "x"), (grad, (B, n, d), "grad"), (lap, (B,), "lap")):
        if tuple(v.shape) != shape:
            raise ValueError(f"energy_parts_accumulate: {k} must be {shape}, got {tuple(v.shape)}")
    ws = None
    if int(nstates) > 0:
        if walker_state is None:
            raise ValueError("energy_parts_accumulate: nstates > 0 needs walker_state")
        ws = L.dev(_state(walker_state), torch.int32, "walker_state")
        if tuple(ws.shape) != (B,):
            raise ValueError(f"energy_parts_accumulate: walker_state must be ({B},), got {tuple(ws.shape)}")
    if centre is not None:
        centre = L.dev(centre, name="centre")
        if centre.numel() != 6:
            raise ValueError("energy_parts_accumulate: centre must hold 6 doubles")
    if parts_out is not None and not (parts_out.is_cuda and parts_out.dtype == torch.float64 and parts_out.is_contiguous() and tuple(parts_out.shape) == (B, 6)):
        raise ValueError(f"energy_parts_accumulate: parts_out must be a contiguous fp64 device tensor ({B}, 6)")
    need = L.lib().ff_energy_parts_workspace_bytes(B, int(nstates))
    if need and workspace.numel() * 8 < need:
        raise ValueError(f"energy_parts_accumulate: workspace of {workspace.numel() * 8} bytes, {need} needed")
    L.check(L.lib().ff_energy_parts_accumulate(L.stream(), B, nup, ndn, int(d), float(Z), L.ptr(x), L.ptr(grad), L.ptr(lap), L.ptr(ws), int(nstates),
                                               L.ptr(centre), L.ptr(parts_out), L.ptr(L.dev(acc, torch.int64, "acc")),
                                               L.ptr(L.dev(workspace, name="workspace"))), "ff_energy_parts_accumulate")


# ---- fixed-node diffusion Monte Carlo (include/fermiflow_dmc.h, csrc/ff_dmc.h) ---------------------------
DMC_REC = L.DMC_REC      # 8-byte words of a step's record
_DMC_STATE = ("x", "logp", "grad", "eloc", "sign")


def _dmc_fields(who, d, B, n, names=_DMC_STATE):
    out = []
    for k in names:
        v = L.dev(d[k], name=f"{who}[{k}]")
        shape = (B, n, 2) if k in ("x", "grad") else (B,)
        if tuple(v.shape) != shape or v.data_ptr() != d[k].data_ptr():
            raise ValueError(f"{who}[{k}] must be a contiguous fp64 device tensor {shape}, got {tuple(d[k].shape)}")
        out.append(v)
    return out


def dmc_workspaces(B, device):
    """the zeroed workspaces of dmc_accept and dmc_comb for B walkers (their first word is a ticket the kernels leave at zero)"""
    f = dict(dtype=torch.float64, device=device)
    return (torch.zeros(max(1, L.lib().ff_dmc_accept_workspace_bytes(B) // 8), **f),
            torch.zeros(max(1, L.lib().ff_dmc_comb_workspace_bytes(B) // 8), **f))


def dmc_propose(nup, ndn, x, grad, tau, drift_limit, noise=None, seed=0, walker_offset=0, step=0, want_xi=False, out=None):
    """ff_dmc_propose: x' = x + tau vbar + sqrt(tau) xi; (x', xi or None).  noise: explicit normals (B, n, 2), else Philox at
    (seed, walker_offset + b, step)."""
    x, grad = L.dev(x, name="x"), L.dev(grad, name="grad")
    B, n = x.shape[0], nup + ndn
    noise = L.dev(noise, name="noise") if noise is not None else None
    for v, k in ((x, "x"), (grad, "grad")) + (((noise, "noise"),) if noise is not None else ()):
        if tuple(v.shape) != (B, n, 2):
            raise ValueError(f"dmc_propose: {k} must be ({B}, {n}, 2), got {tuple(v.shape)}")
    xn = torch.empty_like(x) if out is None else out
    xi = torch.empty_like(x) if want_xi else None
    L.check(L.lib().ff_dmc_propose(L.stream(), B, nup, ndn, 2, float(tau), float(drift_limit), L.ptr(x), L.ptr(grad),
                                   L.ptr(noise), int(seed), int(walker_offset), int(step), L.ptr(xn),
                                   L.ptr(xi)), "ff_dmc_propose")
    return xn, xi


def dmc_accept(nup, ndn, state, prop, tau, drift_limit, ctrl, rec, step_slot, workspace, u=None, seed=0, walker_offset=0, step=0,
               want_mask=False, groups=0):
    """ff_dmc_accept: state = dict x, logp, grad, eloc, sign, w (overwritten in place), prop = dict x ... sign of the proposals; ctrl: 3
    device doubles (E_T, E_ref, c); rec: int64 or fp64 device words, the record goes to words [9 step_slot, 9 step_slot + 9).
    Returns the uint8 accept mask if asked for."""
    B, n = state["x"].shape[0], nup + ndn
    s = _dmc_fields("state", state, B, n, _DMC_STATE + ("w",))
    q = _dmc_fields("prop", prop, B, n)
    ctrl = L.dev(ctrl, name="ctrl")
    if ctrl.numel() != 3 or rec.element_size() != 8 or not rec.is_cuda or not rec.is_contiguous() or rec.numel() < DMC_REC * (int(step_slot) + 1):
        raise ValueError("dmc_accept: ctrl must hold 3 doubles and rec 9 (step_slot + 1) contiguous 8-byte device words")
    need = L.lib().ff_dmc_accept_workspace_bytes(B)
    if workspace.numel() * 8 < need:
        raise ValueError(f"dmc_accept: workspace of {workspace.numel() * 8} bytes, {need} needed")
    u = L.dev(u, name="u") if u is not None else None
    if u is not None and tuple(u.shape) != (B,):
        raise ValueError(f"dmc_accept: u must be ({B},)")
    mask = torch.empty(B, dtype=torch.uint8, device=s[0].device) if want_mask else None
    L.check(L.lib().ff_dmc_accept(L.stream(), B, nup, ndn, 2, float(tau), float(drift_limit), *[L.ptr(v) for v in s], *[L.ptr(v) for v in q],
                                  L.ptr(u), int(seed), int(walker_offset), int(step), L.ptr(ctrl), L.ptr(rec),
                                  int(step_slot), L.ptr(mask), int(groups), L.ptr(L.dev(workspace, name="workspace"))), "ff_dmc_accept")
    return mask


def dmc_comb(nup, ndn, state, out, src, info, workspace, u0=None, seed=0, step=0):
    """ff_dmc_comb: the state (dict x ... sign, w) resampled into `out` (dict x ... sign, other buffers); state["w"] becomes 1; src int32
    (B) and info int32 (4: distinct sources, largest copy count, flag, 0) are written."""
    B, n = state["x"].shape[0], nup + ndn
    s = _dmc_fields("state", state, B, n, _DMC_STATE + ("w",))
    o = _dmc_fields("out", out, B, n)
    if any(a.data_ptr() == b.data_ptr() for a, b in zip(s, o)):
        raise ValueError("dmc_comb: the output buffers must not be the input buffers")
    src, info = L.dev(src, torch.int32, "src"), L.dev(info, torch.int32, "info")
    if src.numel() != B or info.numel() != 4:
        raise ValueError("dmc_comb: src must hold B and info 4 int32 words")
    need = L.lib().ff_dmc_comb_workspace_bytes(B)
    if workspace.numel() * 8 < need:
        raise ValueError(f"dmc_comb: workspace of {workspace.numel() * 8} bytes, {need} needed")
    L.check(L.lib().ff_dmc_comb(L.stream(), B, nup, ndn, 2, L.ptr(s[5]), *[L.ptr(v) for v in s[:5]], L.ptr(L.dev(u0, name="u0") if u0 is not None else None),
                                int(seed), int(step), L.ptr(src), *[L.ptr(v) for v in o], L.ptr(info), L.ptr(L.dev(workspace, name="workspace"))),
            "ff_dmc_comb")


# ---- d = 3 (csrc/ff_ho3d.hip) ---------------------------------------------------------------------------
def logprob3d(tab_up, tab_dn, nup, ndn, x, walker_state=None, derivs=False):
    x = L.dev(x, name="x")
    B = x.shape[0]
    logp = torch.empty(B, dtype=torch.float64, device=x.device)
    grad = torch.empty_like(x) if derivs else None
    lap = torch.empty(B, dtype=torch.float64, device=x.device) if derivs else None
    L.check(L.lib().ff_logprob3d(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)),
                                 L.ptr(x), L.ptr(logp), L.ptr(grad), L.ptr(lap)), "ff_logprob3d")
    return (logp, grad, lap) if derivs else logp


def mcmc_sample_noise3d(tab_up, tab_dn, nup, ndn, g0, g, u, tau=0.1, walker_state=None):
    g0, g, u = L.dev(g0, name="g0"), L.dev(g, name="g"), L.dev(u, name="u")
    B, steps = g0.shape[0], g.shape[0]
    x = torch.empty_like(g0)
    logp = torch.empty(B, dtype=torch.float64, device=g0.device)
    acc = torch.empty(steps, B, dtype=torch.uint8, device=g0.device)
    L.check(L.lib().ff_mcmc_sample_noise3d(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), int(steps), tau, L.ptr(g0),
                                           L.ptr(g), L.ptr(u), L.ptr(x), L.ptr(logp), L.ptr(acc)), "ff_mcmc_sample_noise3d")
    return x, logp, acc


def mcmc_sample3d(tab_up, tab_dn, nup, ndn, B, steps, tau, seed, device, walker_offset=0, walker_state=None):
    n = nup + ndn
    x = torch.empty(B, n, 3, dtype=torch.float64, device=device)
    logp = torch.empty(B, dtype=torch.float64, device=device)
    cnt = torch.empty(B, dtype=torch.int32, device=device)
    L.check(L.lib().ff_mcmc_sample3d(L.stream(), B, nup, ndn, L.ptr(tab_up), L.ptr(tab_dn), L.ptr(_state(walker_state)), int(steps), tau,
                                     int(seed) & (2**64 - 1), int(walker_offset), L.ptr(x), L.ptr(logp), L.ptr(cnt)), "ff_mcmc_sample3d")
    return x, logp, cnt


def backflow_v_div_f32(net, x):
    """Backflow v and div v with the arithmetic in fp32 (fp64 tensors at the boundary)."""
    x = L.dev(x, name="x")
    B, n, d = x.shape
    v = torch.empty_like(x)
    div = torch.empty(B, dtype=torch.float64, device=x.device)
    L.check(L.lib().ff_backflow_v_div_f32(L.stream(), B, n, d, net.ref(), L.ptr(x), L.ptr(v), L.ptr(div)), "ff_backflow_v_div_f32")
    return v, div
