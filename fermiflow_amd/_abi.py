"""The C ABI of include/fermiflow.h (and of include/fermiflow_robust.h: ROBUST_SIGNATURES; include/fermiflow_maps.h: MAPS_SIGNATURES;
include/fermiflow_obdm.h: OBDM_SIGNATURES; include/fermiflow_energy.h: ENERGY_SIGNATURES; include/fermiflow_dmc.h: DMC_SIGNATURES) as ctypes sees it: its three structs and the
signature of every function, declared once.
fermiflow_amd._lib binds libfermiflow_hip.so to this table and tests/hostsim/simlib.py the host simulator's build of the same sources;
tests/test_host_logic.py holds the table to the header, prototype by prototype.  Imports nothing but ctypes."""
import ctypes as C

ABI_VERSION = 110      # ff_version() of the library this binding was written against (include/fermiflow.h)


class FFNet(C.Structure):
    _fields_ = [("He", C.c_int32), ("ew1", C.c_void_p), ("eb1", C.c_void_p), ("ew2", C.c_void_p),
                ("Hm", C.c_int32), ("mw1", C.c_void_p), ("mb1", C.c_void_p), ("mw2", C.c_void_p),
                ("radial_table", C.c_void_p)]


class FFOde(C.Structure):
    _fields_ = [("t0", C.c_double), ("t1", C.c_double), ("rtol", C.c_double), ("atol", C.c_double),
                ("max_steps", C.c_int32), ("walker_cost", C.c_void_p), ("walker_order", C.c_void_p),
                ("walker_h_init", C.c_void_p), ("walker_h_scale", C.c_double), ("walker_h_out", C.c_void_p),
                ("walker_class", C.c_void_p), ("sens_tol", C.c_double), ("walker_h_scale_loose", C.c_double), ("sens_tol_class", C.c_int32),
                ("walker_h_uniform", C.c_int32), ("heavy_class", C.c_int32), ("heavy_tol", C.c_double), ("sum_weight", C.c_double),
                ("compact_finish", C.c_int32), ("after_main_event", C.c_void_p), ("walker_h_equal", C.c_int32)]


class FFKernelPlanInfo(C.Structure):
    _fields_ = [("family", C.c_int32), ("group", C.c_int32), ("round", C.c_int64)]


def ode_struct(**fields):
    """FFOde with EVERY field given by name (pointer fields: an address or None): a field added to ff_ode cannot shift the values behind
    it in a caller that was not updated, that caller fails here instead."""
    names = {name for name, _ in FFOde._fields_}
    if fields.keys() != names:
        raise TypeError(f"ff_ode fields missing {sorted(names - set(fields))}, unknown {sorted(set(fields) - names)}")
    return FFOde(**fields)


# int -> _I, int64_t -> _Q, uint64_t -> _U, double -> _D, size_t -> _Z; const ff_net* / const ff_ode* / ff_kernel_plan_info* -> a pointer
# to their struct; every other pointer (data, void* stream, ff_comm*, ff_comm**, the pointer arrays of ff_adam_step) -> _P
_I, _Q, _U, _D, _Z, _P = C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_size_t, C.c_void_p
_NET, _ODE, _PLAN = C.POINTER(FFNet), C.POINTER(FFOde), C.POINTER(FFKernelPlanInfo)

SIGNATURES = {      # name: (restype, argtypes), in the header's order; a new line where a section of the header begins
    "ff_version": (_I, ()), "ff_shutdown": (_I, ()),
    "ff_comm_unique_id": (_I, (_P,)), "ff_comm_init": (_I, (_P, _I, _I, _P)), "ff_comm_allreduce": (_I, (_P, _P, _P, _Q)), "ff_comm_destroy": (_I, (_P,)),
    "ff_walker_order_workspace_bytes": (_Z, (_Q,)), "ff_walker_order": (_I, (_P, _Q, _P, _P, _P)), "ff_walker_order_mean": (_I, (_P, _Q, _P, _P, _P, _P, _P)),
    "ff_walker_schedule": (_I, (_P, _Q, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _P, _D)), "ff_scale_counts": (_I, (_P, _Q, _P, _P, _P, _D, _P)),
    "ff_last_error": (C.c_char_p, ()), "ff_set_kernel_family": (_I, (_I,)), "ff_kernel_plan": (_I, (_I, _I, _I, _Q, _PLAN)), "ff_set_sens_precision": (_I, (_I,)),
    "ff_fermion_states": (_Q, (_I, _P, _I, _I, _D, _Q, _P, _P, _P)),
    "ff_slater_logabsdet_fwd": (_I, (_P, _Q, _I, _P, _P, _P, _P)), "ff_slater_logabsdet_bwd": (_I, (_P, _Q, _I, _P, _P, _P, _P, _P)),
    "ff_logprob": (_I, (_P, _Q, _I, _I, _P, _P, _P, _P, _P, _P, _P)),
    "ff_mcmc_sample_noise": (_I, (_P, _Q, _I, _I, _P, _P, _P, _I, _D, _P, _P, _P, _P, _P, _P)),
    "ff_mcmc_sample": (_I, (_P, _Q, _I, _I, _P, _P, _P, _I, _D, _U, _Q, _P, _P, _P)),
    "ff_mcmc_continue": (_I, (_P, _Q, _I, _I, _P, _P, _P, _I, _D, _U, _Q, _P, _P, _P, _P)), "ff_rng_fill": (_I, (_P, _Q, _I, _I, _U, _Q, _P, _P, _P)),
    "ff_mlp_eval": (_I, (_P, _Q, _I, _P, _P, _P, _P, _P, _P)), "ff_backflow_v_div": (_I, (_P, _Q, _I, _I, _NET, _P, _P, _P)),
    "ff_mlp_eval_nd": (_I, (_P, _Q, _I, _I, _P, _P, _P, _P, _P, _P)), "ff_backflow_vjp": (_I, (_P, _Q, _I, _I, _NET, _P, _P, _P, _P)),
    "ff_potential": (_I, (_P, _Q, _I, _I, _D, _I, _P, _P)),
    "ff_radial_table_bytes": (_Z, ()), "ff_radial_table_build": (_I, (_P, _NET, _P)),
    "ff_cnf_generate": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _P, _P)), "ff_cnf_generate_frames": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _I, _P, _P)),
    "ff_cnf_delta_logp": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _P, _P, _P)),
    "ff_cnf_adjoint_workspace_bytes": (_Z, (_Q, _I, _I, _I, _I)), "ff_cnf_adjoint": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _P, _P, _P, _P, _P, _P)),
    "ff_cnf_adjoint_energy": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P)),
    "ff_cnf_adjoint_scores_workspace_bytes": (_Z, (_Q, _I, _I, _I, _I)), "ff_cnf_adjoint_scores": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _P, _P, _P, _P)),
    "ff_sr_moments_workspace_bytes": (_Z, (_Q, _I)), "ff_sr_moments": (_I, (_P, _Q, _I, _P, _P, _P, _P, _P)), "ff_sr_finish": (_I, (_P, _I, _P, _P, _P, _P)),
    "ff_sr_state_moments_workspace_bytes": (_Z, (_Q, _I, _I)), "ff_sr_state_moments": (_I, (_P, _Q, _I, _I, _P, _P, _P, _P, _P, _P)),
    "ff_sr_state_finish": (_I, (_P, _I, _I, _P, _P, _P, _P, _P)),
    "ff_eloc_workspace_bytes": (_Z, (_Q, _I, _I)), "ff_eloc": (_I, (_P, _Q, _I, _I, _P, _P, _P, _NET, _ODE, _D, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P)),
    "ff_eloc_nd_workspace_bytes": (_Z, (_Q, _I, _I, _I)),
    "ff_eloc_nd": (_I, (_P, _Q, _I, _I, _I, _P, _P, _P, _NET, _ODE, _D, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P)),
    "ff_eloc_sensitivities": (_I, (_P, _Q, _I, _I, _NET, _ODE, _P, _P, _P)),
    "ff_eloc_finish": (_I, (_P, _Q, _I, _I, _P, _P, _P, _D, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P)),
    "ff_reduce_moments": (_I, (_P, _Q, _P, _D, _P, _D, _P)), "ff_stream_delay": (_I, (_P, _D)),
    "ff_adam_step": (_I, (_P, _I, _P, _P, _P, _P, _P, _D, _D, _D, _D, _D, _Q)), "ff_reduce_energy": (_I, (_P, _Q, _P, _P, _P, _P)),
    "ff_energy_finish": (_I, (_P, _P, _P, _Q, _P)), "ff_energy_estimate_workspace_bytes": (_Z, (_Q,)),
    "ff_energy_estimate": (_I, (_P, _Q, _P, _P, _P, _Q, _P, _P, _P)),
    "ff_observe_buffer_bytes": (_Z, (_I,)), "ff_observe_accumulate": (_I, (_P, _Q, _I, _I, _I, _P, _D, _I, _P)),
    "ff_logprob3d": (_I, (_P, _Q, _I, _I, _P, _P, _P, _P, _P, _P, _P)), "ff_mcmc_sample_noise3d": (_I, (_P, _Q, _I, _I, _P, _P, _P, _I, _D, _P, _P, _P, _P, _P, _P)),
    "ff_mcmc_sample3d": (_I, (_P, _Q, _I, _I, _P, _P, _P, _I, _D, _U, _Q, _P, _P, _P)), "ff_rng_fill3d": (_I, (_P, _Q, _I, _I, _U, _Q, _P, _P, _P)),
    "ff_eloc_finish3d": (_I, (_P, _Q, _I, _I, _P, _P, _P, _D, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P)),
    "ff_backflow_v_div_f32": (_I, (_P, _Q, _I, _I, _NET, _P, _P, _P)),
    "ff_state_sums": (_I, (_P, _Q, _I, _P, _P, _P, _P)), "ff_beta_buffer_doubles": (_Z, (_I,)), "ff_beta_state_partials": (_I, (_P, _Q, _I, _P, _P, _P, _P)),
    "ff_beta_finish": (_I, (_P, _P, _P, _P, _I, _D, _Q, _P, _P, _P, _P)),
}

# include/fermiflow_robust.h, the second public header (the opt-in robust estimator), in its order
ROBUST_SIGNATURES = {
    "ff_energy_robust_workspace_bytes": (_Z, (_Q,)), "ff_energy_robust": (_I, (_P, _Q, _P, _P, _D, _P, _P, _P)),
    "ff_energy_robust_apply": (_I, (_P, _Q, _I, _I, _P, _P, _P, _Q, _I, _P, _P, _P, _P, _P)),
}
ROBUST_NSTAT = 10      # FF_ROBUST_NSTAT: [n_v, m, a, lo, hi, E, E_ss, Ec, n_c, value]

# include/fermiflow_maps.h, the third public header (density maps), in its order
MAPS_SIGNATURES = {
    "ff_maps_buffer_bytes": (_Z, (_I,)), "ff_maps_accumulate": (_I, (_P, _Q, _I, _I, _P, _D, _I, _P)),
}
MAPS_PLANES, MAPS_MAX_BINS = 6, 128      # FF_MAPS_PLANES, FF_MAPS_MAX_BINS

# include/fermiflow_obdm.h, the fourth public header (one-body density matrix, determinant signs), in its order
OBDM_SIGNATURES = {
    "ff_slater_sign": (_I, (_P, _Q, _I, _I, _P, _P, _P, _P, _P)),
    "ff_obdm_buffer_bytes": (_Z, (_I,)), "ff_obdm_workspace_bytes": (_Z, (_Q, _I)),
    "ff_obdm_accumulate": (_I, (_P, _Q, _I, _I, _P, _P, _P, _P, _P, _P, _D, _I, _P, _P)),
}
OBDM_MAX_SHELLS, OBDM_CHUNK, OBDM_HEAD = 8, 256, 5      # FF_OBDM_MAX_SHELLS, FF_OBDM_CHUNK, FF_OBDM_HEAD

# include/fermiflow_energy.h, the fifth public header (energy components), in its order
ENERGY_SIGNATURES = {
    "ff_energy_parts_buffer_bytes": (_Z, (_I,)), "ff_energy_parts_workspace_bytes": (_Z, (_Q, _I)),
    "ff_energy_parts_accumulate": (_I, (_P, _Q, _I, _I, _I, _D, _P, _P, _P, _P, _I, _P, _P, _P, _P)),
}
# FF_ENERGY_PARTS, FF_ENERGY_CHUNK, FF_ENERGY_PARTIAL, FF_ENERGY_HEAD, FF_ENERGY_FIXED, FF_ENERGY_MAX_STATES
ENERGY_PARTS, ENERGY_CHUNK, ENERGY_PARTIAL, ENERGY_HEAD, ENERGY_FIXED, ENERGY_MAX_STATES = 6, 256, 28, 4, 52, 65536

# include/fermiflow_dmc.h, the sixth public header (fixed-node diffusion Monte Carlo), in its order
DMC_SIGNATURES = {
    "ff_dmc_propose": (_I, (_P, _Q, _I, _I, _I, _D, _D, _P, _P, _P, _U, _Q, _Q, _P, _P)),
    "ff_dmc_accept_workspace_bytes": (_Z, (_Q,)),
    "ff_dmc_accept": (_I, (_P, _Q, _I, _I, _I, _D, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U, _Q, _Q, _P, _P, _Q, _P, _I, _P)),
    "ff_dmc_comb_workspace_bytes": (_Z, (_Q,)),
    "ff_dmc_comb": (_I, (_P, _Q, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _U, _Q, _P, _P, _P, _P, _P, _P, _P, _P)),
}
DMC_REC, DMC_CHUNK, DMC_U_SLOT = 9, 256, 64      # FF_DMC_REC, FF_DMC_CHUNK, FF_DMC_U_SLOT


def bind(cdll):
    """Set restype and argtypes of every function of SIGNATURES, ROBUST_SIGNATURES, MAPS_SIGNATURES, OBDM_SIGNATURES, ENERGY_SIGNATURES and DMC_SIGNATURES that `cdll` exports; returns cdll.  One it lacks (the
    host simulator has no ff_comm_*; an A/B build of an earlier commit may lack the newest) is skipped and fails where it is called, as
    any missing symbol."""
    for name, (restype, argtypes) in {**SIGNATURES, **ROBUST_SIGNATURES, **MAPS_SIGNATURES, **OBDM_SIGNATURES, **ENERGY_SIGNATURES, **DMC_SIGNATURES}.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return cdll
