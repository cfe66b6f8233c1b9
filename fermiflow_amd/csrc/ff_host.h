// ff_host.h -- what the host-side launch code of the kernel files shares: the error macros, the device's CU count, the grid
// size of a launch, the ff_ode fields every launch struct carries, the argument checks of the C ABI and the copy-out of the
// ff_eloc workspace.  Host code only; nothing here is seen by a kernel.
#pragma once
#include "ff_common.h"
#include <stdio.h>

void ff_set_error(const char* msg);      // ff_api.hip: ff_last_error() of the calling thread (copies msg)
int64_t ff_device_cus();                 // ff_api.hip: compute units of the current device

// (macros because they return from the entry point that uses them)
#define FF_CHECK(cond, code, msg) do { if (!(cond)) { ff_set_error(msg); return code; } } while (0)
#define FF_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { ff_set_error(hipGetErrorString(e_)); return FF_ELAUNCH; } } while (0)

// workgroups of a launch: one per group of `per_group` items, at most `cap` (a persistent or grid-stride launch)
static inline unsigned ff_grid(int64_t count, int64_t per_group, int64_t cap = INT64_MAX) {
  const int64_t groups = (count + per_group - 1) / per_group;
  return (unsigned)(groups < cap ? groups : cap);
}

// The fields of a launch struct (ff_fwd_args, ff_adj_args) that come straight from ff_net and ff_ode.  forward: the kernel
// integrates from ode->t0 to ode->t1 (CNF.generate, the adjoint), otherwise from t1 back to t0.
template <class Args>
static inline void ff_fill_common(Args& a, int64_t B, const ff_net* net, const ff_ode* ode, bool forward) {
  a.B = B; a.net = *net;
  a.ta = forward ? ode->t0 : ode->t1; a.tb = forward ? ode->t1 : ode->t0;
  a.rtol = ode->rtol; a.atol = ode->atol;
  a.max_steps = ode->max_steps > 0 ? ode->max_steps : 10000;
  a.wcost = ode->walker_cost; a.order = ode->walker_order;
  a.h_init = ode->walker_h_init;
  a.h_scale = ode->walker_h_uniform ? -fabs(ode->walker_h_scale) : fabs(ode->walker_h_scale);      // (the sign carries walker_h_uniform)
  a.h_out = ode->walker_h_out; a.h_equal = ode->walker_h_equal;
}

// --- argument checks: FF_OK, or the status of the refusal with "<who>: <what>" in ff_last_error()
static inline int ff_refuse(int code, const char* who, const char* what) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  ff_set_error(msg);
  return code;
}
// eta complete; mu complete or absent
static inline int ff_check_net(const char* who, const ff_net* net) {
  if (net->He > 0 && net->ew1 && net->eb1 && net->ew2 && (net->Hm == 0 || (net->mw1 && net->mb1 && net->mw2))) return FF_OK;
  return ff_refuse(FF_EINVAL, who, "bad net");
}
// the entry points of the fused ODE kernels: sizes (and whatever else of the caller's `args_ok`), net, hidden widths, tolerances
static inline int ff_check_flow(const char* who, bool args_ok, const ff_net* net, const ff_ode* ode) {
  if (!(args_ok && net && ode)) return ff_refuse(FF_EINVAL, who, "bad argument");
  if (const int st = ff_check_net(who, net)) return st;
  if (!(net->He <= FF_HMAX && net->Hm <= FF_HMAX)) return ff_refuse(FF_EUNSUPPORTED, who, "hidden width > 256");
  if (!(ode->rtol > 0 && ode->atol > 0)) return ff_refuse(FF_EINVAL, who, "tolerances must be positive");
  return FF_OK;
}
// a spin species that has particles has its orbital table ...
static inline int ff_check_tables(const char* who, int nup, int ndn, const int32_t* tab_up, const int32_t* tab_dn) {
  if ((nup == 0 || tab_up) && (ndn == 0 || tab_dn)) return FF_OK;
  return ff_refuse(FF_EINVAL, who, "null orbital table");
}
// ... and its determinant a size the Slater code handles
static inline int ff_check_det_size(const char* who, int nup, int ndn) {
  if (nup <= FF_MAX_NS && ndn <= FF_MAX_NS) return FF_OK;
  return ff_refuse(FF_EUNSUPPORTED, who, "determinant larger than FF_MAX_NS");
}
static inline int ff_check_spins(const char* who, int nup, int ndn, const int32_t* tab_up, const int32_t* tab_dn) {
  if (const int st = ff_check_tables(who, nup, ndn, tab_up, tab_dn)) return st;
  return ff_check_det_size(who, nup, ndn);
}

// z(t0) and Delta out of the ff_eloc workspace (ff_eloc_ws.h), for the callers that ask for copies of their own
static inline int ff_copy_out(void* stream, int64_t B, size_t M, const double* z0, const double* dl, double* z_out, double* dlogp_out) {
  if (z_out && hipMemcpyAsync(z_out, z0, sizeof(double) * (size_t)B * M, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return FF_ELAUNCH;
  if (dlogp_out && hipMemcpyAsync(dlogp_out, dl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return FF_ELAUNCH;
  return FF_OK;
}
