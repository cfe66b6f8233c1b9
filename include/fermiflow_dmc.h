/* fermiflow_dmc.h -- sixth public header of libfermiflow_hip.so: the three small kernels of FIXED-NODE DIFFUSION MONTE CARLO with the
 * trained wave function as guiding function (fermiflow_amd.DMC; no upstream counterpart): drift-diffusion proposals, the Green's-function
 * accept step with weights and the step's record, and a fixed-population comb.  The expensive part of a step -- logp = 2 ln|psi|, its
 * gradient and the local energy of the proposals -- is ff_eloc_nd; the sign of psi is ff_slater_sign at z(t0) (fermiflow_obdm.h).
 * Conventions as in fermiflow.h (device pointers, `stream`, status codes 0 / 1 / 2 / 3, ff_last_error() -- here it starts with
 * "ff_dmc:" --, refusals before any launch, the library allocates nothing, nothing waits for the host).
 * Kernels: fermiflow_amd/csrc/ff_dmc.h.
 *
 * Shapes: x, grad (B, n, 2) in fp64 as ff_eloc_nd writes them (grad is the gradient of log p = 2 ln|psi|), n = nup + ndn; logp, eloc,
 * sign, w (B).  d = 2 only (ff_slater_sign is); n <= 24, a species <= 12.
 *
 * Drift.  v_i = grad_i / 2 is the drift of particle i, and the LIMITED drift is vbar_i = s_i v_i with
 *   s_i = 2 / (1 + sqrt(1 + (2 a tau) |v_i|^2)),   a = drift_limit >= 0   (a = 0: s_i = 1, the plain drift).
 * Every kernel here evaluates it in plain IEEE double arithmetic without fused multiply-adds, in this order:
 *   vx = 0.5 gx, vy = 0.5 gy, v2 = vx vx + vy vy, s = 2 / (1 + sqrt(1 + c v2)) with c = (2 a) tau, vbar = (vx s, vy s).
 *
 * ff_dmc_propose:  x' = (x + tau vbar) + sqrt(tau) xi, coordinate by coordinate, one lane per group of four coordinates.
 *   noise != NULL: xi = noise (B, n, 2).  noise == NULL: xi = ff_normal_quad(seed, walker_offset + b, step, quad) of csrc/ff_rng.h --
 *   Philox4x32-10, counter (walker, step, quad); quad q serves coordinates 4 q .. 4 q + 3 of the walker and the values past the last
 *   coordinate are discarded.  Sharding a batch with walker_offset gives the walkers of the whole batch.
 *   xi_out: (B, n, 2) or NULL; receives exactly the normals used.
 *
 * ff_dmc_accept: one lane per walker.  State x, logp, grad, eloc, sign, w (read and written); proposal x_new ... sign_new (read).
 *   u != NULL: the uniform of walker b is u[b]; else ff_uniform(seed, walker_offset + b, step, FF_DMC_U_SLOT) (a slot no quad uses).
 *   ctrl: 3 doubles on the device, E_T, E_ref, c.
 *     lf = -sum_i |x'_i - x_i - tau vbar_i(x)|^2 / (2 tau),   lb = -sum_i |x_i - x'_i - tau vbar_i(x')|^2 / (2 tau)
 *       (particles in order, each adds dx dx + dy dy to the sum; the sum is divided by 2 tau at the end)
 *     q = ((logp' - logp) + lb) - lf
 *   DEAD: the walker's own state is not finite (a coordinate, a gradient entry, logp, eloc, sign or w is NaN or infinite, or w < 0).
 *         Its w becomes 0, it does not move, it counts as invalid and adds nothing to any sum.
 *   INVALID: one of x', logp', grad', eloc', sign' is not finite.   CROSSED: valid and sign' sign <= 0.
 *   p = 0 if invalid or crossed, else 1 for q >= 0 and exp(q) for q < 0 (a NaN q: 0).  ACCEPTED iff u < p: the five state arrays of the
 *   walker are overwritten with the proposal.  With e_old the state's energy before and e_now after the step,
 *     w <- w exp(tau (E_T - 0.5 (clip(e_old) + clip(e_now)))),   clip(e) = min(max(e, E_ref - c), E_ref + c).
 *   accepted_out: uint8 (B) or NULL, 1 for an accepted walker.
 *   Record: FF_DMC_REC = 9 words of 8 bytes written (not added) to rec + step_slot * FF_DMC_REC, with w the NEW weights:
 *     double [0] sum w  [1] sum w e_now  [2] sum w e_now^2  [3] sum w^2  [4] sum p  [5] max w
 *     int64  [6] accepted  [7] crossed  [8] invalid (proposals that are invalid, and dead walkers)
 *   Determinism: the walkers are cut into chunks of FF_DMC_CHUNK = 256 consecutive walkers, whatever the grid.  Inside a chunk every
 *   quantity is summed in walker order over each of its 8 segments of 32 walkers, the segments are added in order; the workgroup that
 *   draws the last ticket adds the chunks in chunk order.  No floating-point atomics: the record is bit-identical from run to run and
 *   for any grid.  groups: workgroups of the launch, 0 for the library's choice (tests and probes pass others; <= 65536).
 *   rec must hold FF_DMC_REC (step_slot + 1) words: the library cannot see its length, the bound is the caller's.  groups and
 *   accepted_out serve tests and probes; a driver passes 0 and NULL.
 *   workspace: ff_dmc_accept_workspace_bytes(B) = 8 (1 + FF_DMC_REC ceil(B / 256)) bytes; its first word is the ticket: zeroed by the
 *   caller once, zero again after every call.  The rest need not be zero and holds nothing between calls.
 *
 * ff_dmc_comb: fixed population B by systematic resampling.  ws_j = w_j if w_j is finite and > 0, else 0.
 *   Cumulative weights, in this association: chunk c holds the walkers 256 c .. 256 c + 255; loc_j is the left-to-right sum of ws from
 *   the first walker of j's chunk up to j; T_c is loc of the chunk's last walker; P_0 = 0, P_{c+1} = P_c + T_c;
 *   cum_j = P_c + loc_j;   W = cum_{B-1}.
 *   u0 != NULL: one double on the device in [0, 1); else ff_uniform(seed, 2^63, step, 0) (no walker has that index).
 *   Slot k takes src_k = the smallest j with t_k < cum_j, t_k = fl(fl(k + u0) fl(W / B)), found by binary search, and no later than the
 *   last j with ws_j > 0.  src (B) int32 is non-decreasing.  x_out ... sign_out receive the state gathered through src (they must not
 *   alias the inputs), w becomes 1 everywhere.
 *   info: int32 [4]: [0] the number of distinct sources  [1] the largest number of copies of one source  [2] flag  [3] 0.
 *   W = 0 or not finite: status 0, flag = 1, src is the identity (the state is copied through it, w becomes 1); distinct = B, copies 1.
 *   workspace: ff_dmc_comb_workspace_bytes(B) = 8 (4 + B + 3 ceil(B / 256)) bytes; first word the ticket, as above.  Three launches.
 *
 * Refusals (before any launch): FF_EINVAL (1) for a null pointer (unless B == 0; the optional ones are noise, xi_out, u, accepted_out,
 * u0), a negative size, nup + ndn < 1, tau <= 0 or not finite, drift_limit < 0 or not finite, step or step_slot < 0, step >= 2^32,
 * walker_offset < 0, groups < 0 or > 65536; FF_EUNSUPPORTED (2) for d != 2, n > 24, a species > 12, B >= 2^31.  B = 0 is a no-op.
 * The workspace-size functions return 0 for B < 0 or B >= 2^31. */
#ifndef FERMIFLOW_DMC_H
#define FERMIFLOW_DMC_H
#include "fermiflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FF_DMC_REC 9
#define FF_DMC_CHUNK 256
#define FF_DMC_U_SLOT 64

int ff_dmc_propose(void* stream, int64_t B, int nup, int ndn, int d, double tau, double drift_limit, const double* x, const double* grad,
                   const double* noise, uint64_t seed, int64_t walker_offset, int64_t step, double* x_new, double* xi_out);
size_t ff_dmc_accept_workspace_bytes(int64_t B);
int ff_dmc_accept(void* stream, int64_t B, int nup, int ndn, int d, double tau, double drift_limit, double* x, double* logp, double* grad,
                  double* eloc, double* sign, double* w, const double* x_new, const double* logp_new, const double* grad_new,
                  const double* eloc_new, const double* sign_new, const double* u, uint64_t seed, int64_t walker_offset, int64_t step,
                  const double* ctrl, void* rec, int64_t step_slot, uint8_t* accepted_out, int groups, void* workspace);
size_t ff_dmc_comb_workspace_bytes(int64_t B);
int ff_dmc_comb(void* stream, int64_t B, int nup, int ndn, int d, double* w, const double* x, const double* logp, const double* grad,
                const double* eloc, const double* sign, const double* u0, uint64_t seed, int64_t step, int32_t* src, double* x_out,
                double* logp_out, double* grad_out, double* eloc_out, double* sign_out, int32_t* info, void* workspace);

#ifdef __cplusplus
}
#endif
#endif
