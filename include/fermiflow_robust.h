/* fermiflow_robust.h -- second public header of libfermiflow_hip.so: the opt-in ROBUST ground-state estimator (GSVMC.clip_eloc;
 * no upstream counterpart: src/VMC.py:56-59 takes plain means).  It drops failed walkers and clips the local energies about their
 * median before the gradient is formed, device-resident end to end.  Conventions as in fermiflow.h (device pointers, `stream`, status
 * codes 0 / 1 / 2 / 3, ff_last_error()).  Kernels: fermiflow_amd/csrc/ff_robust.h.
 *
 * Definitions, over a batch of N walkers with local energies e_b and log-probabilities l_b:
 *   valid_b    e_b and l_b are both finite (l = NULL: e_b is finite); n_v = the number of valid walkers
 *   m          the LOWER MEDIAN of the valid energies: the element of 0-based rank (n_v - 1) / 2 (integer division) in ascending order,
 *              the order being that of the usual map of the fp64 bit pattern to uint64 (all bits of a negative number flipped, the sign
 *              bit of a non-negative one set; -0.0 sorts below +0.0).  An element of the input: exact.
 *   a          (1 / n_v) sum_valid |e_b - m|                 (the width)
 *   lo, hi     m - k a, m + k a                              (the window)
 *   c_b        min(max(e_b, lo), hi)                         (the clipped energy);  n_c = the number of valid walkers with c_b != e_b
 *   E, E_ss    the mean of the UNCLIPPED valid e_b and sum_valid (e_b - E)^2, clamped at 0 (E_std^2 = E_ss / (n_v - 1)); a sum of
 *              squares that leaves the double range is +inf
 *   Ec         the mean over the valid walkers of c_b
 *   value      (1 / n_v) sum_valid l_b (c_b - Ec)            (the surrogate's value)
 *   u_b        (c_b - Ec) (N / n_v) for a valid walker, exactly 0 for an invalid one (the gradient weights)
 * ff_cnf_adjoint_energy(eloc = u, e_mean = a device zero, scale = 1 / N) then forms the seeds w_b = (c_b - Ec) / n_v.
 * n_v = 0: E, m, a, lo, hi, Ec and the value are NaN, E_ss is NaN, n_c = 0 and every u_b is 0 (the parameter gradient is exactly zero).
 *
 * stat: FF_ROBUST_NSTAT doubles on the device,
 *   [0] n_v  [1] m  [2] a  [3] lo  [4] hi  [5] E  [6] E_ss  [7] Ec  [8] n_c  [9] value
 * (counts as doubles, exact below 2^53).  ff_energy_robust writes [0, 9); ff_energy_robust_apply with finish != 0 writes [9].
 *
 * ff_energy_robust: selection + moments + clipped sums on a WHOLE batch (under data parallelism: on the gathered energies of all ranks,
 *   invalid walkers marked by a NaN energy, logp = NULL -- every rank then holds bit-identical statistics).  Sums are taken about
 *   shift_dev[0] (any finite number, e.g. the previous sweep's E: no cancellation; a non-finite one counts as 0) and about m.
 *   The median is an exact radix select on the 64-bit keys: FF_ROBUST_PASSES (6) launches of FF_ROBUST_DIGIT_BITS (11) bits each,
 *   integer atomics only; moments and clipped sums are one launch each with fixed summation trees, joined in segment order by
 *   whichever workgroup finishes last.  Every result is bit-identical run to run.  Eight launches, nothing waits for the host.
 * ff_energy_robust_apply: serves B walkers (this rank's shard; B = 0 is allowed) of a batch of n_global walkers whose statistics are
 *   in stat.  Writes u_out (B).  Where z / glogp0 (B, n, d; both or neither) are given, OVERWRITES IN PLACE the rows of invalid walkers:
 *   z with the fixed finite configuration  x_i = (FF_ROBUST_SAFE_STEP (i + 1), 0 [, 0])  -- particle i on the first axis at radius
 *   0.25 (i + 1): pairwise distinct, none at the origin -- and glogp0 with zeros (a zero weight is not enough for a failed walker:
 *   0 x NaN would poison the adjoint's sums); valid rows are not touched.  sum_out[0] = sum_valid l_b (c_b - Ec) over the shard (fixed
 *   tree); finish != 0 (a single rank): stat[9] = sum_out[0] / n_v in the same launch; finish = 0: the caller all-reduces sum_out and
 *   divides by stat[0].  One launch.
 * workspace: ff_energy_robust_workspace_bytes(N) bytes (for the apply: of at least its B; the two calls may share one on a stream),
 *   zeroed by the caller ONCE; every call leaves its tickets, its selection state and its histogram at zero again.
 * Limits and refusals (before any launch): FF_EINVAL (1) for null pointers, N < 1, B < 0, n_global < 1, k not finite or <= 0,
 *   z without glogp0; FF_EUNSUPPORTED (2) for N or B >= 2^31, or n d > 60 / n < 1 / d < 1 with z given.
 *   ff_energy_robust_workspace_bytes returns 0 for a size outside the limits. */
#ifndef FERMIFLOW_ROBUST_H
#define FERMIFLOW_ROBUST_H
#include "fermiflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FF_ROBUST_NSTAT 10
#define FF_ROBUST_PASSES 6
#define FF_ROBUST_DIGIT_BITS 11
#define FF_ROBUST_SAFE_STEP 0.25

size_t ff_energy_robust_workspace_bytes(int64_t N);
int ff_energy_robust(void* stream, int64_t N, const double* e, const double* logp, double k, const double* shift_dev, double* stat,
                     void* workspace);
int ff_energy_robust_apply(void* stream, int64_t B, int n, int d, const double* e, const double* logp, double* stat, int64_t n_global,
                           int finish, double* u_out, double* z, double* glogp0, double* sum_out, void* workspace);

#ifdef __cplusplus
}
#endif
#endif
