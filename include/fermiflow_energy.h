/* fermiflow_energy.h -- fifth public header of libfermiflow_hip.so: the ENERGY COMPONENTS of the physical walkers -- kinetic energy by
 * two estimators, trap energy and the Coulomb repulsion by spin pair -- accumulated on the device (fermiflow_amd.EnergyParts; no upstream
 * counterpart).  Conventions as in fermiflow.h (device pointers, `stream`, status codes 0 / 1 / 2 / 3, ff_last_error() -- here it starts
 * with "ff_energy_parts:" --, refusals before any launch, the library allocates nothing).  Kernels: fermiflow_amd/csrc/ff_energy_parts.h.
 *
 * Inputs: x (B, n, d), grad (B, n, d) and lap (B) in fp64 as ff_eloc_nd writes them -- grad and lap are the gradient and the Laplacian
 * of log p = 2 ln|psi| at x.  n = nup + ndn, rows 0 .. nup-1 are spin-up, d = 2 or 3.
 *
 * Components of a walker, K = FF_ENERGY_PARTS = 6, with |grad|^2 = sum over the n d entries:
 *   c[0] T_L    = -lap / 4 - |grad|^2 / 8        the local kinetic energy -1/2 (laplacian psi) / psi
 *   c[1] T_G    = |grad|^2 / 8                   the gradient estimator 1/2 |grad ln psi|^2
 *   c[2] V_trap = 1/2 sum_i |x_i|^2
 *   c[3] V_uu   = Z sum_{i < j, both up} 1 / |x_i - x_j|
 *   c[4] V_ud   = Z sum_{i up, j down} 1 / |x_i - x_j|
 *   c[5] V_dd   = Z sum_{i < j, both down} 1 / |x_i - x_j|
 * With Z == 0 the three pair components are exactly 0 and no pair distance is formed.  Linear in c: the local energy
 * E = c0 + c2 + c3 + c4 + c5, the virial W = 2 c0 - 2 c2 + c3 + c4 + c5 (zero on average in an eigenstate of the harmonic trap with
 * Coulomb repulsion, d = 2 and 3) and dT = c0 - c1 (zero on average for any normalisable psi).
 * A walker is INVALID if one of its six components is not finite as computed (a NaN coordinate or lap, a coincident pair with Z != 0)
 * or, with nstates > 0, if its walker_state entry is outside [0, nstates).  An invalid walker contributes nothing and is counted.
 *
 * centre: 6 doubles on the device, or NULL for zeros.  Every moment is taken about it, d_k = c_k - centre_k: a centre near the means
 * keeps the second moments free of cancellation.  Every call on one accumulator must pass the same values -- buffers that share a
 * centre add up word by word (ranks, checkpoints).
 *
 * parts_out: (B, 6) doubles or NULL; row b receives c of walker b as computed, for an invalid walker too.
 *
 * acc: a caller-owned array of 8-byte words, zeroed by the caller once (and again to reset):
 *   uint64  [0] calls   [1] walkers (valid)   [2] invalid   [3] ticket (zero between calls)
 *   double  [4, 10)   sum[6]     += sum_b d_k                  over the valid walkers of the call
 *           [10, 46)  sum2[6][6] += sum_b d_k d_l              symmetric bit for bit
 *           [46, 52)  blocksq[6] += (sum_b d_k)^2              one call is one block of the block standard error
 *   and with nstates = S > 0, over the valid walkers b of state s (walker_state[b] == s):
 *   uint64  [52, 52 + S)         count[s]
 *   double  [52 + S, 52 + 7 S)   ssum[s][6] += sum_b d_k
 *           [52 + 7 S, 52 + 8 S) sumE2[s]   += sum_b (d0 + d2 + d3 + d4 + d5)^2     -- sum (E - E_centre)^2, E_centre the same sum of centre
 * Means: centre_k + sum[k] / walkers; covariance of the walkers: sum2 / walkers - (sum / walkers)(sum / walkers)^T.
 * ff_energy_parts_buffer_bytes returns 8 (52 + 8 nstates), or 0 for nstates outside [0, FF_ENERGY_MAX_STATES].
 *
 * walker_state: int32 (B), sorted ascending as for ff_state_sums; NULL when nstates == 0.
 *
 * workspace: ff_energy_parts_workspace_bytes(B, nstates) bytes of scratch: 8 FF_ENERGY_PARTIAL ceil(B / FF_ENERGY_CHUNK) (one chunk's
 * worth for B = 0), and 48 B more with nstates > 0 (the components of every walker, for the per-state sums).  It need not be zero and
 * holds nothing between calls.  0 for nstates outside the limits, B < 0 or B >= 2^31.
 *
 * Determinism.  The walkers are cut into chunks of FF_ENERGY_CHUNK consecutive walkers, whatever the grid.  Within a chunk the 6 sums,
 * the 21 second moments k <= l and the number of valid walkers are summed in walker order over each of its 8 segments of 32 walkers
 * (one fused multiply-add per walker and moment), the segments are added in order, and the 28 numbers go to the workspace.  The
 * workgroup that draws the last ticket adds the chunks in chunk order and adds the totals to the accumulator; it alone touches the
 * first 52 words but the ticket.  The per-state sums are a second launch on the same stream: one workgroup per state over its sorted
 * range with a fixed tree, as ff_state_sums; it alone touches the words of its state.  No floating-point atomic is used: a result is
 * bit-identical from run to run and for any grid.
 *
 * Limits and refusals (before any launch): FF_EINVAL (1) for a null pointer (acc; x, grad, lap, workspace and, with nstates > 0,
 * walker_state unless B == 0), a negative size (B, nup, ndn, d < 1, nstates), nup + ndn < 1, Z not finite; FF_EUNSUPPORTED (2) for
 * nup + ndn > 24, (nup + ndn) d > 60, d not 2 or 3, B >= 2^31, nstates > FF_ENERGY_MAX_STATES.  B = 0 is a no-op that counts
 * nothing.  At most two launches per call, one when nstates == 0.  Nothing waits for the host. */
#ifndef FERMIFLOW_ENERGY_H
#define FERMIFLOW_ENERGY_H
#include "fermiflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FF_ENERGY_PARTS 6
#define FF_ENERGY_CHUNK 256
#define FF_ENERGY_PARTIAL 28
#define FF_ENERGY_HEAD 4
#define FF_ENERGY_FIXED 52
#define FF_ENERGY_MAX_STATES 65536

size_t ff_energy_parts_buffer_bytes(int nstates);
size_t ff_energy_parts_workspace_bytes(int64_t B, int nstates);
int ff_energy_parts_accumulate(void* stream, int64_t B, int nup, int ndn, int d, double Z, const double* x, const double* grad,
                               const double* lap, const int32_t* walker_state, int nstates, const double* centre, double* parts_out,
                               void* acc, void* workspace);

#ifdef __cplusplus
}
#endif
#endif
