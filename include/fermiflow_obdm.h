/* fermiflow_obdm.h -- fourth public header of libfermiflow_hip.so: the ONE-BODY REDUCED DENSITY MATRIX rho_1(r, r') of the physical
 * walkers in a harmonic-oscillator basis, accumulated on the device (fermiflow_amd.OneBodyDensityMatrix; no upstream counterpart),
 * and the SIGN of the Slater determinants it needs.  Conventions as in fermiflow.h (device pointers, `stream`, status codes
 * 0 / 1 / 2 / 3, ff_last_error() -- here it starts with "ff_obdm:" --, refusals before any launch, the library allocates nothing).
 * Kernels: fermiflow_amd/csrc/ff_obdm.h.  d = 2 only.
 *
 * Orbitals and basis.  phi_k(x, y) = G(x, y) h_nx(x) h_ny(y), G = pi^-1/2 exp(-(x x + y y) / 2), k -> (nx, ny) in the HO2D list order
 * (shell N = nx + ny = 0, 1, ...; within a shell nx = 0 .. N), h_0 = 1, h_1 = sqrt(2) x,
 * h_{m+1} = sqrt(2 / (m + 1)) x h_m - sqrt(m / (m + 1)) h_{m-1}.  Where G is 0 as computed (|r| > 38.6) phi_k is 0, whatever the
 * polynomials are.  The basis is the first nb = S (S + 1) / 2 orbitals, S = nshells in 1 .. FF_OBDM_MAX_SHELLS: nb <= 36.
 *
 * Walkers: (n, 2) in fp64, n = nup + ndn, rows 0 .. nup-1 are spin-up.  For a walker b and a species s that has particles the caller
 * has drawn ONE point r'_{bs} from the density g(r') = exp(-|r'|^2 / (2 sigma^2)) / (2 pi sigma^2), and for every particle i of s it
 * has the walker x^{(b,i)} = x_b with row i replaced by r'_{bs}: its log-density logp' and the sign of its determinants sign'.
 *   q_{b,i} = (sign_b sign'_{b,i}) exp((logp'_{b,i} - logp_b) / 2)              -- the ratio psi(x^{(b,i)}) / psi(x_b)
 * A sample (b, i) is INVALID if q_{b,i} as computed is not finite or a coordinate of x_{b,i} or of r'_{bs} is not finite.  An invalid
 * sample contributes nothing and is counted in invalid[s].  (logp' = -inf or sign' = 0 with a finite exponent is a valid zero.)
 *   A_a = sum_{i in s, valid} phi_a(x_{b,i}) q_{b,i},   C_c = phi_c(r'_{bs}) / g(r'_{bs}),   a, c < nb
 *   T^s = sum_b (A C^T + C A^T) / 2                                              -- this call's matrix, symmetric bit for bit
 * r' is meant to be a draw from g: for |r'| beyond 38 sigma (sigma < 1) g is 0 as computed and C is not finite.
 *
 * acc: a caller-owned array of 8-byte words, zeroed by the caller once (and again to reset); E = 2 nb nb:
 *   uint64  [0] calls   [1] walkers   [2] invalid[up]   [3] invalid[down]   [4] ticket (zero between calls)
 *   double  [5, 5 + E) sum[2][nb][nb] += T          [5 + E, 5 + 2 E) sumsq[2][nb][nb] += T o T (entry by entry)
 * One call is one block of the block standard error: rho^s = sum^s / walkers, and with m = calls the error of an entry is
 * sqrt(max(sumsq / m - (sum / m)^2, 0) / (m - 1)) / (walkers / m).  ff_obdm_buffer_bytes returns 8 (5 + 2 E), or 0 for nshells
 * outside [1, FF_OBDM_MAX_SHELLS].
 *
 * workspace: ff_obdm_workspace_bytes(B, nshells) bytes of scratch, 8 E ceil(B / FF_OBDM_CHUNK) (one chunk's worth for B = 0); it need
 * not be zero and holds nothing between calls.  0 for nshells outside the limits, B < 0 or B >= 2^31.
 *
 * Determinism.  The walkers are cut into chunks of FF_OBDM_CHUNK consecutive walkers, whatever the grid.  The partial matrix
 * sum_b A_a C_c of a chunk is summed in walker order, one fused multiply-add per walker, and written to the workspace.  The workgroup
 * that draws the last ticket adds the chunks' partial matrices in chunk order, forms T = (M + M^T) / 2 and T o T and adds them to sum
 * and sumsq; it alone touches sum, sumsq, calls and walkers.  invalid is a sum of integers.  No floating-point atomic is used: a
 * result is bit-identical from run to run and for any grid.
 *
 * ff_slater_sign: sign_out[b] = sign(det Phi_up(z_b)) sign(det Phi_dn(z_b)) in {-1, 0, +1}, Phi_s[i][j] = phi_{tab_s[state_b][j]}(z_i)
 * (tables and walker_state as ff_logprob; walker_state NULL: state 0).  The positive factor G of a row is left out: the sign is that
 * of det[h_nx_j(x_i) h_ny_j(y_i)], from the partial-pivoting LU of the log-determinant kernels, (-1)^exchanges prod sgn(pivot).  Two
 * particles of one species at the same point give exactly 0.  NaN if a coordinate of the walker is not finite (or the polynomials of a
 * finite coordinate beyond 1e40 leave the double range).  One lane per walker; a species of 0 particles has sign 1.
 *
 * Limits and refusals (before any launch): FF_EINVAL (1) for a null pointer, a negative size, nup + ndn < 1, nshells < 1, sigma not
 * finite or <= 0; FF_EUNSUPPORTED (2) for nshells > FF_OBDM_MAX_SHELLS, nup + ndn > 24, nup or ndn > 12 (FF_MAX_NS), B >= 2^31.
 * B = 0 is a no-op that counts nothing.  Nothing waits for the host. */
#ifndef FERMIFLOW_OBDM_H
#define FERMIFLOW_OBDM_H
#include "fermiflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FF_OBDM_MAX_SHELLS 8
#define FF_OBDM_CHUNK 256
#define FF_OBDM_HEAD 5

int ff_slater_sign(void* stream, int64_t B, int nup, int ndn, const int32_t* tab_up, const int32_t* tab_dn, const int32_t* walker_state,
                   const double* z, double* sign_out);
size_t ff_obdm_buffer_bytes(int nshells);
size_t ff_obdm_workspace_bytes(int64_t B, int nshells);
/* x (B, n, 2), rprime (B, 2, 2) [walker][species][coordinate], logp (B), sign (B), logp_moved (B, n), sign_moved (B, n) */
int ff_obdm_accumulate(void* stream, int64_t B, int nup, int ndn, const double* x, const double* rprime, const double* logp,
                       const double* sign, const double* logp_moved, const double* sign_moved, double sigma, int nshells, void* acc,
                       void* workspace);

#ifdef __cplusplus
}
#endif
#endif
