/* fermiflow_maps.h -- third public header of libfermiflow_hip.so: two-dimensional DENSITY MAPS of the physical walkers as integer
 * histograms accumulated on the device (fermiflow_amd.DensityMaps; no upstream counterpart: the reference bins model.x on the host).
 * Conventions as in fermiflow.h (device pointers, `stream`, status codes 0 / 1 / 2 / 3, ff_last_error() -- here it starts with
 * "ff_maps:" --, refusals before any launch, the library allocates nothing).  Kernel: fermiflow_amd/csrc/ff_maps.h.
 *
 * Walkers: x (B, n, 2) in fp64, n = nup + ndn, the first nup particles are spin-up.  The window is the square [-L, L)^2 with
 * L = extent, cut into nbins x nbins cells; scale = nbins / (2 L).
 *
 * Six planes, each a histogram of samples (p, q):
 *   0 up, 1 down             lab frame: (p, q) = (x_i, y_i) of every particle of the species           nup, ndn samples per walker
 *   2 uu, 3 ud, 4 du, 5 dd   rotating frame: every ORDERED pair (i, j), i != j; the first letter is the species of the reference
 *                            particle i, the second that of the partner j          nup (nup - 1), nup ndn, ndn nup, ndn (ndn - 1)
 * Rotating frame of reference particle i, all in fp64:
 *   rho = sqrt(x_i x_i + y_i y_i);   (c, s) = (1, 0) if rho == 0 as computed, else (x_i / rho, y_i / rho)
 *   p = c x_j + s y_j;   q = c y_j - s x_j
 * -- the frame in which particle i sits at (rho, 0).  The reference particle itself is not binned in a pair plane (its law there is
 * the radial density); the partner is binned at (p, q).
 *
 * Slot of a sample, of the P = nbins^2 + 2 slots of its plane:
 *   invalid   P - 1   a coordinate that enters it is not finite (for a pair: any of its four), or rho, p or q is not finite.  A NaN
 *                     coordinate spoils only the samples it is part of.
 *   otherwise a = (p + L) scale, b = (q + L) scale, and
 *   overflow  P - 2   unless 0 <= a < nbins and 0 <= b < nbins
 *   cell      (int)a * nbins + (int)b
 *
 * acc: a caller-owned array of uint64 words, zeroed by the caller once (and again to reset):
 *   [0] calls   [1] walkers   [2, 2 + 6 P) sum[6][P]
 * Counts only: no squares, no scratch, no ticket.  The cells of a map are Poisson counts (error sqrt(count)).  Every word is an
 * integer and no floating-point atomic is used: a result is bit-identical from run to run whatever the grid, and additive over
 * ranks.  ff_maps_buffer_bytes returns 8 (2 + 6 P), or 0 for nbins outside [1, FF_MAPS_MAX_BINS].
 *
 * ff_maps_accumulate adds the B walkers of x to acc: one launch per 2^22 walkers (2^22 x 552 ordered pairs < 2^32, the bound of
 * the kernel's uint32 counters), all of them ONE call -- calls += 1, walkers += B.  B = 0 is a no-op.  Nothing waits for the host.
 * Limits and refusals (before any launch): FF_EINVAL (1) for a null pointer, a negative size, nup + ndn < 1, nbins < 1, extent not
 * finite or <= 0; FF_EUNSUPPORTED (2) for nbins > FF_MAPS_MAX_BINS (128) or nup + ndn > 24. */
#ifndef FERMIFLOW_MAPS_H
#define FERMIFLOW_MAPS_H
#include "fermiflow.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FF_MAPS_PLANES 6
#define FF_MAPS_MAX_BINS 128

size_t ff_maps_buffer_bytes(int nbins);
int ff_maps_accumulate(void* stream, int64_t B, int nup, int ndn, const double* x, double extent, int nbins, void* acc);

#ifdef __cplusplus
}
#endif
#endif
