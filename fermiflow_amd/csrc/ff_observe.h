// ff_observe.h -- observables of the physical walkers as INTEGER histograms accumulated on the device: the radial density
// of each spin species and the pair-distance distribution of each pair of species (ff_observe_accumulate, include/fermiflow.h).
//
// Classes c (the first nup particles are spin-up, as everywhere):
//   0 up: r = |x_i|     1 down: r = |x_i|     2 up-up   3 up-down   4 down-down: r = |x_i - x_j|, i < j
// A sample r = sqrt(sum_k delta_k^2) (fp64) goes to slot
//   nbins + 1 ("invalid")   if r is not finite,
//   nbins     ("overflow")  if r >= rmax,
//   min((int)(r * (nbins / rmax)), nbins - 1) otherwise
// of its class; every class has FF_OBS_SLOTS(nbins) = nbins + 2 slots.  (Finite coordinates whose squares overflow the
// double range are summed again scaled by 2^-512 -- exact --, so r = 1e300 is an overflow sample, not an invalid one.)
//
// The accumulator is a caller-owned buffer of uint64 words (S = 5 (nbins + 2)):
//   [0] calls   [1] walkers   [2, 2 + S) sum   [2 + S, 2 + 2S) sumsq   [2 + 2S, 2 + 3S) scratch   [2 + 3S] ticket
// sum: total count per slot; sumsq: sum over calls of (that call's count)^2 -- one block per call for the block standard
// error; scratch + ticket: this call's counts while it runs, zero between calls.  The caller zeroes the buffer once.
//
// Lane mapping: ONE LANE PER WALKER.  A wave takes 64 consecutive walkers, stages their contiguous span of coordinates through
// LDS with coalesced loads (as ff_potential_stream_kernel; row stride n d | 1 doubles: conflict-free when every lane reads its
// own walker) and walks the n + n (n - 1) / 2 samples of its walker; every sample is one non-returning LDS integer add
// (ds_add_u32) into the workgroup's histogram.  One lane per SAMPLE would issue the same number of LDS adds, pay an index
// decode per sample and read the staged rows with conflicts; what it would buy -- lanes of one instruction spread over the
// classes -- the private copies below buy more directly.  At one instruction all lanes add to the same class, and the density
// puts most of them into a few dozen bins: the histogram is kept in `ncopy` (up to 8) interleaved copies, lane l adds to copy
// l % ncopy, so lanes that meet in a bin land on neighbouring banks instead of one address.
// At the end a workgroup adds its non-zero slots to the call's scratch with global integer atomics; the workgroup that
// finishes last (the ticket) folds the scratch into sum / sumsq and clears it.  No floating-point atomics anywhere: every
// word is an exact integer whatever the order, the grid or the number of ranks.
#pragma once
#include "ff_common.h"

#define FF_OBS_CLASSES 5
#define FF_OBS_MAX_BINS 1024
#define FF_OBS_MAX_COORD 60              // n d of the staged rows
#define FF_OBS_MAX_LAUNCH ((int64_t)1 << 22)  // walkers per launch: 2^22 x 276 pairs < 2^32, so no uint32 LDS slot can wrap whatever the grid;
                                              // a call with more walkers is several launches, the last of which folds (ff_observe_accumulate)
#define FF_OBS_HIST_WORDS 8192           // LDS words of the histogram copies (32 KB)
#define FF_OBS_MAX_COPIES 8
#define FF_OBS_LDS_BYTES (65536 - 64)    // histogram copies + staged rows of the workgroup's waves (the 64 KB of a launch, less the static words)
#define FF_OBS_GRID_PER_CU 2             // persistent grid: workgroups per compute unit (each flushes its histogram once)
#define FF_OBS_SLOTS(nbins) ((nbins) + 2)

FF_D int ff_obs_slot(double dx, double dy, double dz, double rmax, double scale, int nbins) {
  const double big = 1.7976931348623157e308;
  double r = sqrt(dx * dx + dy * dy + dz * dz);
  if (!(r <= big)) {                                   // inf or NaN
    if (fabs(dx) <= big && fabs(dy) <= big && fabs(dz) <= big) {      // finite terms whose squares left the double range
      const double ax = dx * 0x1p-512, ay = dy * 0x1p-512, az = dz * 0x1p-512;
      r = sqrt(ax * ax + ay * ay + az * az) * 0x1p512;
    }
    if (!(r <= big)) return nbins + 1;
  }
  if (r >= rmax) return nbins;
  const int k = (int)(r * scale);
  return k < nbins - 1 ? k : nbins - 1;
}

// blockDim.x = 64 nwave; dynamic LDS: [S ncopy uint32, padded to 16 bytes | nwave x 64 rows of (n d | 1) doubles].
// magic = ceil(2^32 / (n d)): e / (n d) = umulhi(e, magic) for the e < 64 x 60 of a tile.
// B, x: the walkers of this launch.  call_walkers: the walkers of the whole call if this launch closes it (its last workgroup
// folds the scratch), 0 if another launch of the same call follows on the stream (the counts stay in the scratch).
__global__ void __launch_bounds__(256)
ff_observe_kernel(int64_t B, int nup, int n, int d, const double* __restrict__ x, double rmax, double scale, int nbins, int ncopy,
                  unsigned magic, int64_t call_walkers, unsigned long long* __restrict__ acc) {
  FF_DYN_LDS(lds);
  __shared__ unsigned s_last;         // (the dynamic LDS holds 4- and 8-byte words only: it needs no more than 8-byte alignment)
  const int S = FF_OBS_CLASSES * FF_OBS_SLOTS(nbins), HW = S * ncopy;
  const int t = threadIdx.x, nt = blockDim.x, lane = t & (FF_WAVE - 1), wave = t / FF_WAVE, nwave = nt / FF_WAVE;
  const int M = n * d, stride = M | 1;
  unsigned* const hist = reinterpret_cast<unsigned*>(lds);            // [slot][copy]
  double* const sx = lds + ((HW + 3) / 4) * 2 + wave * FF_WAVE * stride;
  for (int k = t; k < HW; k += nt) hist[k] = 0u;
  __syncthreads();
  unsigned* const h = hist + (lane & (ncopy - 1));
  const int slots = FF_OBS_SLOTS(nbins);
  const int64_t ntiles = (B + FF_WAVE - 1) / FF_WAVE;
  for (int64_t tile = (int64_t)blockIdx.x * nwave + wave; tile < ntiles; tile += (int64_t)gridDim.x * nwave) {
    const int64_t b0 = tile * FF_WAVE;
    const int nw = (int)((B - b0) < FF_WAVE ? (B - b0) : FF_WAVE);
    const int tot = nw * M;
    const double* __restrict__ src = x + b0 * M;
    FF_WAVE_SYNC();                                     // (the previous tile's rows have been read)
    for (int k0 = 0; k0 < M; k0 += 8) {                 // eight loads in flight per lane, then their LDS stores
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int e = (k0 + u) * FF_WAVE + lane;
        v[u] = (k0 + u < M && e < tot) ? src[e] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int e = (k0 + u) * FF_WAVE + lane;
        if (k0 + u < M && e < tot) {
          const int w = (int)__umulhi((unsigned)e, magic);
          sx[w * stride + (e - w * M)] = v[u];
        }
      }
    }
    FF_WAVE_SYNC();
    if (lane < nw) {
      const double* row = sx + lane * stride;
      for (int i = 0; i < n; i++) {
        const double xi = row[i * d], yi = row[i * d + 1], zi = d == 3 ? row[i * d + 2] : 0.0;
        const int ci = i < nup ? 0 : 1;
        atomicAdd(&h[(ci * slots + ff_obs_slot(xi, yi, zi, rmax, scale, nbins)) * ncopy], 1u);
        for (int j = i + 1; j < n; j++) {
          const double xj = row[j * d], yj = row[j * d + 1], zj = d == 3 ? row[j * d + 2] : 0.0;
          const int cj = 2 + ci + (j < nup ? 0 : 1);      // up-up 2, up-down 3, down-down 4 (i < j: a down i has a down j)
          atomicAdd(&h[(cj * slots + ff_obs_slot(xi - xj, yi - yj, zi - zj, rmax, scale, nbins)) * ncopy], 1u);
        }
      }
    }
  }
  __syncthreads();
  // the workgroup's counts -> the call's scratch (non-zero slots only)
  unsigned long long* const sum = acc + 2, * const sumsq = sum + S, * const scratch = sumsq + S, * const ticket = scratch + S;
  for (int k = t; k < S; k += nt) {
    unsigned c = 0u;
    for (int q = 0; q < ncopy; q++) c += hist[k * ncopy + q];
    if (c) atomicAdd(&scratch[k], (unsigned long long)c);
  }
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(ticket, 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  if (call_walkers == 0) {            // not the call's last launch: only the ticket starts again
    if (t == 0) atomicExch(ticket, 0ull);
    return;
  }
  // the last workgroup folds the call.  Every word other workgroups wrote in this launch is read by a returning atomic (which
  // also clears it); sum, sumsq, calls and walkers are touched by the last workgroup of a call only.
  for (int k = t; k < S; k += nt) {
    const unsigned long long c = atomicExch(&scratch[k], 0ull);
    if (c) { sum[k] += c; sumsq[k] += c * c; }
  }
  if (t == 0) {
    acc[0] += 1ull;
    acc[1] += (unsigned long long)call_walkers;
    atomicExch(ticket, 0ull);
  }
}
