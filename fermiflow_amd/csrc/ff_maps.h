// ff_maps.h -- two-dimensional density maps of the physical walkers as INTEGER histograms accumulated on the device: the lab-frame
// density rho(x, y) of each spin species and the pair density of each ordered pair of species in the frame that rotates with the
// reference particle (ff_maps_accumulate, include/fermiflow_maps.h -- planes, rotation and slots are defined there).
//
// The accumulator is a caller-owned buffer of uint64 words (P = nbins^2 + 2 slots per plane: cells, overflow, invalid):
//   [0] calls   [1] walkers   [2, 2 + 6 P) sum[6][P]
//
// Mapping: ONE PLANE, OR A BAND OF ONE, PER WORKGROUP; one lane per walker.  A plane of 128 x 128 cells is 64 KB of uint32 and the six
// are 393 KB, so no workgroup holds them all.  The slots of a plane are cut into `nbands` bands of W <= FF_MAPS_BAND_WORDS words
// (32 KB: two bands at 128 bins, one up to 90) and the grid is (slices of the walkers) x (planes that have samples) x (bands): a
// workgroup walks its slice's walkers, forms the samples of ITS plane only -- so the sample arithmetic is done once per band, not once
// per plane and band of the whole map -- and adds those whose slot lies in its band to an LDS-private histogram with non-returning
// integer adds (ds_add_u32).  At the end it adds its non-zero slots straight to `sum` with 64-bit global integer atomics.
// Weighed against it: opting in to more than 64 KB of LDS per launch (one workgroup holds a whole plane; a device
// attribute set at run time, one workgroup of 64 KB + 8 B per 160 KB compute unit where two bands leave room for four) and a smaller
// LDS tile with global adds outside it (the occupied part of a plane is not known before the walkers are read).
// A lane reads the row of its own walker from global memory: the rows of a wave are one contiguous span, every line of it is used
// whole, and the partner loop's re-reads are served by the vector cache; staging the rows in LDS (ff_observe.h) would take the
// room of a co-resident workgroup.  A slice is at least FF_MAPS_MIN_TILES tiles of blockDim.x walkers: the flush of a band costs up
// to W global atomics, so a workgroup must bring many more samples than its band has occupied cells.
// calls and walkers are added by one thread of the launch that closes the call.  No floating-point atomics anywhere: every word is
// an exact integer whatever the order, the grid or the number of ranks.
#pragma once
#include "ff_common.h"
#include "../../include/fermiflow_maps.h"

#define FF_MAPS_MAX_LAUNCH ((int64_t)1 << 22)  // walkers per launch: 2^22 x 552 ordered pairs < 2^32, so no uint32 LDS slot can wrap whatever the grid
#define FF_MAPS_BAND_WORDS 8193          // LDS words of a band: half the 128^2 + 2 slots of the largest plane
#define FF_MAPS_MIN_TILES 8              // tiles of blockDim.x walkers a workgroup takes at least (while the batch has them)
#define FF_MAPS_GRID_PER_CU 4            // persistent grid: workgroups per compute unit (four bands of 32 KB fit the CU's 160 KB)
#define FF_MAPS_SLOTS(nbins) ((nbins) * (nbins) + 2)

// slot of the sample (p, q) within its plane; ok: every coordinate that entered it (and rho) is finite
FF_D int ff_maps_slot(bool ok, double p, double q, double L, double scale, int nbins) {
  const double big = 1.7976931348623157e308;
  if (!(ok && fabs(p) <= big && fabs(q) <= big)) return nbins * nbins + 1;
  const double a = (p + L) * scale, b = (q + L) * scale, nb = (double)nbins;
  if (!(a >= 0.0 && a < nb && b >= 0.0 && b < nb)) return nbins * nbins;
  return (int)a * nbins + (int)b;
}

// gridDim.x = nslice x nact x nbands; dynamic LDS: W uint32.  planes: the nact planes that have samples, three bits each.
// B, x: the walkers of this launch.  call_walkers: the walkers of the whole call if this launch closes it, 0 if another launch of the
// same call follows on the stream.
__global__ void __launch_bounds__(256)
ff_maps_kernel(int64_t B, int nup, int n, const double* __restrict__ x, double L, double scale, int nbins, unsigned planes, int nact,
               int nbands, int W, int64_t call_walkers, unsigned long long* __restrict__ acc) {
  FF_DYN_LDS(lds);
  unsigned* const hist = reinterpret_cast<unsigned*>(lds);
  const int t = threadIdx.x, nt = blockDim.x;
  const int per = nact * nbands, nslice = (int)gridDim.x / per;
  const int slice = (int)blockIdx.x / per, rem = (int)blockIdx.x - slice * per, pa = rem / nbands, band = rem - pa * nbands;
  const int plane = (int)(planes >> (3 * pa)) & 7;
  const int P = FF_MAPS_SLOTS(nbins), c0 = band * W, nw = (P - c0 < W ? P - c0 : W);      // this band: slots [c0, c0 + nw)
  for (int k = t; k < nw; k += nt) hist[k] = 0u;
  __syncthreads();
  // plane -> species of the reference particle i and of the partner j (lab planes: i alone)
  const bool lab = plane < 2;
  const int si = lab ? plane : (plane - 2) >> 1, sj = lab ? si : (plane - 2) & 1;
  const int i0 = si ? nup : 0, i1 = si ? n : nup, j0 = sj ? nup : 0, j1 = sj ? n : nup;
  const double big = 1.7976931348623157e308;
  const int64_t ntiles = (B + nt - 1) / nt;
  for (int64_t tile = slice; tile < ntiles; tile += nslice) {
    const int64_t b = tile * nt + t;
    if (b >= B) continue;
    const double* __restrict__ row = x + b * (2 * n);
    for (int i = i0; i < i1; i++) {
      const double xi = row[2 * i], yi = row[2 * i + 1];
      const bool oki = fabs(xi) <= big && fabs(yi) <= big;
      if (lab) {
        const unsigned s = (unsigned)(ff_maps_slot(oki, xi, yi, L, scale, nbins) - c0);
        if (s < (unsigned)nw) atomicAdd(&hist[s], 1u);
        continue;
      }
      const double rho = sqrt(xi * xi + yi * yi);
      const bool okr = oki && rho <= big;
      const double c = rho == 0.0 ? 1.0 : xi / rho, sn = rho == 0.0 ? 0.0 : yi / rho;
      for (int j = j0; j < j1; j++) {
        if (j == i) continue;
        const double xj = row[2 * j], yj = row[2 * j + 1];
        const bool ok = okr && fabs(xj) <= big && fabs(yj) <= big;
        const double p = c * xj + sn * yj, q = c * yj - sn * xj;
        const unsigned s = (unsigned)(ff_maps_slot(ok, p, q, L, scale, nbins) - c0);
        if (s < (unsigned)nw) atomicAdd(&hist[s], 1u);
      }
    }
  }
  __syncthreads();
  // the workgroup's counts -> sum (non-zero slots only)
  unsigned long long* const sum = acc + 2 + (size_t)plane * P + c0;
  for (int k = t; k < nw; k += nt) {
    const unsigned cnt = hist[k];
    if (cnt) atomicAdd(&sum[k], (unsigned long long)cnt);
  }
  if (call_walkers != 0 && blockIdx.x == 0 && t == 0) {
    atomicAdd(&acc[0], 1ull);
    atomicAdd(&acc[1], (unsigned long long)call_walkers);
  }
}
