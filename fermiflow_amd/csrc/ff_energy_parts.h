// ff_energy_parts.h -- the energy components of the physical walkers (kinetic by two estimators, trap, Coulomb repulsion by spin pair),
// their first and second moments and their per-state sums, accumulated on the device (ff_energy_parts_accumulate).  Contract, accumulator
// layout and the determinism rules: include/fermiflow_energy.h.
//
// ff_energy_parts_kernel: ONE LANE PER WALKER, the idiom of ff_observe.h.  A workgroup of `nwave` waves (4, 2 or 1 by the size of a staged
// row) takes CHUNKS of FF_ENERGY_CHUNK consecutive walkers (chunk = blockIdx.x, + gridDim.x, ...); a wave takes the chunk's tiles of 64
// walkers (tile = wave, + nwave, ...) and everything about a tile stays inside the wave (FF_WAVE_SYNC, no workgroup barrier):
//   stage   the contiguous span of the tile's coordinates goes through the wave's LDS region with coalesced loads (row stride n d | 1
//           doubles: conflict-free when every lane then reads its own walker); every lane walks its n one-body terms and, unless Z == 0,
//           its n (n - 1) / 2 pairs.  The same region then takes the tile's gradients for |grad|^2.
//   rows    the lane leaves its six centred components and its valid flag (zeros for an invalid or absent walker) in the region, row
//           stride 7 doubles (odd: the lanes' stores fall on different banks).
//   reduce  lane (s, q), s < 2, q < 28, sums quantity q -- a sum, a second moment k <= l, the valid count -- over the 32 walkers of
//           segment s of the tile in walker order, one fused multiply-add each, and stores it in the workgroup's segment table.
// After one workgroup barrier 28 threads add the chunk's 8 segments in order and write the chunk's partials to the workspace.  The
// workgroup that draws the last ticket reads the partials back through LDS (coalesced, `fold_chunks` chunks at a time), adds them in
// chunk order and adds the totals to the accumulator.
//
// ff_energy_state_kernel: one workgroup per state over its sorted range of the components the first kernel left in the workspace, fixed
// tree (ff_state_sums_kernel's), eight numbers: the valid count, the six centred sums and the sum of squares of the centred energy.
#pragma once
#include "ff_common.h"
#include "../../include/fermiflow_energy.h"

#define FF_EP_MAX_COORD 60               // n d of the staged rows
#define FF_EP_ROW 7                      // six centred components and the valid flag
#define FF_EP_SEGW 32                    // walkers per segment: two segments per tile, eight per chunk
#define FF_EP_NSEG (FF_ENERGY_CHUNK / FF_EP_SEGW)
#define FF_EP_LDS_BYTES (65536 - 64)     // the 64 KB of a launch, less the static words
#define FF_EP_GRID_PER_CU 4              // grid cap: workgroups per compute unit
#define FF_EP_BIG 1.7976931348623157e308

// quantity q in [6, 27) -> its pair k <= l of components, row-major over the upper triangle
FF_D void ff_ep_pair(int q, int& k, int& l) {
  int r = q - FF_ENERGY_PARTS;
  k = 0;
#pragma unroll
  for (int u = 0; u < FF_ENERGY_PARTS - 1; u++)
    if (r >= FF_ENERGY_PARTS - k) { r -= FF_ENERGY_PARTS - k; k++; }
  l = k + r;
}

// the span of `tot` doubles at src -> rows of M doubles at row stride `stride` in the wave's region (ff_observe_kernel's staging)
FF_D void ff_ep_stage(const double* __restrict__ src, int tot, int M, int stride, unsigned magic, int lane, double* sx) {
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
}

// blockDim.x = 64 nwave; dynamic LDS: [FF_EP_NSEG x 28 segment partials | nwave regions of `region` doubles], region >= 64 (n d | 1) and
// >= 64 FF_EP_ROW.  magic = ceil(2^32 / (n d)): e / (n d) = umulhi(e, magic) for the e < 64 x 60 of a tile.  parts_ws: (B, 6) in the
// workspace when the per-state launch follows, else NULL.  fold_chunks = nwave region / 28: chunks per pass of the last workgroup.
__global__ void __launch_bounds__(256)
ff_energy_parts_kernel(int64_t B, int nup, int n, int d, double Z, const double* __restrict__ x, const double* __restrict__ grad,
                       const double* __restrict__ lap, const int* __restrict__ wstate, int nstates, const double* __restrict__ centre,
                       double* __restrict__ parts_out, double* __restrict__ parts_ws, unsigned magic, int region, int fold_chunks,
                       unsigned long long* __restrict__ acc, double* __restrict__ ws) {
  FF_DYN_LDS(lds);
  __shared__ unsigned s_last;
  const int t = threadIdx.x, nt = blockDim.x, lane = t & (FF_WAVE - 1), wave = t / FF_WAVE;
  const int M = n * d, stride = M | 1;
  double* const segs = lds;                                            // [segment][quantity]
  double* const pool = lds + FF_EP_NSEG * FF_ENERGY_PARTIAL;           // the waves' regions
  double* const sx = pool + wave * region;
  double ctr[FF_ENERGY_PARTS];
#pragma unroll
  for (int k = 0; k < FF_ENERGY_PARTS; k++) ctr[k] = centre ? centre[k] : 0.0;
  // what this lane sums in the reduce step: quantity rq over segment rs of the tile
  const int rs = lane / FF_ENERGY_PARTIAL, rq = lane - rs * FF_ENERGY_PARTIAL;
  int rk = rq, rl = FF_EP_ROW - 1;                                     // a sum: d_k x the flag (1 for the walkers that count, whose rows are not zero)
  if (rq >= FF_ENERGY_PARTS && rq < FF_ENERGY_PARTIAL - 1) ff_ep_pair(rq, rk, rl);
  if (rq == FF_ENERGY_PARTIAL - 1) rk = FF_EP_ROW - 1;                 // the count: flag x flag
  const int64_t nchunks = (B + FF_ENERGY_CHUNK - 1) / FF_ENERGY_CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t b0 = ch * FF_ENERGY_CHUNK;
    const int cn = (int)(B - b0 < FF_ENERGY_CHUNK ? B - b0 : FF_ENERGY_CHUNK);
    __syncthreads();                                   // (the previous chunk's segment table has been read)
    for (int w0 = wave * FF_WAVE; w0 < FF_ENERGY_CHUNK; w0 += nt) {
      const int nw = cn - w0 < 0 ? 0 : (cn - w0 < FF_WAVE ? cn - w0 : FF_WAVE);      // wave-uniform
      const int64_t b = b0 + w0 + lane;
      double c[FF_ENERGY_PARTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      bool valid = false;
      FF_WAVE_SYNC();                                  // (the previous tile's rows have been read)
      if (nw > 0) {
        ff_ep_stage(x + (b0 + w0) * M, nw * M, M, stride, magic, lane, sx);
        FF_WAVE_SYNC();
        if (lane < nw) {
          const double* row = sx + lane * stride;
          double ho = 0.0;
          for (int i = 0; i < M; i++) ho = fma(row[i], row[i], ho);
          c[2] = 0.5 * ho;
          if (Z != 0.0) {
            double suu = 0.0, sud = 0.0, sdd = 0.0;
            for (int i = 0; i < n; i++) {
              const double xi = row[i * d], yi = row[i * d + 1], zi = d == 3 ? row[i * d + 2] : 0.0;
              double si = 0.0, so = 0.0;                // partners of i's own species, of the other
              for (int j = i + 1; j < n; j++) {
                const double dx = xi - row[j * d], dy = yi - row[j * d + 1], dz = d == 3 ? zi - row[j * d + 2] : 0.0;
                const double inv = 1.0 / sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
                if ((i < nup) == (j < nup)) si += inv; else so += inv;
              }
              if (i < nup) { suu += si; sud += so; } else sdd += si;      // (i < j: a down i has down partners only)
            }
            c[3] = Z * suu; c[4] = Z * sud; c[5] = Z * sdd;
          }
        }
        FF_WAVE_SYNC();                                // (the coordinates have been read)
        ff_ep_stage(grad + (b0 + w0) * M, nw * M, M, stride, magic, lane, sx);
        FF_WAVE_SYNC();
        if (lane < nw) {
          const double* row = sx + lane * stride;
          double gg = 0.0;
          for (int i = 0; i < M; i++) gg = fma(row[i], row[i], gg);
          c[1] = 0.125 * gg;
          c[0] = fma(-0.25, lap[b], -c[1]);
          valid = fabs(c[0]) <= FF_EP_BIG && fabs(c[1]) <= FF_EP_BIG && fabs(c[2]) <= FF_EP_BIG && fabs(c[3]) <= FF_EP_BIG &&
                  fabs(c[4]) <= FF_EP_BIG && fabs(c[5]) <= FF_EP_BIG;
          if (nstates > 0) { const int st = wstate[b]; valid = valid && st >= 0 && st < nstates; }
#pragma unroll
          for (int k = 0; k < FF_ENERGY_PARTS; k++) {
            if (parts_out) parts_out[b * FF_ENERGY_PARTS + k] = c[k];
            if (parts_ws) parts_ws[b * FF_ENERGY_PARTS + k] = c[k];
          }
        }
        FF_WAVE_SYNC();                                // (the gradients have been read)
      }
#pragma unroll
      for (int k = 0; k < FF_ENERGY_PARTS; k++) sx[lane * FF_EP_ROW + k] = valid ? c[k] - ctr[k] : 0.0;
      sx[lane * FF_EP_ROW + FF_EP_ROW - 1] = valid ? 1.0 : 0.0;
      FF_WAVE_SYNC();
      if (lane < 2 * FF_ENERGY_PARTIAL) {
        const double* row = sx + rs * FF_EP_SEGW * FF_EP_ROW;
        double a = 0.0;
        for (int w = 0; w < FF_EP_SEGW; w++) a = fma(row[w * FF_EP_ROW + rk], row[w * FF_EP_ROW + rl], a);
        segs[(w0 / FF_EP_SEGW + rs) * FF_ENERGY_PARTIAL + rq] = a;
      }
    }
    __syncthreads();
    if (t < FF_ENERGY_PARTIAL) {
      double a = segs[t];
      for (int s = 1; s < FF_EP_NSEG; s++) a += segs[s * FF_ENERGY_PARTIAL + t];
      ws[ch * FF_ENERGY_PARTIAL + t] = a;
    }
  }
  unsigned long long* const ticket = acc + 3;
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(ticket, 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // the last workgroup: the chunks in chunk order.  The first 52 words but the ticket are touched here only.
  double tot = 0.0;
  for (int64_t c0 = 0; c0 < nchunks; c0 += fold_chunks) {
    const int nc = (int)(nchunks - c0 < fold_chunks ? nchunks - c0 : fold_chunks);
    __syncthreads();
    for (int e = t; e < nc * FF_ENERGY_PARTIAL; e += nt) pool[e] = ws[c0 * FF_ENERGY_PARTIAL + e];
    __syncthreads();
    if (t < FF_ENERGY_PARTIAL) {                       // eight LDS loads ahead of their additions; the order of the additions is the chunks'
      int c = 0;
      for (; c + 8 <= nc; c += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = pool[(c + u) * FF_ENERGY_PARTIAL + t];
#pragma unroll
        for (int u = 0; u < 8; u++) tot += v[u];
      }
      for (; c < nc; c++) tot += pool[c * FF_ENERGY_PARTIAL + t];
    }
  }
  double* const sum = reinterpret_cast<double*>(acc + FF_ENERGY_HEAD), * const sum2 = sum + FF_ENERGY_PARTS,
        * const blocksq = sum2 + FF_ENERGY_PARTS * FF_ENERGY_PARTS;
  if (t < FF_ENERGY_PARTS) {
    sum[t] += tot;
    blocksq[t] += tot * tot;
  } else if (t < FF_ENERGY_PARTIAL - 1) {
    int k, l;
    ff_ep_pair(t, k, l);
    sum2[k * FF_ENERGY_PARTS + l] += tot;
    if (l != k) sum2[l * FF_ENERGY_PARTS + k] += tot;
  } else if (t == FF_ENERGY_PARTIAL - 1) {
    const unsigned long long nv = (unsigned long long)tot;            // (an exact integer below 2^31)
    acc[0] += 1ull;
    acc[1] += nv;
    acc[2] += (unsigned long long)B - nv;
  }
  if (t == 0) atomicExch(ticket, 0ull);
}

// parts (B, 6): the components of every walker as the kernel above computed them; a walker of a state's range counts if all six are
// finite (its state is in range by construction)
__global__ void __launch_bounds__(256)
ff_energy_state_kernel(int64_t B, const int* __restrict__ wstate, const double* __restrict__ parts, const double* __restrict__ centre,
                       int nstates, unsigned long long* __restrict__ acc) {
  __shared__ double sm[8][256];
  const int s = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  auto lower = [&](int key) -> int64_t {   // first index with wstate[i] >= key
    int64_t lo = 0, hi = B;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (wstate[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
  };
  const int64_t b0 = lower(s), b1 = lower(s + 1);
  double ctr[FF_ENERGY_PARTS];
#pragma unroll
  for (int k = 0; k < FF_ENERGY_PARTS; k++) ctr[k] = centre ? centre[k] : 0.0;
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};             // count, six sums, sum of squares of the centred energy
  for (int64_t i = b0 + t; i < b1; i += nt) {
    double dk[FF_ENERGY_PARTS];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < FF_ENERGY_PARTS; k++) {
      const double c = parts[i * FF_ENERGY_PARTS + k];
      ok = ok && fabs(c) <= FF_EP_BIG;
      dk[k] = c - ctr[k];
    }
    if (ok) {
      const double de = (((dk[0] + dk[2]) + dk[3]) + dk[4]) + dk[5];
      a[0] += 1.0;
#pragma unroll
      for (int k = 0; k < FF_ENERGY_PARTS; k++) a[1 + k] += dk[k];
      a[7] = fma(de, de, a[7]);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; k++) sm[k][t] = a[k];
  __syncthreads();
  int w = 1;
  while (w * 2 < nt) w *= 2;
  for (; w > 0; w >>= 1) {
    if (t < w && t + w < nt) {
#pragma unroll
      for (int k = 0; k < 8; k++) sm[k][t] += sm[k][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    const size_t S = (size_t)nstates;
    double* const f = reinterpret_cast<double*>(acc);
    acc[FF_ENERGY_FIXED + s] += (unsigned long long)sm[0][0];
#pragma unroll
    for (int k = 0; k < FF_ENERGY_PARTS; k++) f[FF_ENERGY_FIXED + S + (size_t)s * FF_ENERGY_PARTS + k] += sm[1 + k][0];
    f[FF_ENERGY_FIXED + 7 * S + s] += sm[7][0];
  }
}
