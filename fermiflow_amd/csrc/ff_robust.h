// ff_robust.h -- the opt-in robust ground-state estimator (ff_energy_robust / ff_energy_robust_apply, include/fermiflow_robust.h, which
// states the contract: valid walkers, the lower median m, the width a, the window [lo, hi], clipped energies, gradient weights u).
//
// Launches of ff_energy_robust (N walkers, segments of FF_ROB_SEG):
//   1-6  ff_robust_select_kernel, pass p = 0 .. 5: an exact radix select on the order-preserving 64-bit keys, FF_ROBUST_DIGIT_BITS = 11
//        bits per pass from the top (the last pass: the 9 that remain).  Pass p counts the digit of the keys whose higher digits equal
//        the prefix chosen so far; the workgroup that draws the last ticket folds the histogram, picks the digit that holds the target
//        rank and leaves prefix and remaining rank in the workspace for the next pass.  Pass 0 counts every valid key, so it also
//        yields n_v; the last pass writes n_v and m to stat and clears the state.
//        Counting: the leading digits of local energies near 30 are the same for the whole batch, so a plain histogram would put the
//        64 lanes of every wave on ONE LDS address (and 65 536 global atomics on one address took 6 ms in ff_state_sums_kernel).  A wave
//        therefore first finds, for every lane, the lanes that hold the same digit -- one ballot per digit bit: 11 v_cmp + scalar
//        and/andn2, no loop over distinct digits and no divergence -- and the lowest lane of each group issues ONE LDS add of the
//        group's size.  The histogram is private to the workgroup (2048 x uint32, 8 KB) and flushed once, non-zero bins only, with
//        global integer atomics: at 65 536 walkers 64 adds on the leading digit's word.  Integers only: the result does not depend on
//        the grid or on the order of anything.
//   7    ff_robust_moments_kernel: sum |e - m|, sum (e - c0), sum (e - c0)^2 over the valid walkers (c0 = the finite shift), fixed tree
//        per segment, partials joined in segment order by the last workgroup, which goes on to a, lo, hi, E, E_ss.
//   8    ff_robust_clip_kernel: sum (c - m) and n_c the same way; the finish gives Ec = m + sum / n_v.  (Its window comes out of
//        launch 7's finish, so fusing the two would take a second pass over a reduction that has not finished.)
// ff_energy_robust_apply is ff_robust_apply_kernel: u, the sanitised rows, sum l (c - Ec) with the same join.
//
// Workspace (uint64 words; zeroed by the caller once): [0] ticket  [1] prefix  [2] remaining rank  [3] n_v  [4, 8) unused
//   [8, 8 + 2048) histogram   then 4 doubles per segment: the partial sums of the launch that runs (scratch, need not be zero).
#pragma once
#include "ff_common.h"
#include "../../include/fermiflow_robust.h"

#define FF_ROB_BINS (1 << FF_ROBUST_DIGIT_BITS)
#define FF_ROB_SEG 1024                  // walkers per segment; a multiple of the block size (the ballots want a uniform trip count)
#define FF_ROB_THREADS 256
#define FF_ROB_MAX_GRID 1024             // workgroups of a selection pass (each flushes its histogram once); more segments: grid stride
#define FF_ROB_MAX_N ((int64_t)1 << 31)  // walkers per call (exclusive): no uint32 LDS bin can wrap
#define FF_ROB_MAX_COORD 60
#define FF_ROB_W_TICKET 0
#define FF_ROB_W_PREFIX 1
#define FF_ROB_W_RANK 2
#define FF_ROB_W_NV 3
#define FF_ROB_W_HIST 8
#define FF_ROB_HDR (FF_ROB_W_HIST + FF_ROB_BINS)
#define FF_ROB_PART 4                    // doubles of partial sums per segment

FF_D bool ff_rob_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for NaN)
// the order-preserving map of a double to uint64 and back
FF_D unsigned long long ff_rob_key(double v) {
  const unsigned long long u = ((unsigned long long)(unsigned)__double2hiint(v) << 32) | (unsigned long long)(unsigned)__double2loint(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
FF_D double ff_rob_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __hiloint2double((int)(unsigned)(u >> 32), (int)(unsigned)(u & 0xffffffffull));
}
FF_D bool ff_rob_valid(const double* __restrict__ e, const double* __restrict__ logp, int64_t j, double& v) {
  v = e[j];
  return ff_rob_finite(v) && (logp == nullptr || ff_rob_finite(logp[j]));
}
// digit p of a key: bits [shift, shift + width)
FF_D int ff_rob_shift(int pass) { return pass < FF_ROBUST_PASSES - 1 ? 64 - FF_ROBUST_DIGIT_BITS * (pass + 1) : 0; }
FF_D int ff_rob_width(int pass) { return pass < FF_ROBUST_PASSES - 1 ? FF_ROBUST_DIGIT_BITS : 64 - FF_ROBUST_DIGIT_BITS * (FF_ROBUST_PASSES - 1); }

__global__ void __launch_bounds__(FF_ROB_THREADS)
ff_robust_select_kernel(int64_t N, const double* __restrict__ e, const double* __restrict__ logp, int pass,
                        unsigned long long* __restrict__ ws, double* __restrict__ stat) {
  __shared__ unsigned lh[FF_ROB_BINS];
  __shared__ unsigned long long sc[FF_ROB_THREADS];
  __shared__ unsigned s_last;
  const int t = threadIdx.x, nt = blockDim.x, lane = t & (FF_WAVE - 1);
  const int shift = ff_rob_shift(pass), width = ff_rob_width(pass), nb = 1 << width, hs = shift + width;
  const unsigned long long prefix = ws[FF_ROB_W_PREFIX];       // (written by the previous pass's launch)
  for (int k = t; k < FF_ROB_BINS; k += nt) lh[k] = 0u;
  __syncthreads();
  const int64_t nseg = (N + FF_ROB_SEG - 1) / FF_ROB_SEG;
  for (int64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x)
    for (int k = t; k < FF_ROB_SEG; k += nt) {                 // every lane of a wave makes every trip: the ballots are wave-wide
      const int64_t j = seg * FF_ROB_SEG + k;
      bool act = false;
      unsigned dg = 0u;
      if (j < N) {
        double v;
        if (ff_rob_valid(e, logp, j, v)) {
          const unsigned long long key = ff_rob_key(v);
          if (pass == 0 || (key >> hs) == (prefix >> hs)) { act = true; dg = (unsigned)(key >> shift) & (unsigned)(nb - 1); }
        }
      }
      unsigned long long peers = __ballot(act);
      if (peers == 0ull) continue;                             // (wave-uniform)
      for (int bit = 0; bit < width; bit++) {                  // the lanes that hold this lane's digit
        const bool one = (dg >> bit) & 1u;
        const unsigned long long b = __ballot(act && one);
        peers &= one ? b : ~b;
      }
      if (act && (peers & (~peers + 1ull)) == (1ull << lane)) atomicAdd(&lh[dg], (unsigned)__popcll(peers));
    }
  __syncthreads();
  unsigned long long* const hist = ws + FF_ROB_W_HIST;
  for (int k = t; k < nb; k += nt) {
    const unsigned c = lh[k];
    if (c) atomicAdd(&hist[k], (unsigned long long)c);
  }
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(&ws[FF_ROB_W_TICKET], 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // the last workgroup.  Thread t folds bins [t C, (t + 1) C): every word other workgroups added to is read by a returning atomic,
  // which also clears it; the totals (below 2^31) are kept in the LDS histogram for the walk through the chosen chunk
  const int C = (nb + nt - 1) / nt, k0 = t * C < nb ? t * C : nb, k1 = k0 + C < nb ? k0 + C : nb;
  unsigned long long mine = 0ull;
  for (int k = k0; k < k1; k++) {
    const unsigned long long c = atomicExch(&hist[k], 0ull);
    lh[k] = (unsigned)c;
    mine += c;
  }
  sc[t] = mine;
  __syncthreads();
  for (int off = 1; off < nt; off <<= 1) {                     // inclusive scan over the threads' chunks
    const unsigned long long v = t >= off ? sc[t - off] : 0ull;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  const unsigned long long incl = sc[t], excl = incl - mine, total = sc[nt - 1];
  const unsigned long long nv = pass == 0 ? total : ws[FF_ROB_W_NV];
  const unsigned long long r = pass == 0 ? (nv ? (nv - 1ull) / 2ull : 0ull) : ws[FF_ROB_W_RANK];
  __syncthreads();                                             // (everybody has read the state before anybody writes it)
  const bool lastpass = pass == FF_ROBUST_PASSES - 1;
  if (nv > 0ull && excl <= r && r < incl) {                    // the one thread whose chunk holds the target rank
    unsigned long long rr = r - excl;
    int digit = k0;
    for (int k = k0; k < k1; k++) {
      const unsigned long long c = lh[k];
      if (rr < c) { digit = k; break; }
      rr -= c;
    }
    const unsigned long long np = (pass == 0 ? 0ull : prefix) | ((unsigned long long)digit << shift);
    if (!lastpass) {
      ws[FF_ROB_W_PREFIX] = np; ws[FF_ROB_W_RANK] = rr; ws[FF_ROB_W_NV] = nv;
    } else {
      stat[0] = (double)nv; stat[1] = ff_rob_unkey(np);
      ws[FF_ROB_W_PREFIX] = 0ull; ws[FF_ROB_W_RANK] = 0ull; ws[FF_ROB_W_NV] = 0ull;
    }
  }
  if (t == 0) {
    if (nv == 0ull) {                                          // no valid walker: the state stays zero, the median is NaN
      ws[FF_ROB_W_PREFIX] = 0ull; ws[FF_ROB_W_RANK] = 0ull; ws[FF_ROB_W_NV] = 0ull;
      if (lastpass) { stat[0] = 0.0; stat[1] = __longlong_as_double(0x7ff8000000000000ll); }
    }
    atomicExch(&ws[FF_ROB_W_TICKET], 0ull);
  }
}

// NV partial sums of this workgroup's segment -> part; the workgroup that finishes last joins the partials of all segments in segment
// order (thread t takes k = t, t + nt, ...; the tree joins the threads: one association whoever is last) and leaves the totals in
// sm[c][0].  Returns whether this workgroup is that one; the ticket is left at zero.
template <int NV>
FF_D bool ff_rob_join(double (*sm)[FF_ROB_THREADS], unsigned& s_last, const double* v, double* __restrict__ part,
                      unsigned long long* __restrict__ ticket) {
  const int t = threadIdx.x, nt = blockDim.x;
  int w0 = 1;
  while (w0 * 2 < nt) w0 *= 2;      // largest power of two below the block size
#pragma unroll
  for (int c = 0; c < NV; c++) sm[c][t] = v[c];
  __syncthreads();
  for (int w = w0; w > 0; w >>= 1) {
    if (t < w && t + w < nt) {
#pragma unroll
      for (int c = 0; c < NV; c++) sm[c][t] += sm[c][t + w];
    }
    __syncthreads();
  }
  if (t < NV) part[(int64_t)blockIdx.x * FF_ROB_PART + t] = sm[t][0];
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(ticket, 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  double s[NV];
#pragma unroll
  for (int c = 0; c < NV; c++) s[c] = 0.0;
  for (int k = t; k < (int)gridDim.x; k += nt) {
#pragma unroll
    for (int c = 0; c < NV; c++) s[c] += part[(int64_t)k * FF_ROB_PART + c];
  }
#pragma unroll
  for (int c = 0; c < NV; c++) sm[c][t] = s[c];
  __syncthreads();
  for (int w = w0; w > 0; w >>= 1) {
    if (t < w && t + w < nt) {
#pragma unroll
      for (int c = 0; c < NV; c++) sm[c][t] += sm[c][t + w];
    }
    __syncthreads();
  }
  if (t == 0) atomicExch(ticket, 0ull);
  return true;
}

// grid: one workgroup per segment
__global__ void __launch_bounds__(FF_ROB_THREADS)
ff_robust_moments_kernel(int64_t N, const double* __restrict__ e, const double* __restrict__ logp, const double* __restrict__ shift_dev,
                         double kclip, double* __restrict__ stat, double* __restrict__ part, unsigned long long* __restrict__ ticket) {
  __shared__ double sm[3][FF_ROB_THREADS];
  __shared__ unsigned s_last;
  const double c0 = ff_finite_shift(shift_dev[0]), nv = stat[0], m = stat[1];
  const int t = threadIdx.x, nt = blockDim.x;
  const int64_t j0 = (int64_t)blockIdx.x * FF_ROB_SEG;
  double v3[3] = {0.0, 0.0, 0.0};
  for (int k = t; k < FF_ROB_SEG && j0 + k < N; k += nt) {
    double v;
    if (ff_rob_valid(e, logp, j0 + k, v)) {
      const double dv = v - c0;
      v3[0] += fabs(v - m); v3[1] += dv; v3[2] = fma(dv, dv, v3[2]);
    }
  }
  if (!ff_rob_join<3>(sm, s_last, v3, part, ticket)) return;
  if (t == 0) {
    const double a = sm[0][0] / nv, d = sm[1][0] / nv;            // (n_v = 0: 0 / 0, every statistic NaN)
    double ss = sm[2][0] - sm[1][0] * d;                          // sum (e - E)^2 = sum (e - c0)^2 - n_v (E - c0)^2
    if (sm[2][0] > 1.7976931348623157e308) ss = sm[2][0];         // (squares that left the double range: +inf, not inf - inf)
    stat[2] = a; stat[3] = m - kclip * a; stat[4] = m + kclip * a;
    stat[5] = c0 + d; stat[6] = ss < 0.0 ? 0.0 : ss;
  }
}

__global__ void __launch_bounds__(FF_ROB_THREADS)
ff_robust_clip_kernel(int64_t N, const double* __restrict__ e, const double* __restrict__ logp, double* __restrict__ stat,
                      double* __restrict__ part, unsigned long long* __restrict__ ticket) {
  __shared__ double sm[2][FF_ROB_THREADS];
  __shared__ unsigned s_last;
  const double nv = stat[0], m = stat[1], lo = stat[3], hi = stat[4];
  const int t = threadIdx.x, nt = blockDim.x;
  const int64_t j0 = (int64_t)blockIdx.x * FF_ROB_SEG;
  double v2[2] = {0.0, 0.0};
  for (int k = t; k < FF_ROB_SEG && j0 + k < N; k += nt) {
    double v;
    if (ff_rob_valid(e, logp, j0 + k, v)) {
      const double c = fmin(fmax(v, lo), hi);
      v2[0] += c - m; v2[1] += c != v ? 1.0 : 0.0;
    }
  }
  if (!ff_rob_join<2>(sm, s_last, v2, part, ticket)) return;
  if (t == 0) { stat[7] = m + sm[0][0] / nv; stat[8] = sm[1][0]; }
}

__global__ void __launch_bounds__(FF_ROB_THREADS)
ff_robust_apply_kernel(int64_t B, int n, int d, const double* __restrict__ e, const double* __restrict__ logp, double* __restrict__ stat,
                       double n_global, int finish, double* __restrict__ u, double* __restrict__ z, double* __restrict__ g,
                       double* __restrict__ sum_out, double* __restrict__ part, unsigned long long* __restrict__ ticket) {
  __shared__ double sm[1][FF_ROB_THREADS];
  __shared__ unsigned s_last;
  const double nv = stat[0], lo = stat[3], hi = stat[4], ec = stat[7], ratio = n_global / nv;
  const int t = threadIdx.x, nt = blockDim.x, M = n * d;
  const int64_t j0 = (int64_t)blockIdx.x * FF_ROB_SEG;
  double v1[1] = {0.0};
  for (int k = t; k < FF_ROB_SEG && j0 + k < B; k += nt) {
    const int64_t b = j0 + k;
    const double v = e[b], l = logp[b];
    if (ff_rob_finite(v) && ff_rob_finite(l)) {
      const double dc = fmin(fmax(v, lo), hi) - ec;
      u[b] = dc * ratio;
      v1[0] = fma(l, dc, v1[0]);
    } else {
      u[b] = 0.0;
      if (z)                       // failed walkers are rare: the row is written by the walker's own lane
        for (int i = 0; i < M; i++) { z[b * M + i] = i % d == 0 ? FF_ROBUST_SAFE_STEP * (double)(i / d + 1) : 0.0; g[b * M + i] = 0.0; }
    }
  }
  if (!ff_rob_join<1>(sm, s_last, v1, part, ticket)) return;
  if (t == 0) {
    sum_out[0] = sm[0][0];
    if (finish) stat[9] = sm[0][0] / nv;
  }
}
