// ff_dmc.h -- the three small kernels of fixed-node diffusion Monte Carlo on the trained wave function (ff_dmc_propose, ff_dmc_accept,
// ff_dmc_comb).  Contract, the order of every sum and the record's layout: include/fermiflow_dmc.h.
//
// ff_dmc_propose_kernel: one lane per group of four coordinates (a Philox block is four normals).
// ff_dmc_accept_kernel: ONE LANE PER WALKER; a workgroup of 256 takes chunks of FF_DMC_CHUNK walkers (chunk = blockIdx.x, + gridDim.x,
//   ...).  Every lane leaves its nine record entries in a row of LDS (row stride 9 doubles, odd: the lanes' stores fall on different
//   banks); thread (s, q), s < 8, q < 9, folds quantity q over the 32 walkers of segment s in walker order; nine threads add the
//   segments in order and write the chunk's partials to the workspace.  The workgroup that draws the last ticket adds the chunks in
//   chunk order and writes the record (ff_energy_parts_kernel's scheme).
// ff_dmc_comb: three launches.  ff_dmc_cum_kernel: a chunk's weights go through LDS, one thread forms their left-to-right partial
//   sums (the association is the contract) and the last-ticket workgroup scans the chunk totals in tiles of 256.
//   ff_dmc_resample_kernel: one lane per slot, binary search over cum_j = P[j / 256] + loc[j], the gather, w = 1.
//   ff_dmc_comb_stats_kernel: src is non-decreasing, so a source's copies are a run; the first lane of a run finds its end by binary
//   search.  Integer atomics only.
// The drift, the proposal and the two Green's-function exponents are evaluated without fused multiply-adds: the header states plain IEEE
// arithmetic, and a numpy restatement reproduces it bit for bit.  The library is built with -ffp-contract=fast, under which the backend
// fuses a product into the addition that follows whatever the source says, so every product that feeds an addition goes through
// ff_dmc_mul: the rounded product is made opaque (FF_OPAQUE, no instruction) before it is used.
#pragma once
#include "ff_common.h"
#include "ff_rng.h"
#include "../../include/fermiflow_dmc.h"

#define FF_DMC_SEGW 32                   // walkers per segment: eight segments per chunk
#define FF_DMC_NSEG (FF_DMC_CHUNK / FF_DMC_SEGW)
#define FF_DMC_GRID_PER_CU 4             // grid cap: workgroups per compute unit
#define FF_DMC_BIG 1.7976931348623157e308
#define FF_DMC_HEAD 4                    // words in front of the comb's arrays: ticket, W, last positive walker, unused

FF_D bool ff_dmc_finite(double v) { return fabs(v) <= FF_DMC_BIG; }

// a * b rounded to a double of its own: never the first half of a fused multiply-add
FF_D double ff_dmc_mul(double a, double b) {
  double p = a * b;
  FF_OPAQUE(p);
  return p;
}

// the limited drift of one particle from its gradient of log p; c = (2 a) tau
FF_D void ff_dmc_drift(double gx, double gy, double c, double& bx, double& by) {
  const double vx = 0.5 * gx, vy = 0.5 * gy;
  const double v2 = ff_dmc_mul(vx, vx) + ff_dmc_mul(vy, vy);
  const double s = 2.0 / (1.0 + sqrt(1.0 + ff_dmc_mul(c, v2)));
  bx = vx * s;
  by = vy * s;
}

// Q = ceil(n / 2) quads per walker; sqrt_tau and c = (2 a) tau come from the host
__global__ void __launch_bounds__(256)
ff_dmc_propose_kernel(int64_t B, int n, int Q, double tau, double sqrt_tau, double c, const double* __restrict__ x,
                      const double* __restrict__ grad, const double* __restrict__ noise, uint64_t seed, uint64_t woff, uint32_t step,
                      double* __restrict__ x_new, double* __restrict__ xi_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * Q) return;
  const int64_t b = e / Q;
  const int quad = (int)(e - b * Q);
  const int np = n - 2 * quad < 2 ? n - 2 * quad : 2;       // particles of this quad: 2, or 1 at the tail of an odd n
  const int64_t o = (b * n + 2 * quad) * 2;
  double z[4];
  if (noise) {
    for (int k = 0; k < 2 * np; k++) z[k] = noise[o + k];
  } else {
    ff_normal_quad(seed, woff + (uint64_t)b, step, (uint32_t)quad, z);
  }
  for (int p = 0; p < np; p++) {
    double bx, by;
    ff_dmc_drift(grad[o + 2 * p], grad[o + 2 * p + 1], c, bx, by);
    x_new[o + 2 * p] = (x[o + 2 * p] + ff_dmc_mul(tau, bx)) + ff_dmc_mul(sqrt_tau, z[2 * p]);
    x_new[o + 2 * p + 1] = (x[o + 2 * p + 1] + ff_dmc_mul(tau, by)) + ff_dmc_mul(sqrt_tau, z[2 * p + 1]);
    if (xi_out) { xi_out[o + 2 * p] = z[2 * p]; xi_out[o + 2 * p + 1] = z[2 * p + 1]; }
  }
}

// blockDim.x = FF_DMC_CHUNK.  ws: [ticket | nchunks x FF_DMC_REC partials]
__global__ void __launch_bounds__(256)
ff_dmc_accept_kernel(int64_t B, int n, double tau, double c, double* __restrict__ x, double* __restrict__ logp, double* __restrict__ grad,
                     double* __restrict__ eloc, double* __restrict__ sign, double* __restrict__ w, const double* __restrict__ x_new,
                     const double* __restrict__ logp_new, const double* __restrict__ grad_new, const double* __restrict__ eloc_new,
                     const double* __restrict__ sign_new, const double* __restrict__ u, uint64_t seed, uint64_t woff, uint32_t step,
                     const double* __restrict__ ctrl, double* __restrict__ rec, uint8_t* __restrict__ accepted_out,
                     unsigned long long* __restrict__ ws) {
  __shared__ double rows[FF_DMC_CHUNK * FF_DMC_REC];
  __shared__ double segs[FF_DMC_NSEG * FF_DMC_REC];
  __shared__ unsigned s_last;
  const int t = threadIdx.x;
  const double e_t = ctrl[0], lo = ctrl[1] - ctrl[2], hi = ctrl[1] + ctrl[2];
  double* const part = reinterpret_cast<double*>(ws + 1);
  const int rs = t / FF_DMC_REC, rq = t - rs * FF_DMC_REC;      // what this thread folds: quantity rq over segment rs
  const int64_t nchunks = (B + FF_DMC_CHUNK - 1) / FF_DMC_CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t b = ch * FF_DMC_CHUNK + t;
    double r[FF_DMC_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (b < B) {
      const double lp = logp[b], e_old = eloc[b], sg = sign[b], w_old = w[b];
      const double lpn = logp_new[b], e_new = eloc_new[b], sgn = sign_new[b];
      bool alive = ff_dmc_finite(lp) && ff_dmc_finite(e_old) && ff_dmc_finite(sg) && ff_dmc_finite(w_old) && w_old >= 0.0;
      bool valid = ff_dmc_finite(lpn) && ff_dmc_finite(e_new) && ff_dmc_finite(sgn);
      double q;
      {
        double sf = 0.0, sb = 0.0;
        for (int i = 0; i < n; i++) {
          const int64_t o = (b * n + i) * 2;
          const double x0 = x[o], y0 = x[o + 1], x1 = x_new[o], y1 = x_new[o + 1];
          const double gx0 = grad[o], gy0 = grad[o + 1], gx1 = grad_new[o], gy1 = grad_new[o + 1];
          alive = alive && ff_dmc_finite(x0) && ff_dmc_finite(y0) && ff_dmc_finite(gx0) && ff_dmc_finite(gy0);
          valid = valid && ff_dmc_finite(x1) && ff_dmc_finite(y1) && ff_dmc_finite(gx1) && ff_dmc_finite(gy1);
          double bx, by;
          ff_dmc_drift(gx0, gy0, c, bx, by);
          const double dx = (x1 - x0) - ff_dmc_mul(tau, bx), dy = (y1 - y0) - ff_dmc_mul(tau, by);
          sf = sf + (ff_dmc_mul(dx, dx) + ff_dmc_mul(dy, dy));
          ff_dmc_drift(gx1, gy1, c, bx, by);
          const double ex = (x0 - x1) - ff_dmc_mul(tau, bx), ey = (y0 - y1) - ff_dmc_mul(tau, by);
          sb = sb + (ff_dmc_mul(ex, ex) + ff_dmc_mul(ey, ey));
        }
        const double two_tau = 2.0 * tau;
        const double lf = -(sf / two_tau), lb = -(sb / two_tau);
        q = ((lpn - lp) + lb) - lf;
      }
      if (!alive) {
        w[b] = 0.0;
        r[8] = 1.0;
        if (accepted_out) accepted_out[b] = 0;
      } else {
        double p = 0.0;
        if (!valid) r[8] = 1.0;
        else if (!(sgn * sg > 0.0)) r[7] = 1.0;
        else p = q >= 0.0 ? 1.0 : (q < 0.0 ? exp(q) : 0.0);
        const double ub = u ? u[b] : ff_uniform(seed, woff + (uint64_t)b, step, FF_DMC_U_SLOT);
        const bool acc = ub < p;
        if (acc) {
          for (int i = 0; i < 2 * n; i++) { x[b * 2 * n + i] = x_new[b * 2 * n + i]; grad[b * 2 * n + i] = grad_new[b * 2 * n + i]; }
          logp[b] = lpn; eloc[b] = e_new; sign[b] = sgn;
        }
        if (accepted_out) accepted_out[b] = acc ? 1 : 0;
        const double e_now = acc ? e_new : e_old;
        const double mid = 0.5 * (fmin(fmax(e_old, lo), hi) + fmin(fmax(e_now, lo), hi));
        const double wn = w_old * exp(tau * (e_t - mid));
        w[b] = wn;
        const double we = wn * e_now;
        r[0] = wn; r[1] = we; r[2] = we * e_now; r[3] = wn * wn; r[4] = p; r[5] = wn; r[6] = acc ? 1.0 : 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < FF_DMC_REC; k++) rows[t * FF_DMC_REC + k] = r[k];
    __syncthreads();
    if (t < FF_DMC_NSEG * FF_DMC_REC) {
      const double* row = rows + rs * FF_DMC_SEGW * FF_DMC_REC + rq;
      double a = 0.0;
      if (rq == 5) { for (int k = 0; k < FF_DMC_SEGW; k++) a = fmax(a, row[k * FF_DMC_REC]); }
      else { for (int k = 0; k < FF_DMC_SEGW; k++) a += row[k * FF_DMC_REC]; }
      segs[t] = a;
    }
    __syncthreads();
    if (t < FF_DMC_REC) {
      double a = segs[t];
      for (int s = 1; s < FF_DMC_NSEG; s++) a = t == 5 ? fmax(a, segs[s * FF_DMC_REC + t]) : a + segs[s * FF_DMC_REC + t];
      part[ch * FF_DMC_REC + t] = a;
    }
  }
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(ws, 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (t < FF_DMC_REC) {      // the last workgroup: the chunks in chunk order
    double tot = 0.0;
    for (int64_t ch = 0; ch < nchunks; ch++) tot = t == 5 ? fmax(tot, part[ch * FF_DMC_REC + t]) : tot + part[ch * FF_DMC_REC + t];
    if (t < 6) rec[t] = tot;
    else reinterpret_cast<long long*>(rec)[t] = (long long)tot;      // (an exact integer below 2^31)
  }
  if (t == 0) atomicExch(ws, 0ull);
}

// blockDim.x = FF_DMC_CHUNK.  ws: [ticket, W, last positive walker, - | loc (B) | T (nchunks) | P (nchunks) | JL (nchunks)]
__global__ void __launch_bounds__(256)
ff_dmc_cum_kernel(int64_t B, const double* __restrict__ w, int* __restrict__ info, unsigned long long* __restrict__ ws) {
  __shared__ double s[FF_DMC_CHUNK];
  __shared__ double s_acc;
  __shared__ long long s_jl;
  __shared__ unsigned s_last;
  const int t = threadIdx.x;
  const int64_t nchunks = (B + FF_DMC_CHUNK - 1) / FF_DMC_CHUNK;
  double* const loc = reinterpret_cast<double*>(ws + FF_DMC_HEAD);
  double* const T = loc + B, * const P = T + nchunks;
  long long* const JL = reinterpret_cast<long long*>(P + nchunks);
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t b0 = ch * FF_DMC_CHUNK;
    const int cn = (int)(B - b0 < FF_DMC_CHUNK ? B - b0 : FF_DMC_CHUNK);
    double v = 0.0;
    if (t < cn) { v = w[b0 + t]; v = (v > 0.0 && v <= FF_DMC_BIG) ? v : 0.0; }
    __syncthreads();                                   // (the previous chunk's partial sums have been written out)
    s[t] = v;
    __syncthreads();
    if (t == 0) {                                      // left to right: the association of the contract
      double a = 0.0;
      long long jl = -1;
      for (int k = 0; k < cn; k++) {
        const double wk = s[k];
        if (wk > 0.0) jl = b0 + k;
        a += wk;
        s[k] = a;
      }
      T[ch] = a;
      JL[ch] = jl;
    }
    __syncthreads();
    if (t < cn) loc[b0 + t] = s[t];
  }
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(ws, 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (t == 0) { s_acc = 0.0; s_jl = -1; }
  for (int64_t c0 = 0; c0 < nchunks; c0 += FF_DMC_CHUNK) {      // the last workgroup: P_c, W and the last positive walker
    const int nc = (int)(nchunks - c0 < FF_DMC_CHUNK ? nchunks - c0 : FF_DMC_CHUNK);
    __syncthreads();
    if (t < nc) s[t] = T[c0 + t];
    __syncthreads();
    if (t == 0) {
      double a = s_acc;
      long long jl = s_jl;
      for (int k = 0; k < nc; k++) {
        const double tk = s[k];
        s[k] = a;
        a += tk;
        const long long j = JL[c0 + k];
        if (j > jl) jl = j;
      }
      s_acc = a; s_jl = jl;
    }
    __syncthreads();
    if (t < nc) P[c0 + t] = s[t];
  }
  __syncthreads();
  if (t == 0) {
    const double W = s_acc;
    reinterpret_cast<double*>(ws)[1] = W;
    reinterpret_cast<long long*>(ws)[2] = s_jl;
    info[0] = 0; info[1] = 0; info[2] = (W > 0.0 && W <= FF_DMC_BIG) ? 0 : 1; info[3] = 0;
    atomicExch(ws, 0ull);
  }
}

__global__ void __launch_bounds__(256)
ff_dmc_resample_kernel(int64_t B, int M, double* __restrict__ w, const double* __restrict__ x, const double* __restrict__ logp,
                       const double* __restrict__ grad, const double* __restrict__ eloc, const double* __restrict__ sign,
                       const double* __restrict__ u0, uint64_t seed, uint32_t step, int* __restrict__ src, double* __restrict__ x_out,
                       double* __restrict__ logp_out, double* __restrict__ grad_out, double* __restrict__ eloc_out,
                       double* __restrict__ sign_out, const unsigned long long* __restrict__ ws) {
  const int64_t nchunks = (B + FF_DMC_CHUNK - 1) / FF_DMC_CHUNK;
  const double* const loc = reinterpret_cast<const double*>(ws + FF_DMC_HEAD);
  const double* const P = loc + B + nchunks;
  const double W = reinterpret_cast<const double*>(ws)[1];
  const int64_t jlast = reinterpret_cast<const long long*>(ws)[2];
  const bool ok = W > 0.0 && W <= FF_DMC_BIG;
  const double uv = u0 ? u0[0] : ff_uniform(seed, 1ull << 63, step, 0u);
  const double dw = W / (double)B;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < B; k += (int64_t)gridDim.x * blockDim.x) {
    int64_t j = k;
    if (ok) {
      const double tk = ((double)k + uv) * dw;
      int64_t a = 0, b = B;                           // the smallest j with tk < cum_j, or B
      while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (tk < P[mid / FF_DMC_CHUNK] + loc[mid]) b = mid; else a = mid + 1;
      }
      j = a > jlast ? jlast : a;
    }
    src[k] = (int)j;
    for (int i = 0; i < M; i++) { x_out[k * M + i] = x[j * M + i]; grad_out[k * M + i] = grad[j * M + i]; }
    logp_out[k] = logp[j]; eloc_out[k] = eloc[j]; sign_out[k] = sign[j];
    w[k] = 1.0;
  }
}

__global__ void __launch_bounds__(256)
ff_dmc_comb_stats_kernel(int64_t B, const int* __restrict__ src, int* __restrict__ info) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < B; k += (int64_t)gridDim.x * blockDim.x) {
    const int sk = src[k];
    if (k > 0 && src[k - 1] == sk) continue;
    int64_t a = k + 1, b = B;                          // the end of the run that starts here
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (src[mid] > sk) b = mid; else a = mid + 1;
    }
    atomicAdd(&info[0], 1);
    atomicMax(&info[1], (int)(a - k));
  }
}
