// ff_obdm.h -- the one-body reduced density matrix of the physical walkers in the harmonic-oscillator basis, accumulated on the
// device (ff_obdm_accumulate), and the sign of the Slater determinants its wave-function ratios need (ff_slater_sign).  Contract,
// accumulator layout and the determinism rules: include/fermiflow_obdm.h.
//
// ff_slater_sign_kernel<NS>, NS = max(nup, ndn): ONE LANE PER WALKER, as ff_slater_logabsdet_fwd.  A species of ns < NS particles is
// the leading block of an NS x NS matrix whose other rows are rows of the identity: the same determinant, and the elimination of the
// block is the same arithmetic (a padding row holds zeros where the pivot search looks and is never chosen), so one instantiation per
// NS serves every (nup, ndn).  Both species run through the same code (#pragma unroll 1).  The rows carry the polynomials
// h_nx(x) h_ny(y) only: the Gaussian of a row is a positive factor that changes no sign and would underflow to a zero row in the tail.
// The eight Hermite values of a coordinate come from one pass of the recurrence over literal coefficients; an orbital picks its two by
// three selects each (the degrees are data here: the tables of the excited states).  The matrix stays in registers (ff_lu_absdet_reg);
// 64 lanes per workgroup so that a large NS has the whole register file of a SIMD: no scratch up to NS = 11; NS = 12 (144 doubles and the
// row exchanges' temporaries) spills 156 bytes per lane, outside any loop.
//
// ff_obdm_kernel: a workgroup of 256 threads takes CHUNKS of FF_OBDM_CHUNK consecutive walkers (chunk = blockIdx.x, + gridDim.x, ...).
// A chunk is walked in slabs of `slabw` walkers (128, 64 or 32 by the size of the basis, so that a slab's vectors fit 44 KB of LDS):
//   form    thread t < 2 slabw takes (species t / slabw, walker t % slabw) and forms A[nb] and C[nb] into LDS: the orbital values of a
//           point are 8 + 8 Hermite values from one pass of the recurrence and nb products with COMPILE-TIME degrees (ff_obdm_shells;
//           no coefficient table, no select, no private array indexed at run time).  The row stride 2 nb + 1 is odd: the lanes' stores
//           fall on different banks.
//   update  the threads own the 2 nb^2 matrix entries (entry e = t + 256 k, k < FF_OBDM_EPT = 11 at nb = 36, one at nb <= 10: a
//           compile-time bound, the partial sums stay in registers) and run over the slab's walkers in order: one fused multiply-add
//           per walker and entry, A[a] a broadcast read and C[c] consecutive words of a row.
// After its last slab the chunk's partial matrix goes to the workspace.  The workgroup that draws the last ticket sums the chunks in
// chunk order into LDS, symmetrises and adds T and T o T to the accumulator.  invalid[] is added with integer atomics.
#pragma once
#include "ff_common.h"
#include "ff_slater.h"
#include "../../include/fermiflow_obdm.h"

#define FF_OBDM_THREADS 256
#define FF_OBDM_EPT 11                   // matrix entries per thread: ceil(2 x 36 x 36 / 256)
#define FF_OBDM_GRID_PER_CU 4            // grid cap: workgroups per compute unit (three slabs of 44 KB fit the CU's 160 KB)
#define FF_OBDM_NB(nshells) ((nshells) * ((nshells) + 1) / 2)
#define FF_OBDM_BIG 1.7976931348623157e308

// h[m] = h_m(x), m = 0 .. 7: the recurrence over literal coefficients (the numbers of ff_herm_lit)
FF_D void ff_obdm_herm8(double x, double (&h)[8]) {
  constexpr double RA[7] = {1.4142135623730951, 1.0, 0.81649658092772603, 0.70710678118654752, 0.63245553203367588,
                            0.57735026918962576, 0.53452248382484879};
  constexpr double RB[7] = {0.0, 0.70710678118654752, 0.81649658092772603, 0.86602540378443865, 0.89442719099991588,
                            0.91287092917527686, 0.92582009977255146};
  h[0] = 1.0;
  h[1] = RA[0] * x;
#pragma unroll
  for (int m = 1; m < 7; m++) h[m + 1] = fma(RA[m] * x, h[m], -RB[m] * h[m - 1]);
}
FF_D double ff_obdm_sel8(const double (&h)[8], int n) {
  const bool b0 = n & 1, b1 = n & 2, b2 = n & 4;
  const double a0 = b0 ? h[1] : h[0], a1 = b0 ? h[3] : h[2], a2 = b0 ? h[5] : h[4], a3 = b0 ? h[7] : h[6];
  const double c0 = b1 ? a1 : a0, c1 = b1 ? a3 : a2;
  return b2 ? c1 : c0;
}
// orbital index k < 36 -> nx | ny << 3, branch-free (ff_orb_decode's shell search as seven compares)
FF_D int ff_obdm_degrees(int k) {
  const int sh = (k >= 1) + (k >= 3) + (k >= 6) + (k >= 10) + (k >= 15) + (k >= 21) + (k >= 28);
  const int nx = k - sh * (sh + 1) / 2;
  return nx | ((sh - nx) << 3);
}

template <int NS>
__global__ void __launch_bounds__(FF_WAVE)
ff_slater_sign_kernel(int64_t B, int nup, int ndn, const int* __restrict__ tab_up, const int* __restrict__ tab_dn,
                      const int* __restrict__ wstate, const double* __restrict__ z, double* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = nup + ndn, st = wstate ? wstate[b] : 0;
  const double* __restrict__ row = z + b * (2 * n);
  double sg = 1.0;
  bool fin = true;
#pragma unroll 1
  for (int sp = 0; sp < 2; sp++) {
    const int ns = sp ? ndn : nup, off = sp ? nup : 0;
    if (!ns) continue;
    const int* __restrict__ orb = (sp ? tab_dn : tab_up) + st * ns;
    int deg[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) deg[j] = ff_obdm_degrees(j < ns ? orb[j] : 0);
    double D[NS][NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
      const bool act = i < ns;
      const double xi = act ? row[2 * (off + i)] : 0.0, yi = act ? row[2 * (off + i) + 1] : 0.0;
      fin = fin && fabs(xi) <= FF_OBDM_BIG && fabs(yi) <= FF_OBDM_BIG;
      double hx[8], hy[8];
      ff_obdm_herm8(xi, hx);
      ff_obdm_herm8(yi, hy);
#pragma unroll
      for (int j = 0; j < NS; j++) {
        const double v = ff_obdm_sel8(hx, deg[j] & 7) * ff_obdm_sel8(hy, deg[j] >> 3);
        D[i][j] = (act && j < ns) ? v : (i == j ? 1.0 : 0.0);
      }
    }
    double s;
    ff_lu_absdet_reg<NS>(D, nullptr, &s);
    sg *= s;
  }
  out[b] = fin ? (sg == 0.0 ? 0.0 : sg) : __longlong_as_double(0x7ff8000000000000ll);      // (no -0)
}

// dst[J] = f h_nx(J) h_ny(J)  (ADD: dst[J] += ...) for the orbitals J of the shells below `nshells` (uniform); every index is static
template <int SH, bool ADD, class Dst>
FF_D void ff_obdm_shells(const double (&hx)[8], const double (&hy)[8], double f, int nshells, Dst& dst) {
  if constexpr (SH < FF_OBDM_MAX_SHELLS) {
    if (SH < nshells) {
#pragma unroll
      for (int nx = 0; nx <= SH; nx++) {
        const double v = f * (hx[nx] * hy[SH - nx]);
        if constexpr (ADD) dst[SH * (SH + 1) / 2 + nx] += v;
        else dst[SH * (SH + 1) / 2 + nx] = v;
      }
      ff_obdm_shells<SH + 1, ADD>(hx, hy, f, nshells, dst);
    }
  }
}

// G(x, y) = pi^-1/2 exp(-(x x + y y) / 2) and the polynomials' argument: the point itself where `ok` and G > 0, the origin otherwise
// (phi = 0 there by the header's rule: the factor is 0 and the polynomials must stay finite)
FF_D double ff_obdm_gauss(bool ok, double x, double y, double& r2, bool& use) {
  r2 = x * x + y * y;
  const double gs = FF_PI_SQRT_INV * exp(-0.5 * r2);
  use = ok && gs > 0.0;
  return gs;
}

// A[nb] | C[nb] of walker b and species sp -> out (LDS)
FF_D void ff_obdm_form(int64_t b, int sp, int nup, int n, const double* __restrict__ x, const double* __restrict__ rp,
                       const double* __restrict__ logp, const double* __restrict__ sign, const double* __restrict__ lpm,
                       const double* __restrict__ sgm, double two_s2, double two_pi_s2, int nshells, int nb, double* out,
                       unsigned long long* __restrict__ invalid) {
  const int ns = sp ? n - nup : nup, off = sp ? nup : 0;
  const double rx = rp[(b * 2 + sp) * 2], ry = rp[(b * 2 + sp) * 2 + 1];
  const bool okr = ns > 0 && fabs(rx) <= FF_OBDM_BIG && fabs(ry) <= FF_OBDM_BIG;
  double hx[8], hy[8];
  {
    double r2;
    bool use;
    const double gs = ff_obdm_gauss(okr, rx, ry, r2, use);
    const double g = exp(-r2 / two_s2) / two_pi_s2;
    ff_obdm_herm8(use ? rx : 0.0, hx);
    ff_obdm_herm8(use ? ry : 0.0, hy);
    double* C = out + nb;
    ff_obdm_shells<0, false>(hx, hy, use ? gs / g : 0.0, nshells, C);
  }
  double A[FF_MAX_ORB];
#pragma unroll
  for (int j = 0; j < FF_MAX_ORB; j++) A[j] = 0.0;
  const double lp = logp[b], sg = sign[b];
  unsigned bad = 0u;
  for (int i = 0; i < ns; i++) {
    const int64_t p = b * n + off + i;
    const double xi = x[2 * p], yi = x[2 * p + 1];
    const double q = (sg * sgm[p]) * exp(0.5 * (lpm[p] - lp));
    const bool ok = okr && fabs(xi) <= FF_OBDM_BIG && fabs(yi) <= FF_OBDM_BIG && fabs(q) <= FF_OBDM_BIG;
    bad += ok ? 0u : 1u;
    double r2;
    bool use;
    const double gs = ff_obdm_gauss(ok, xi, yi, r2, use);
    ff_obdm_herm8(use ? xi : 0.0, hx);
    ff_obdm_herm8(use ? yi : 0.0, hy);
    ff_obdm_shells<0, true>(hx, hy, use ? gs * q : 0.0, nshells, A);
  }
#pragma unroll
  for (int j = 0; j < FF_MAX_ORB; j++)
    if (j < nb) out[j] = A[j];
  if (bad) atomicAdd(&invalid[sp], (unsigned long long)bad);
}

// dynamic LDS: max(2 slabw (2 nb + 1), 2 nb nb) doubles; slabw = 1 << lgslab
__global__ void __launch_bounds__(FF_OBDM_THREADS)
ff_obdm_kernel(int64_t B, int nup, int n, const double* __restrict__ x, const double* __restrict__ rp, const double* __restrict__ logp,
               const double* __restrict__ sign, const double* __restrict__ lpm, const double* __restrict__ sgm, double two_s2,
               double two_pi_s2, int nshells, int lgslab, unsigned long long* __restrict__ acc, double* __restrict__ ws) {
  FF_DYN_LDS(lds);
  __shared__ unsigned s_last;
  const int t = threadIdx.x;
  const int nb = FF_OBDM_NB(nshells), nb2 = nb * nb, E = 2 * nb2, stride = 2 * nb + 1, slabw = 1 << lgslab;
  int offA[FF_OBDM_EPT], offC[FF_OBDM_EPT];
#pragma unroll
  for (int k = 0; k < FF_OBDM_EPT; k++) {
    const int e = t + k * FF_OBDM_THREADS, s = e >= nb2 ? 1 : 0, rem = e - s * nb2, a = rem / nb, c = rem - a * nb;
    offA[k] = e < E ? s * slabw * stride + a : 0;
    offC[k] = e < E ? s * slabw * stride + nb + c : 0;
  }
  const int64_t nchunks = (B + FF_OBDM_CHUNK - 1) / FF_OBDM_CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t b0 = ch * FF_OBDM_CHUNK;
    const int cn = (int)(B - b0 < FF_OBDM_CHUNK ? B - b0 : FF_OBDM_CHUNK);
    double m[FF_OBDM_EPT];
#pragma unroll
    for (int k = 0; k < FF_OBDM_EPT; k++) m[k] = 0.0;
    for (int w0 = 0; w0 < cn; w0 += slabw) {
      const int nw = cn - w0 < slabw ? cn - w0 : slabw;
      __syncthreads();                                  // (the previous slab has been read)
      if (t < 2 * slabw) {
        const int sp = t >> lgslab, w = t & (slabw - 1);
        if (w < nw)
          ff_obdm_form(b0 + w0 + w, sp, nup, n, x, rp, logp, sign, lpm, sgm, two_s2, two_pi_s2, nshells, nb,
                       lds + (sp * slabw + w) * stride, acc + 2);
      }
      __syncthreads();
      for (int w = 0; w < nw; w++) {
        const double* row = lds + w * stride;
#pragma unroll
        for (int k = 0; k < FF_OBDM_EPT; k++)
          if (t + k * FF_OBDM_THREADS < E) m[k] = fma(row[offA[k]], row[offC[k]], m[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < FF_OBDM_EPT; k++)
      if (t + k * FF_OBDM_THREADS < E) ws[ch * E + t + k * FF_OBDM_THREADS] = m[k];
  }
  unsigned long long* const ticket = acc + 4;
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(ticket, 1ull) == (unsigned long long)(gridDim.x - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // the last workgroup: the chunks in chunk order, then T = (M + M^T) / 2.  sum, sumsq, calls and walkers are touched here only.
  for (int e = t; e < E; e += FF_OBDM_THREADS) {
    double s = 0.0;
    for (int64_t ch = 0; ch < nchunks; ch++) s += ws[ch * E + e];
    lds[e] = s;
  }
  __syncthreads();
  double* const sum = reinterpret_cast<double*>(acc + FF_OBDM_HEAD), * const sumsq = sum + E;
  for (int e = t; e < E; e += FF_OBDM_THREADS) {
    const int s = e >= nb2 ? 1 : 0, rem = e - s * nb2, a = rem / nb, c = rem - a * nb;
    const double T = 0.5 * (lds[e] + lds[s * nb2 + c * nb + a]);
    sum[e] += T;
    sumsq[e] += T * T;
  }
  if (t == 0) {
    acc[0] += 1ull;
    acc[1] += (unsigned long long)B;
    atomicExch(ticket, 0ull);
  }
}
