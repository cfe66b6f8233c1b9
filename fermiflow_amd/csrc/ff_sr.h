// ff_sr.h -- moments of the per-walker log-derivatives O (B, P) for stochastic reconfiguration (included by ff_cnf_adj.hip):
//     S_raw = sum_b O_b O_b^T    o_sum = sum_b O_b    g_sum = sum_b O_b (e_b - E)    sum_b (e_b - E)    B
// as RAW sums (ff_sr_moments; ranks add them with one all-reduce), and from the summed numbers (ff_sr_finish)
//     fisher = S_raw / B - obar obar^T    obar = o_sum / B    grad = g_sum / B - obar * sum(e - E) / B.
//
// S_raw runs on v_mfma_f64_16x16x4_f64 (ff_mfma16, ff_common.h): P is padded to 16-column tiles by zero operands, and for the tile
// (I, J) and four walkers b0 .. b0 + 3 both operands have the SAME lane layout -- lane l supplies A[l % 16][l / 16] = O[b0 + l / 16][16 I + l % 16]
// and B[l / 16][l % 16] = O[b0 + l / 16][16 J + l % 16] -- so one LDS read per tile and four walkers serves either side.  Register
// v of lane l holds the result's row 4 v + l / 16, column l % 16 (tools/probes/wide_probe.hip).
//
// Work split.  Tiles are grouped into panels of four (64 columns); a workgroup of four waves takes ONE chunk of FF_SR_CHUNK walkers
// and ONE panel pair (PI >= PJ: the lower triangle), wave w the tile row 4 PI + w against the four tile columns of PJ: four
// accumulators, 16 registers.  The chunk's 128 columns pass through LDS in slabs of FF_SR_KB walkers: per four walkers a wave reads
// five operands from LDS for four matrix instructions (256 cycles).  A chunk's rows (FF_SR_CHUNK x 8 P bytes: 4.9 MB at P = 300) are
// read once per panel pair.  Consecutive workgroup ids are dealt round-robin over the eight XCDs, each with an L2 of its own, so the
// kernel renumbers them: the workgroups of ONE XCD take consecutive (chunk, pair) items, and a chunk's panel pairs re-read it
// through the same L2 (4 MB: not the whole chunk at P = 300, but its pairs walk the slabs side by side).  Not measured.
// The vectors ride along: the workgroups (PI, 0) also sum their 64 columns of O and of O (e - E), walker by walker, from the slab.
//
// Determinism.  The chunks are FF_SR_CHUNK walkers whatever the grid; a workgroup adds its walkers in walker order; every
// workgroup writes its partial tiles to the workspace and ff_sr_reduce_kernel adds the chunks' partials in chunk order.  No
// floating-point atomics: the sums are bit-identical from run to run.  Only entries i >= j are taken from the product and
// mirrored, so S_raw -- and fisher, whose correction obar_i obar_j is one rounded product either way -- is exactly symmetric.
#pragma once

#define FF_SR_CHUNK 2048     // walkers per chunk (fixed: the summation order must not depend on the launch)
#define FF_SR_KB 16          // walkers per LDS slab
#define FF_SR_PW 64          // columns per panel (four tiles)
#define FF_SR_LROW 80        // doubles per LDS row of a panel: the four rows a half wave reads start 128 bytes apart modulo the banks
#define FF_SR_PMAX (6 * FF_HMAX)

struct ff_sr_args {
  int64_t B, nitems;      // nitems = nchunks * npairs
  int P, npanels, npairs;
  const double* scores;
  const double* eloc;
  const double* e_mean;
  double* ptile;      // (nchunks, npairs, 4 waves, 4 tiles, 256) partial tiles in the accumulators' lane layout
  double* pvec;       // (nchunks, 2 * npanels * 64 + 1) partial o_sum | g_sum | sum(e - E)
};

static inline int64_t ff_sr_nchunks(int64_t B) { return (B + FF_SR_CHUNK - 1) / FF_SR_CHUNK; }
static inline int ff_sr_npanels(int P) { return (P + FF_SR_PW - 1) / FF_SR_PW; }
FF_HD size_t ff_sr_pvec_len(int npanels) { return (size_t)2 * npanels * FF_SR_PW + 1; }

__global__ void __launch_bounds__(256)
ff_sr_moments_kernel(ff_sr_args A) {
  __shared__ double s_o[2][FF_SR_KB][FF_SR_LROW];
  __shared__ double s_de[FF_SR_KB];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  // item of this workgroup: XCD x = blockIdx % 8 takes the items x * (grid / 8) ...; the grid is a multiple of 8, the tail is idle
  const int64_t item = (int64_t)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
  if (item >= A.nitems) return;
  const int64_t chunk = item / A.npairs;
  const int pair = (int)(item - chunk * A.npairs);
  int pr = pair, PI = 0;
  while (pr > PI) { pr -= PI + 1; PI++; }      // pair index -> (PI, PJ), PJ <= PI
  const int PJ = pr;
  const bool diag = PI == PJ, vecs = PJ == 0;
  const int64_t b_lo = chunk * FF_SR_CHUNK, b_hi = b_lo + FF_SR_CHUNK < A.B ? b_lo + FF_SR_CHUNK : A.B;
  const double emean = A.e_mean[0];
  ff_d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = ff_d4{0.0, 0.0, 0.0, 0.0};
  double osum = 0.0, gsum = 0.0, esum = 0.0;
  const int lc = tid & 63, lr0 = tid >> 6;      // slab loads: thread -> column lc of the rows lr0, lr0 + 4, ...
  const int colI = PI * FF_SR_PW + lc, colJ = PJ * FF_SR_PW + lc;
  for (int64_t b0 = b_lo; b0 < b_hi; b0 += FF_SR_KB) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FF_SR_KB / 4; q++) {
      const int r = lr0 + 4 * q;
      const int64_t b = b0 + r;
      const bool inb = b < b_hi;
      s_o[0][r][lc] = (inb && colI < A.P) ? A.scores[b * A.P + colI] : 0.0;
      if (!diag) s_o[1][r][lc] = (inb && colJ < A.P) ? A.scores[b * A.P + colJ] : 0.0;
    }
    if (tid < FF_SR_KB) s_de[tid] = (b0 + tid < b_hi) ? A.eloc[b0 + tid] - emean : 0.0;
    __syncthreads();
    const double (*oI)[FF_SR_LROW] = s_o[0];
    const double (*oJ)[FF_SR_LROW] = s_o[diag ? 0 : 1];
#pragma unroll
    for (int kk = 0; kk < FF_SR_KB; kk += 4) {
      const int r = kk + (lane >> 4), c = lane & 15;
      const double a = oI[r][16 * wv + c];
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = ff_mfma16(a, oJ[r][16 * t + c], acc[t]);
    }
    if (vecs) {      // (workgroup-uniform) the first wave: column sums, walker by walker; one of its lanes' twin in wave 1: sum(e - E)
      if (tid < FF_SR_PW) {
#pragma unroll
        for (int r = 0; r < FF_SR_KB; r++) {
          const double o = s_o[0][r][tid];
          osum += o;
          gsum = fma(o, s_de[r], gsum);
        }
      } else if (tid == FF_SR_PW && PI == 0) {
#pragma unroll
        for (int r = 0; r < FF_SR_KB; r++) esum += s_de[r];
      }
    }
  }
  double* out = A.ptile + (((size_t)chunk * A.npairs + pair) * 4 + wv) * 4 * 256;
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int v = 0; v < 4; v++) out[t * 256 + v * 64 + lane] = acc[t][v];
  if (vecs) {
    double* pv = A.pvec + (size_t)chunk * ff_sr_pvec_len(A.npanels);
    if (tid < FF_SR_PW) {
      pv[PI * FF_SR_PW + tid] = osum;
      pv[(A.npanels + PI) * FF_SR_PW + tid] = gsum;
    } else if (tid == FF_SR_PW && PI == 0) {
      pv[2 * A.npanels * FF_SR_PW] = esum;
    }
  }
}

// sums = the chunks' partials added in chunk order; the product's entries i >= j, mirrored
__global__ void __launch_bounds__(256)
ff_sr_reduce_kernel(ff_sr_args A, int64_t nchunks, double* __restrict__ sums) {
  const int P = A.P;
  const int64_t ntile = (int64_t)A.npairs * 4096;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ntile) {
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; c++) s += A.ptile[c * ntile + e];
    int pr = (int)(e / 4096), PI = 0;
    while (pr > PI) { pr -= PI + 1; PI++; }
    const int rem = (int)(e % 4096), wv = rem / 1024, t = (rem / 256) % 4, v = (rem / 64) % 4, l = rem % 64;
    const int i = PI * FF_SR_PW + 16 * wv + 4 * v + (l >> 4), j = pr * FF_SR_PW + 16 * t + (l & 15);
    if (i < P && j <= i) {
      sums[(size_t)i * P + j] = s;
      sums[(size_t)j * P + i] = s;
    }
    return;
  }
  const int64_t q = e - ntile;
  const size_t vlen = ff_sr_pvec_len(A.npanels);
  if (q < 2 * (int64_t)A.npanels * FF_SR_PW) {
    const int which = (int)(q / (A.npanels * FF_SR_PW)), k = (int)(q % (A.npanels * FF_SR_PW));
    if (k < P) {
      double s = 0.0;
      for (int64_t c = 0; c < nchunks; c++) s += A.pvec[c * vlen + q];
      sums[(size_t)P * P + (size_t)which * P + k] = s;
    }
  } else if (q == 2 * (int64_t)A.npanels * FF_SR_PW) {
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; c++) s += A.pvec[c * vlen + vlen - 1];
    sums[(size_t)P * P + 2 * P] = s;
    sums[(size_t)P * P + 2 * P + 1] = (double)A.B;
  }
}

__global__ void __launch_bounds__(256)
ff_sr_finish_kernel(int P, const double* __restrict__ sums, double* __restrict__ fisher, double* __restrict__ obar, double* __restrict__ grad) {
  const double* osum = sums + (size_t)P * P;
  const double* gsum = osum + P;
  const double n = osum[2 * P + 1], de = osum[2 * P] / n;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)P * P) {
    const int i = (int)(e / P), j = (int)(e % P);
    const double oi = osum[i] / n, oj = osum[j] / n, s = sums[e] / n, oo = oi * oj;      // (oo rounded on its own: the same number for (i, j) and (j, i))
    fisher[e] = s - oo;
  } else if (e < (int64_t)P * P + P) {
    const int i = (int)(e - (int64_t)P * P);
    const double oi = osum[i] / n, g = gsum[i] / n, od = oi * de;
    obar[i] = oi;
    grad[i] = g - od;
  }
}

extern "C" {

static int sr_check(int64_t B, int P) {
  if (B < 0) return ff_refuse(FF_EINVAL, "ff_sr", "negative batch size");
  if (P < 1 || P > FF_SR_PMAX) return ff_refuse(FF_EUNSUPPORTED, "ff_sr", "1 <= P <= 1536 parameters");
  return FF_OK;
}

size_t ff_sr_moments_workspace_bytes(int64_t B, int P) {
  if (B < 0 || P < 1 || P > FF_SR_PMAX) return 0;
  const int np = ff_sr_npanels(P);
  const size_t per_chunk = (size_t)(np * (np + 1) / 2) * 4096 + ff_sr_pvec_len(np);
  return sizeof(double) * ((size_t)ff_sr_nchunks(B) * per_chunk + 1);
}

int ff_sr_moments(void* stream, int64_t B, int P, const double* scores, const double* eloc, const double* e_mean, double* sums,
                  void* workspace) {
  if (const int st = sr_check(B, P)) return st;
  FF_CHECK(sums && (B == 0 || (scores && eloc && e_mean && workspace)), FF_EINVAL, "ff_sr: null pointer");
  const size_t nsums = (size_t)P * P + 2 * (size_t)P + 2;
  if (B == 0) {      // (all sums zero, the count among them)
    if (hipMemsetAsync(sums, 0, sizeof(double) * nsums, (hipStream_t)stream) != hipSuccess) return FF_ELAUNCH;
    return FF_OK;
  }
  ff_sr_args a = {};
  a.B = B; a.P = P; a.npanels = ff_sr_npanels(P); a.npairs = a.npanels * (a.npanels + 1) / 2;
  a.scores = scores; a.eloc = eloc; a.e_mean = e_mean;
  const int64_t nchunks = ff_sr_nchunks(B);
  a.ptile = (double*)workspace;
  a.pvec = a.ptile + (size_t)nchunks * a.npairs * 4096;
  a.nitems = nchunks * a.npairs;
  FF_LAUNCH(ff_sr_moments_kernel, (unsigned)((a.nitems + 7) / 8 * 8), 256, stream, a);
  FF_LAUNCH_CHECK();
  const int64_t nred = (int64_t)a.npairs * 4096 + 2 * (int64_t)a.npanels * FF_SR_PW + 1;
  FF_LAUNCH(ff_sr_reduce_kernel, (unsigned)((nred + 255) / 256), 256, stream, a, nchunks, sums);
  FF_LAUNCH_CHECK();
  return FF_OK;
}

int ff_sr_finish(void* stream, int P, const double* sums, double* fisher, double* obar, double* grad) {
  if (const int st = sr_check(0, P)) return st;
  FF_CHECK(sums && fisher && obar && grad, FF_EINVAL, "ff_sr: null pointer");
  const int64_t n = (int64_t)P * P + P;
  FF_LAUNCH(ff_sr_finish_kernel, (unsigned)((n + 255) / 256), 256, stream, P, sums, fisher, obar, grad);
  FF_LAUNCH_CHECK();
  return FF_OK;
}

}  // extern "C"
