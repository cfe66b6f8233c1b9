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
//
// Walkers of several many-body states (BetaVMC; ff_sr_state_moments / ff_sr_state_finish).  The Fisher block of the flow's
// parameters is the pooled within-state scatter (1/B) [S_raw - sum_n o_n o_n^T / c_n], o_n and c_n the column sums and the count of
// state n.  S_raw is the SAME kernel body (STATES = true differs under `if constexpr` only): the workgroups that sum columns walker
// by walker look the baseline up by state (g_sum = sum_b O_b (e_b - mean_e[state_b])) and flush their running column sum at every
// change of state into the slot chunk + state of `pstate`.  walker_state is sorted, so along the batch both coordinates are
// monotone: the (chunk, state) segments, at most nchunks + nstates - 1 of them, have distinct slots -- O((nchunks + nstates) P)
// doubles, not nchunks nstates P.  ff_sr_state_reduce_kernel finds the walkers of state n by two binary searches in walker_state,
// hence its count (exact) and the chunks c_lo .. c_hi it touches, and adds exactly the slots c + n of those chunks in chunk order:
// a slot no segment wrote is never read.  The correction sum_n o_n o_n^T / c_n is the Gram matrix of the nstates rows o_n / sqrt(c_n):
// ff_sr_state_finish writes those rows and runs ff_sr_moments_kernel / ff_sr_reduce_kernel on them -- mirrored, exactly symmetric,
// and so is fisher = (S_raw - gram) / B.
#pragma once

#define FF_SR_CHUNK 2048     // walkers per chunk (fixed: the summation order must not depend on the launch)
#define FF_SR_KB 16          // walkers per LDS slab
#define FF_SR_PW 64          // columns per panel (four tiles)
#define FF_SR_LROW 80        // doubles per LDS row of a panel: the four rows a half wave reads start 128 bytes apart modulo the banks
#define FF_SR_PMAX (6 * FF_HMAX)
#define FF_SR_NSMAX 65536    // many-body states of ff_sr_state_moments

struct ff_sr_args {
  int64_t B, nitems;      // nitems = nchunks * npairs
  int P, npanels, npairs;
  const double* scores;
  const double* eloc;
  const double* e_mean;
  double* ptile;      // (nchunks, npairs, 4 waves, 4 tiles, 256) partial tiles in the accumulators' lane layout
  double* pvec;       // (nchunks, 2 * npanels * 64 + 1) partial o_sum | g_sum | sum(e - E)
};

struct ff_sr_state_args {      // (STATES only; e_mean of ff_sr_args is then the per-state baseline)
  const int32_t* walker_state;
  int nstates;
  double* pstate;     // (nchunks + nstates, npanels * 64) running column sums, flushed at every change of state into the slot chunk + state
};
struct ff_sr_no_states {};

static inline int64_t ff_sr_nchunks(int64_t B) { return (B + FF_SR_CHUNK - 1) / FF_SR_CHUNK; }
static inline int ff_sr_npanels(int P) { return (P + FF_SR_PW - 1) / FF_SR_PW; }
FF_HD size_t ff_sr_pvec_len(int npanels) { return (size_t)2 * npanels * FF_SR_PW + 1; }

template <bool STATES, class XA>
FF_D void ff_sr_moments_body(const ff_sr_args& A, const XA& X, double (*s_o)[FF_SR_KB][FF_SR_LROW], double* s_de, int* s_st) {
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
  double emean = 0.0;
  if constexpr (!STATES) emean = A.e_mean[0];
  ff_d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = ff_d4{0.0, 0.0, 0.0, 0.0};
  double osum = 0.0, gsum = 0.0, esum = 0.0;
  int cur = -1;      // STATES: the state osum belongs to (-1: none yet / a row without one)
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
    if constexpr (STATES) {
      if (tid < FF_SR_KB) {      // rows past the end: no state, nothing to add; a state outside [0, nstates): no slot, and NaN into g_sum
        int st = -1;
        double de = 0.0;
        if (b0 + tid < b_hi) {
          st = X.walker_state[b0 + tid];
          const bool ok = st >= 0 && st < X.nstates;
          de = ok ? A.eloc[b0 + tid] - A.e_mean[st] : __longlong_as_double(0x7ff8000000000000ll);
          if (!ok) st = -1;
        }
        s_st[tid] = st;
        s_de[tid] = de;
      }
    } else {
      if (tid < FF_SR_KB) s_de[tid] = (b0 + tid < b_hi) ? A.eloc[b0 + tid] - emean : 0.0;
    }
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
          if constexpr (STATES) {      // (wave-uniform) a change of state: the running sum goes to the slot chunk + state
            const int st = s_st[r];
            if (st != cur) {
              if (cur >= 0) X.pstate[((size_t)chunk + cur) * ((size_t)A.npanels * FF_SR_PW) + PI * FF_SR_PW + tid] = osum;
              osum = 0.0;
              cur = st;
            }
          }
          const double o = s_o[0][r][tid];
          osum += o;
          gsum = fma(o, s_de[r], gsum);
        }
      } else if (!STATES && tid == FF_SR_PW && PI == 0) {
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
      if constexpr (STATES) {
        if (cur >= 0) X.pstate[((size_t)chunk + cur) * ((size_t)A.npanels * FF_SR_PW) + PI * FF_SR_PW + tid] = osum;
      } else {
        pv[PI * FF_SR_PW + tid] = osum;
      }
      pv[(A.npanels + PI) * FF_SR_PW + tid] = gsum;
    } else if (!STATES && tid == FF_SR_PW && PI == 0) {
      pv[2 * A.npanels * FF_SR_PW] = esum;
    }
  }
}

__global__ void __launch_bounds__(256)
ff_sr_moments_kernel(ff_sr_args A) {
  __shared__ double s_o[2][FF_SR_KB][FF_SR_LROW];
  __shared__ double s_de[FF_SR_KB];
  ff_sr_moments_body<false>(A, ff_sr_no_states{}, s_o, s_de, nullptr);
}

__global__ void __launch_bounds__(256)
ff_sr_state_moments_kernel(ff_sr_args A, ff_sr_state_args X) {
  __shared__ double s_o[2][FF_SR_KB][FF_SR_LROW];
  __shared__ double s_de[FF_SR_KB];
  __shared__ int s_st[FF_SR_KB];
  ff_sr_moments_body<true>(A, X, s_o, s_de, s_st);
}

// sums = the chunks' partials added in chunk order; the product's entries i >= j, mirrored
// (STATES: S_raw as before; of the vectors only g_sum, behind the nstates rows of o_state -- ff_sr_state_reduce_kernel writes those and the counts)
template <bool STATES>
FF_D void ff_sr_reduce_body(const ff_sr_args& A, int64_t nchunks, double* __restrict__ sums, int nstates) {
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
    if (k < P && !(STATES && which == 0)) {
      double s = 0.0;
      for (int64_t c = 0; c < nchunks; c++) s += A.pvec[c * vlen + q];
      if constexpr (STATES) sums[(size_t)P * P + (size_t)nstates * P + k] = s;
      else sums[(size_t)P * P + (size_t)which * P + k] = s;
    }
  } else if (!STATES && q == 2 * (int64_t)A.npanels * FF_SR_PW) {
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; c++) s += A.pvec[c * vlen + vlen - 1];
    sums[(size_t)P * P + 2 * P] = s;
    sums[(size_t)P * P + 2 * P + 1] = (double)A.B;
  }
}

__global__ void __launch_bounds__(256)
ff_sr_reduce_kernel(ff_sr_args A, int64_t nchunks, double* __restrict__ sums) {
  ff_sr_reduce_body<false>(A, nchunks, sums, 0);
}

__global__ void __launch_bounds__(256)
ff_sr_state_sums_kernel(ff_sr_args A, int64_t nchunks, double* __restrict__ sums, int nstates) {
  ff_sr_reduce_body<true>(A, nchunks, sums, nstates);
}

// o_state[n][k] and c_state[n]: the walkers of state n are [lo, hi) by two binary searches in the sorted walker_state; its segments
// sit in the slots c + n of the chunks c_lo .. c_hi, added in chunk order
__global__ void __launch_bounds__(256)
ff_sr_state_reduce_kernel(ff_sr_args A, ff_sr_state_args X, double* __restrict__ sums) {
  const int P = A.P;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)X.nstates * P) return;
  const int n = (int)(e / P), k = (int)(e % P);
  int64_t lo = 0, hi = A.B;      // first walker with state >= n
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (X.walker_state[m] < n) lo = m + 1; else hi = m;
  }
  int64_t up = lo;               // first walker with state > n
  hi = A.B;
  while (up < hi) {
    const int64_t m = (up + hi) >> 1;
    if (X.walker_state[m] <= n) up = m + 1; else hi = m;
  }
  double s = 0.0;
  if (up > lo) {
    const size_t w = (size_t)A.npanels * FF_SR_PW;
    for (int64_t c = lo / FF_SR_CHUNK; c <= (up - 1) / FF_SR_CHUNK; c++) s += X.pstate[((size_t)c + n) * w + k];
  }
  sums[(size_t)P * P + e] = s;
  if (k == 0) sums[(size_t)P * P + (size_t)X.nstates * P + P + n] = (double)(up - lo);
}

// rows o_n / sqrt(c_n) of the within-state correction's Gram matrix (empty states: zero rows), obar_state = o_n / c_n (0 for an
// empty state); workgroup 0 also totals the counts (whole numbers below 2^53: exact in any order)
__global__ void __launch_bounds__(256)
ff_sr_state_rows_kernel(int P, int nstates, const double* __restrict__ sums, double* __restrict__ rows, double* __restrict__ obar_state,
                        double* __restrict__ total) {
  __shared__ double s_c[256];
  const double* ostate = sums + (size_t)P * P;
  const double* cstate = ostate + (size_t)nstates * P + P;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)nstates * P) {
    const double c = cstate[e / P], o = ostate[e];
    rows[e] = c > 0.0 ? o / sqrt(c) : 0.0;
    obar_state[e] = c > 0.0 ? o / c : 0.0;
  }
  if (blockIdx.x == 0) {      // (workgroup-uniform)
    double s = 0.0;
    for (int n = threadIdx.x; n < nstates; n += 256) s += cstate[n];
    s_c[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int t = 1; t < 256; t++) s += s_c[t];
      total[0] = s;
    }
  }
}

// fisher = (S_raw - gram) / B (both exactly symmetric), grad = g_sum / B; B = 0 gives NaN
__global__ void __launch_bounds__(256)
ff_sr_state_finish_kernel(int P, int nstates, const double* __restrict__ sums, const double* __restrict__ gram, const double* __restrict__ total,
                          double* __restrict__ fisher, double* __restrict__ grad) {
  const double n = total[0];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)P * P) {
    fisher[e] = (sums[e] - gram[e]) / n;
  } else if (e < (int64_t)P * P + P) {
    const int i = (int)(e - (int64_t)P * P);
    grad[i] = sums[(size_t)P * P + (size_t)nstates * P + i] / n;
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

// doubles of the partial tiles and vectors of B walkers
static size_t sr_partials_len(int64_t B, int P) {
  const int np = ff_sr_npanels(P);
  const size_t per_chunk = (size_t)(np * (np + 1) / 2) * 4096 + ff_sr_pvec_len(np);
  return (size_t)ff_sr_nchunks(B) * per_chunk;
}

size_t ff_sr_moments_workspace_bytes(int64_t B, int P) {
  if (B < 0 || P < 1 || P > FF_SR_PMAX) return 0;
  return sizeof(double) * (sr_partials_len(B, P) + 1);
}

static ff_sr_args sr_args(int64_t B, int P, const double* scores, const double* eloc, const double* e_mean, void* workspace) {
  ff_sr_args a = {};
  a.B = B; a.P = P; a.npanels = ff_sr_npanels(P); a.npairs = a.npanels * (a.npanels + 1) / 2;
  a.scores = scores; a.eloc = eloc; a.e_mean = e_mean;
  const int64_t nchunks = ff_sr_nchunks(B);
  a.ptile = (double*)workspace;
  a.pvec = a.ptile + (size_t)nchunks * a.npairs * 4096;
  a.nitems = nchunks * a.npairs;
  return a;
}

// the two launches of ff_sr_moments (B > 0)
static int sr_moments_launch(void* stream, const ff_sr_args& a, double* sums) {
  FF_LAUNCH(ff_sr_moments_kernel, (unsigned)((a.nitems + 7) / 8 * 8), 256, stream, a);
  FF_LAUNCH_CHECK();
  const int64_t nred = (int64_t)a.npairs * 4096 + 2 * (int64_t)a.npanels * FF_SR_PW + 1;
  FF_LAUNCH(ff_sr_reduce_kernel, (unsigned)((nred + 255) / 256), 256, stream, a, ff_sr_nchunks(a.B), sums);
  FF_LAUNCH_CHECK();
  return FF_OK;
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
  return sr_moments_launch(stream, sr_args(B, P, scores, eloc, e_mean, workspace), sums);
}

int ff_sr_finish(void* stream, int P, const double* sums, double* fisher, double* obar, double* grad) {
  if (const int st = sr_check(0, P)) return st;
  FF_CHECK(sums && fisher && obar && grad, FF_EINVAL, "ff_sr: null pointer");
  const int64_t n = (int64_t)P * P + P;
  FF_LAUNCH(ff_sr_finish_kernel, (unsigned)((n + 255) / 256), 256, stream, P, sums, fisher, obar, grad);
  FF_LAUNCH_CHECK();
  return FF_OK;
}

// ---- walkers of several many-body states
static int sr_state_check(int64_t B, int P, int nstates) {
  if (const int st = sr_check(B, P)) return st;
  if (nstates < 1 || nstates > FF_SR_NSMAX) return ff_refuse(FF_EUNSUPPORTED, "ff_sr", "1 <= nstates <= 65536 states");
  return FF_OK;
}

static size_t sr_pstate_len(int64_t B, int P, int nstates) {
  return ((size_t)ff_sr_nchunks(B) + nstates) * ff_sr_npanels(P) * FF_SR_PW;
}
// the finish: rows (nstates, P) | gram sums (P*P + 2P + 2) | total count | partials of nstates rows
static size_t sr_state_finish_len(int P, int nstates) {
  return (size_t)nstates * P + ((size_t)P * P + 2 * (size_t)P + 2) + 1 + sr_partials_len(nstates, P);
}

size_t ff_sr_state_moments_workspace_bytes(int64_t B, int P, int nstates) {
  if (B < 0 || P < 1 || P > FF_SR_PMAX || nstates < 1 || nstates > FF_SR_NSMAX) return 0;
  const size_t moments = sr_partials_len(B, P) + sr_pstate_len(B, P, nstates), finish = sr_state_finish_len(P, nstates);
  return sizeof(double) * ((moments > finish ? moments : finish) + 1);
}

int ff_sr_state_moments(void* stream, int64_t B, int P, int nstates, const double* scores, const double* eloc, const int32_t* walker_state,
                        const double* mean_e, double* sums, void* workspace) {
  if (const int st = sr_state_check(B, P, nstates)) return st;
  FF_CHECK(sums && (B == 0 || (scores && eloc && walker_state && mean_e && workspace)), FF_EINVAL, "ff_sr: null pointer");
  const size_t nsums = (size_t)P * P + (size_t)nstates * P + P + nstates;
  if (B == 0) {
    if (hipMemsetAsync(sums, 0, sizeof(double) * nsums, (hipStream_t)stream) != hipSuccess) return FF_ELAUNCH;
    return FF_OK;
  }
  const ff_sr_args a = sr_args(B, P, scores, eloc, mean_e, workspace);
  ff_sr_state_args x = {};
  x.walker_state = walker_state; x.nstates = nstates;
  x.pstate = (double*)workspace + sr_partials_len(B, P);
  FF_LAUNCH(ff_sr_state_moments_kernel, (unsigned)((a.nitems + 7) / 8 * 8), 256, stream, a, x);
  FF_LAUNCH_CHECK();
  const int64_t nred = (int64_t)a.npairs * 4096 + 2 * (int64_t)a.npanels * FF_SR_PW;
  FF_LAUNCH(ff_sr_state_sums_kernel, (unsigned)((nred + 255) / 256), 256, stream, a, ff_sr_nchunks(B), sums, nstates);
  FF_LAUNCH_CHECK();
  FF_LAUNCH(ff_sr_state_reduce_kernel, (unsigned)(((int64_t)nstates * P + 255) / 256), 256, stream, a, x, sums);
  FF_LAUNCH_CHECK();
  return FF_OK;
}

int ff_sr_state_finish(void* stream, int P, int nstates, const double* sums, double* fisher, double* obar_state, double* grad, void* workspace) {
  if (const int st = sr_state_check(0, P, nstates)) return st;
  FF_CHECK(sums && fisher && obar_state && grad && workspace, FF_EINVAL, "ff_sr: null pointer");
  double* rows = (double*)workspace;
  double* gram = rows + (size_t)nstates * P;
  double* total = gram + ((size_t)P * P + 2 * (size_t)P + 2);
  const double* cstate = sums + (size_t)P * P + (size_t)nstates * P + P;
  FF_LAUNCH(ff_sr_state_rows_kernel, (unsigned)(((int64_t)nstates * P + 255) / 256), 256, stream, P, nstates, sums, rows, obar_state, total);
  FF_LAUNCH_CHECK();
  // the Gram matrix of the rows by the moments pass itself (its vectors are by-products: the counts stand in for the energies)
  if (const int st = sr_moments_launch(stream, sr_args(nstates, P, rows, cstate, cstate, total + 1), gram)) return st;
  const int64_t n = (int64_t)P * P + P;
  FF_LAUNCH(ff_sr_state_finish_kernel, (unsigned)((n + 255) / 256), 256, stream, P, nstates, sums, gram, total, fisher, grad);
  FF_LAUNCH_CHECK();
  return FF_OK;
}

}  // extern "C"
