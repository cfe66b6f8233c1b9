// ff_mcmc.h -- the register-resident Metropolis samplers (FreeFermion.sample, src/base_dist.py:58-71) for the compile-time shapes
// of mcmc_dispatch (ff_walkers.hip); every other shape and d = 3 run sixteen lanes per determinant (ff_mcmc_rows_kernel, ff_ho3d.hip).
//
// A walker's coordinates and log-probability stay in VGPRs for all `steps` proposals: per walker-step the only HBM traffic is the
// proposal noise (parity mode) or nothing at all (Philox mode).  The chain is stated ONCE, in two drivers:
//   ff_mc_logp_chain   u < exp(log p' - log p), the reference's arithmetic operation for operation; noise-fed (g0, g, u from HBM, the
//                      next step's row requested one step ahead) or Philox-fed with a per-step draw
//   ff_mc_ratio_chain  Philox-fed, the same decision taken on the determinants of the polynomial parts of the orbitals
// and three LAYOUTS say who holds which coordinates and how log p is formed from them:
//   ff_mc_one_lane     one lane per walker                                          ff_mcmc_kernel<NU, ND, NOISE>
//   ff_mc_spin_lanes   two lanes per walker, one per spin species (NU = ND = NS)    ff_mcmc_spin_kernel<NS, true>, ff_mcmc_spin_philox_kernel<NS, GROUND>
//   ff_mc_pair_lanes   two lanes per walker splitting the particles of ONE species  ff_mcmc_pair_kernel<NS, NOISE, GROUND>
// A layout provides  MS (coordinates per lane), M (per walker), w (ff_mc_head), load(row, dst), store(row, x), logprob(xs) and, for the
// Philox-fed chains, draw(step, z, u); for the ratio chain also r2sum(xs) and polydet2(xs).  Everything is inlined and statically
// indexed: nothing leaves the registers.  Same noise stream, same walkers, bit for bit, from every kernel of a shape.
#pragma once
#include "ff_common.h"
#include "ff_slater.h"
#include "ff_rng.h"

// x + tau*g exactly as torch computes it (two roundings): hipcc's default -ffp-contract=fast would fuse
// the pair into one FMA and the walkers would no longer be bit-identical to the reference's.
// the empty asm makes the product opaque, so the backend cannot contract mul+add into v_fma_f64
FF_D double ff_mul_rn(double a, double b) { double r = a * b; FF_OPAQUE(r); return r; }
FF_D double ff_add_rn(double a, double b) { double r = a + b; FF_OPAQUE(r); return r; }
template <int N>
FF_D void ff_propose(const double* x, double tau, const double* z, double* nx) {
#pragma unroll
  for (int i = 0; i < N; i++) nx[i] = ff_add_rn(x[i], ff_mul_rn(tau, z[i]));
}

// p = exp(new_logp - logp) with torch's edge semantics: NaN stays NaN (rejects: a NaN walker, or -inf - -inf when a singular
// walker proposes another singular one), -inf gives exactly 0 (rejects), +inf (a walker with log p = -inf, e.g. every particle
// at the origin, proposing a regular one) accepts.  The clamped exponential gives e^708 for dlp >= 708, which every u < 1
// accepts, and 0 below -708, where torch's p is a denormal that only u == 0 exactly (a 2^-53 event) would accept.
FF_D double ff_accept_prob(double dlp) { return !(dlp == dlp) ? dlp : (dlp < -708.0 ? 0.0 : ff_exp(fmin(dlp, 708.0))); }

// The decision u < |psi(x')|^2 / |psi(x)|^2 (src/base_dist.py:66-68) taken as  u e^{R' - R} P^2 < P'^2,  R = sum_i r_i^2,  P the
// determinant of the POLYNOMIAL parts h_nx_j(x_i) h_ny_j(y_i) of the orbitals (the Gaussian of a row factors out of the determinant):
// no exp per particle, no log per determinant.  dRt = R - R'.  IEEE comparisons: a NaN on either side rejects; e^{R - R'} below the
// double range is the reference's p = 0 (reject).
FF_D bool ff_ratio_accept(double u, double dRt, double P2, double Pn2) {
  const double lhs = u * ff_exp(fmin(fmax(-dRt, -700.0), 708.0)) * P2;
  return (dRt >= -708.0) & (lhs < Pn2);
}

// What a lane knows of its walker.  LPW lanes per walker; lanes past the last walker shadow it (they take part in the barriers and
// lane exchanges and store nothing).  md: the largest Hermite degree in the workgroup, as a scalar (wave-uniform loop bounds in
// ff_herm_rec).
struct ff_mc_head { int64_t b; int sub; bool live; uint64_t wid; int md; };

// Lane `sub` of a walker decodes the N0 orbitals of its table (sub ? tab_dn : tab_up) of the walker's state into degrees
// o0 = [nx | ny] and, with N1 > 0, N1 orbitals of tab_dn into o1 (once, outside the step loop).
template <int LPW, int N0, int N1>
FF_D ff_mc_head ff_mc_preamble(int64_t B, const int* __restrict__ tab_up, const int* __restrict__ tab_dn, const int* __restrict__ wstate,
                               int64_t woff, int* o0, int* o1) {
  static_assert(LPW == 1 || LPW == 2, "one or two lanes per walker");
  __shared__ int s_md;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  ff_mc_head w;
  w.b = LPW == 2 ? gid >> 1 : gid;
  w.sub = LPW == 2 ? (int)(gid & 1) : 0;
  if (threadIdx.x == 0) s_md = 0;
  __syncthreads();
  w.live = w.b < B;
  if (!w.live) w.b = B - 1;
  const int st = wstate ? wstate[w.b] : 0;
  const int* __restrict__ tab = w.sub ? tab_dn : tab_up;
  int md = 0;
#pragma unroll
  for (int j = 0; j < N0; j++) ff_orb_decode(tab[st * N0 + j], o0[j], o0[N0 + j]);
#pragma unroll
  for (int j = 0; j < N1; j++) ff_orb_decode(tab_dn[st * N1 + j], o1[j], o1[N1 + j]);
#pragma unroll
  for (int j = 0; j < 2 * N0; j++) md = o0[j] > md ? o0[j] : md;
#pragma unroll
  for (int j = 0; j < 2 * N1; j++) md = o1[j] > md ? o1[j] : md;
  atomicMax(&s_md, md);
  __syncthreads();
  w.md = FF_UNIFORM(s_md);
  w.wid = (uint64_t)(woff + w.b);
  return w;
}

// A launch is GROUND when no per-walker state is given and both orbital tables are the list 0 .. NS-1 in order (closed shells: every
// GSVMC model).  Decided on the device, once per kernel, from scalar loads of the tables -- neither the host nor the C ABI knows their
// contents -- and the same for every wave of the launch.  (The pair kernel has one table: tab_b = tab_a.)
template <int NS>
FF_D bool ff_mc_is_ground(const int* __restrict__ tab_a, const int* __restrict__ tab_b, const int* __restrict__ wstate) {
  int bad = wstate != nullptr ? 1 : 0;
#pragma unroll
  for (int j = 0; j < NS; j++) bad |= (tab_a[j] ^ j) | (tab_b[j] ^ j);
  return FF_UNIFORM(bad) == 0;
}
// ff_mc_preamble of a ground launch: the degrees are the constants of ff_slater.h (the final log p, the reference's arithmetic, reads
// them from o0 and md like every launch; the step loop of the ratio chain does not read them at all), so there is no table to decode,
// no largest degree to agree on and no barrier.
template <int LPW, int NS>
FF_D ff_mc_head ff_mc_preamble_ground(int64_t B, int64_t woff, int* o0) {
  static_assert(LPW == 2, "the two-lanes-per-walker layouts");
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  ff_mc_head w;
  w.b = gid >> 1;
  w.sub = (int)(gid & 1);
  w.live = w.b < B;
  if (!w.live) w.b = B - 1;
#pragma unroll
  for (int j = 0; j < NS; j++) { o0[j] = ff_ground_nx(j); o0[NS + j] = ff_ground_ny(j); }
  w.md = ff_ground_md(NS);
  w.wid = (uint64_t)(woff + w.b);
  return w;
}

// Initial walkers: explicit (parity mode; ff_mcmc_continue) or step 0 of the walker's stream.
template <bool NOISE, class Layout>
FF_D void ff_mc_init(const Layout& L, const double* __restrict__ g0, double* x) {
  if (NOISE || g0 != nullptr) {
    L.load(g0 + L.w.b * Layout::M, x);
  } else {
    double u0;
    L.draw(0u, x, u0);
  }
}

// x_out, logp_out, acc_count: the latter two written by one lane per walker
template <class Layout>
FF_D void ff_mc_store(const Layout& L, const double* x, double logp, int nacc, double* __restrict__ x_out, double* __restrict__ logp_out,
                      int* __restrict__ acc_count) {
  if (!L.w.live) return;
  L.store(x_out + L.w.b * Layout::M, x);
  if (L.w.sub == 0) {
    if (logp_out) logp_out[L.w.b] = logp;
    if (acc_count) acc_count[L.w.b] = nacc;
  }
}

// The chain on log p.  NOISE: g0 (B, M), g (S, B, M), u (S, B) -- the noise of step s+1 is requested from HBM before step s is computed
// (one step of software pipelining: a walker's chain is serial, so without it every step would expose a full HBM round trip).
// Otherwise Philox counters (seed, woff + b); g0 != nullptr: the walkers to continue from.
template <bool NOISE, class Layout>
FF_D void ff_mc_logp_chain(const Layout& L, int64_t B, int steps, double tau, const double* __restrict__ g0, const double* __restrict__ g,
                           const double* __restrict__ u, double* __restrict__ x_out, double* __restrict__ logp_out,
                           uint8_t* __restrict__ accept, int* __restrict__ acc_count) {
  constexpr int MS = Layout::MS, M = Layout::M;
  const int64_t b = L.w.b;
  double x[MS], nx[MS];
  ff_mc_init<NOISE>(L, g0, x);
  double logp = L.logprob(x);
  int nacc = 0;
  double gq[MS], uq = 0.0;
  if (NOISE && steps > 0) {
    L.load(g + b * M, gq);
    uq = u[b];
  }
  for (int s = 0; s < steps; s++) {
    double uu = 0.0;
    if constexpr (NOISE) {
      ff_propose<MS>(x, tau, gq, nx);
      uu = uq;
      if (s + 1 < steps) {
        L.load(g + ((int64_t)(s + 1) * B + b) * M, gq);
        uq = u[(int64_t)(s + 1) * B + b];
      }
    } else {
      double z[MS];
      L.draw((uint32_t)(s + 1), z, uu);
      ff_propose<MS>(x, tau, z, nx);
    }
    const double nl = L.logprob(nx);
    const bool acc = uu < ff_accept_prob(nl - logp);   // NaN p -> reject, +inf p -> accept (IEEE), as torch
    if (acc) {
#pragma unroll
      for (int i = 0; i < MS; i++) x[i] = nx[i];
      logp = nl;
      nacc++;
    }
    if (accept && L.w.live && L.w.sub == 0) accept[(int64_t)s * B + b] = acc ? 1 : 0;
  }
  ff_mc_store(L, x, logp, nacc, x_out, logp_out, acc_count);
}

// The Philox-fed chain of the two-lanes-per-walker layouts (throughput mode).  Same stream, same walkers as ff_rng_fill + the noise-fed
// chain above; what differs is how a step is evaluated (~925 wave-instructions per step):
//  * the decision is ff_ratio_accept: the serial tail LU -> log -> exp -> compare of a step becomes determinant -> multiply -> compare;
//  * step s + 1's normals and uniform are drawn while step s is decided (they depend on nothing of it);
//  * R and P^2 of the current walker are carried; log|psi|^2 of the final walker is evaluated once at the end by the same routine as
//    everywhere else.
// Each lane holds its share of R (the two shares meet through one DPP swap) and the walker's P^2.
template <class Layout>
FF_D void ff_mc_ratio_chain(const Layout& L, int steps, double tau, const double* __restrict__ g0, double* __restrict__ x_out,
                            double* __restrict__ logp_out, int* __restrict__ acc_count) {
  constexpr int MS = Layout::MS;
  double x[MS], zq[MS], uq = 0.0;
  ff_mc_init<false>(L, g0, x);
  if (steps > 0) L.draw(1u, zq, uq);
  double Rc = L.r2sum(x), P2 = L.polydet2(x);
  int nacc = 0;
  for (int s = 0; s < steps; s++) {
    double nx[MS];
    ff_propose<MS>(x, tau, zq, nx);
    const double uu = uq;
    if (s + 1 < steps) L.draw((uint32_t)(s + 2), zq, uq);
    const double Rn = L.r2sum(nx), dR = Rc - Rn, dRt = dR + ff_swap1(dR);
    const double Pn2 = L.polydet2(nx);
    const bool acc = ff_ratio_accept(uu, dRt, P2, Pn2);
    if (acc) {
#pragma unroll
      for (int i = 0; i < MS; i++) x[i] = nx[i];
      Rc = Rn;
      P2 = Pn2;
      nacc++;
    }
  }
  ff_mc_store(L, x, L.logprob(x), nacc, x_out, logp_out, acc_count);
}

// ---------------------------------------------------------------------------------------------------
// One lane per walker: all M = 2 (NU + ND) coordinates, both determinants.  Quad q of a step's Philox blocks is the normals of
// coordinates 4q .. 4q+3, block NU + ND the uniform.
template <int NU, int ND>
struct ff_mc_one_lane {
  static_assert(NU > 0 && ND >= 0, "compile-time spin sizes");
  static constexpr int n = NU + ND, M = 2 * n, MS = M;
  ff_mc_head w;
  uint64_t seed;
  int ou[2 * NU], od[2 * (ND > 0 ? ND : 1)];
  FF_D void load(const double* __restrict__ row, double* dst) const {
#pragma unroll
    for (int i = 0; i < M; i++) dst[i] = row[i];
  }
  FF_D void store(double* __restrict__ row, const double* x) const {
#pragma unroll
    for (int i = 0; i < M; i++) row[i] = x[i];
  }
  FF_D void draw(uint32_t step, double* z, double& u) const {
#pragma unroll
    for (int q = 0; q < (M + 3) / 4; q++) {
      double z4[4];
      ff_normal_quad(seed, w.wid, step, (uint32_t)q, z4);
#pragma unroll
      for (int k = 0; k < 4; k++) if (4 * q + k < M) z[4 * q + k] = z4[k];
    }
    u = ff_uniform(seed, w.wid, step, (uint32_t)n);
  }
  FF_D double logprob(const double* x) const {
    double s = 0.0;
    s += ff_slater_logabsdet_reg<NU>(ou, ou + NU, x, w.md);
    if constexpr (ND > 0) s += ff_slater_logabsdet_reg<ND>(od, od + ND, x + 2 * NU, w.md);
    return 2.0 * s;
  }
};

// ---------------------------------------------------------------------------------------------------
// TWO lanes per walker, one per spin species (NU = ND = NS): at 65 536 walkers one lane per walker is one wave per SIMD and nothing
// hides the latency of its serial chain (Philox rounds, Box-Muller, pivots).  Lane (b, spin) holds the coordinates of its own particles
// and evaluates its own determinant; the two log|det| meet through one DPP swap (a + b is commutative: both lanes form the identical
// sum, and it is the reference's 2*(up + down)), both lanes take the same accept decision.
// Philox: the walker's blocks are dealt over its two lanes: lane 0 evaluates quads 0 .. mid, lane 1 the quads behind and the block of
// the uniform; for odd NS the second half of the middle quad and the uniform change lanes by one DPP swap (two blocks per lane and
// step at NS = 3 where every lane evaluated three).  Determinants up to 3 x 3 in closed form (no pivot search, no reciprocal).
// GROUND: the launch is ground (ff_mc_is_ground) -- polydet2 with compile-time degrees; everything else is the same code.
template <int NS, bool GROUND = false>
struct ff_mc_spin_lanes {
  static constexpr int MS = 2 * NS, M = 2 * MS, n = 2 * NS;
  static constexpr bool ODD = (NS & 1) != 0;
  static constexpr int MID = (NS - 1) / 2;                          // odd NS: the quad whose halves belong to different spins
  static constexpr int NB = ODD ? (NS + 1) / 2 : NS / 2 + 1;        // Philox blocks per lane and step
  ff_mc_head w;
  uint64_t seed;
  int oo[2 * NS];
  FF_D void load(const double* __restrict__ row, double* dst) const {
#pragma unroll
    for (int i = 0; i < MS; i++) dst[i] = row[w.sub * MS + i];
  }
  FF_D void store(double* __restrict__ row, const double* x) const {
#pragma unroll
    for (int i = 0; i < MS; i++) row[w.sub * MS + i] = x[i];
  }
  FF_D double logprob(const double* x) const {
    const double L = ff_slater_logabsdet_reg<NS>(oo, oo + NS, x, w.md);
    return 2.0 * (L + ff_swap1(L));
  }
  FF_D double r2sum(const double* x) const {
    double R = 0.0;
#pragma unroll
    for (int i = 0; i < MS; i++) R = fma(x[i], x[i], R);
    return R;
  }
  FF_D double polydet2(const double* x) const {      // (P_up P_dn)^2
    double P;
    if constexpr (GROUND) P = ff_slater_polydet_ground<NS>(x);
    else P = ff_slater_polydet_reg<NS>(oo, oo + NS, x, w.md);
    const double PP = P * ff_swap1(P);
    return PP * PP;
  }
  // this spin's normals of one step (z[i]: coordinate sub * MS + i of the walker) and the walker's uniform of that step
  FF_D void draw(uint32_t step, double* z, double& u) const {
    const int sp = w.sub;
    auto swap32 = [](uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true); };
    ff_u4 R[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) {
      uint32_t slot;
      if constexpr (ODD) slot = sp ? (uint32_t)(k < NB - 1 ? MID + 1 + k : n) : (uint32_t)k;
      else slot = (k < NB - 1) ? (uint32_t)(sp * (NS / 2) + k) : (uint32_t)n;
      R[k] = ff_philox(seed, w.wid, step, slot);
    }
    auto word = [&](int pair, int c) -> uint32_t {     // word c of pair `pair` of this lane's own blocks (static indices)
      const ff_u4& r = R[pair >> 1];
      return (pair & 1) ? (c ? r.w : r.z) : (c ? r.y : r.x);
    };
    uint32_t uh, ul;
    if constexpr (ODD) {
      const ff_u4& last = R[NB - 1];       // lane 0: the middle quad (its second half is lane 1's first pair); lane 1: the uniform's block
      const uint32_t r0 = swap32(sp ? last.x : last.z), r1 = swap32(sp ? last.y : last.w);
#pragma unroll
      for (int j = 0; j < NS; j++) {
        const uint32_t a0 = word(j, 0), a1 = word(j, 1);
        const uint32_t b0 = j == 0 ? r0 : word(j > 0 ? j - 1 : 0, 0), b1 = j == 0 ? r1 : word(j > 0 ? j - 1 : 0, 1);
        ff_normal_pair32(sp ? b0 : a0, sp ? b1 : a1, z[2 * j], z[2 * j + 1]);
      }
      uh = sp ? last.x : r0; ul = sp ? last.y : r1;
    } else {
#pragma unroll
      for (int j = 0; j < NS; j++) ff_normal_pair32(word(j, 0), word(j, 1), z[2 * j], z[2 * j + 1]);
      uh = R[NB - 1].x; ul = R[NB - 1].y;
    }
    u = ff_uniform_words(uh, ul);
  }
};

// ---------------------------------------------------------------------------------------------------
// ONE spin species (ndown = 0: the finite-temperature runs, src/BetaFermionHO2D.py) with TWO lanes per walker.  There is no second
// species to split off here, so the lanes split the PARTICLES: lane h of a walker owns the Philox quads q = h, h + 2, ... (quad q = the
// four normals of particles 2q, 2q + 1), proposes those particles' moves and evaluates their rows of the Slater matrix; the rows change
// hands through one DPP swap per entry, then both lanes run the same LU on the same matrix -- the same determinant bits, hence the
// same accept decision, as one lane per walker.
// slot s of a lane: particle pid(s) = 4 (s / 2) + 2 h + (s & 1)  (quad q = 2 (s / 2) + h); it exists if pid < NS
template <int NS, bool GROUND = false>
struct ff_mc_pair_lanes {
  static constexpr int M = 2 * NS, NQT = (NS + 1) / 2, NQL = (NQT + 1) / 2, NPL = 2 * NQL, MS = 2 * NPL;   // quads total / per lane, slots
  ff_mc_head w;
  uint64_t seed;
  int oo[2 * NS];
  FF_D int pid(int sl) const { return 4 * (sl >> 1) + 2 * w.sub + (sl & 1); }
  FF_D void load(const double* __restrict__ row, double* dst) const {     // this lane's coordinates of a (B, NS, 2) array row
#pragma unroll
    for (int sl = 0; sl < NPL; sl++) {
      const int p = pid(sl) < NS ? pid(sl) : 0;
      dst[2 * sl] = row[2 * p]; dst[2 * sl + 1] = row[2 * p + 1];
    }
  }
  FF_D void store(double* __restrict__ row, const double* x) const {
#pragma unroll
    for (int sl = 0; sl < NPL; sl++) {
      if (pid(sl) < NS) { row[2 * pid(sl)] = x[2 * sl]; row[2 * pid(sl) + 1] = x[2 * sl + 1]; }
    }
  }
  FF_D void draw(uint32_t step, double* z, double& u) const {
#pragma unroll
    for (int k = 0; k < NQL; k++) ff_normal_quad(seed, w.wid, step, (uint32_t)(2 * k + w.sub), z + 4 * k);
    u = ff_uniform(seed, w.wid, step, (uint32_t)NS);
  }
  // the walker's NS x NS matrix from the rows the two lanes hold (Dm: this lane's), the same on both lanes
  FF_D void gather(const double (&Dm)[NPL][NS], double (&Dfull)[NS][NS]) const {
#pragma unroll
    for (int i = 0; i < NS; i++) {
      const int q = i >> 1, owner = q & 1, sl = 2 * (q >> 1) + (i & 1);   // static: which lane and slot hold row i
#pragma unroll
      for (int j = 0; j < NS; j++) {
        const double mine = Dm[sl][j], other = ff_swap1(mine);
        Dfull[i][j] = (w.sub == owner) ? mine : other;
      }
    }
  }
  // log|psi|^2 of the walker whose coordinates (this lane's share) are in `xs`
  FF_D double logprob(const double* xs) const {
    double Dm[NPL][NS], Dfull[NS][NS];
#pragma unroll
    for (int sl = 0; sl < NPL; sl++) ff_slater_row_reg<NS>(oo, oo + NS, xs[2 * sl], xs[2 * sl + 1], w.md, Dm[sl]);
    gather(Dm, Dfull);
    return 2.0 * (0.0 + ff_lu_logabsdet_reg<NS>(Dfull));
  }
  // squared determinant of the polynomial parts of the orbitals, same exchange of rows
  FF_D double polydet2(const double* xs) const {
    double Dm[NPL][NS], Dfull[NS][NS];
#pragma unroll
    for (int sl = 0; sl < NPL; sl++) {
      if constexpr (GROUND) ff_poly_row_ground<NS>(xs[2 * sl], xs[2 * sl + 1], Dm[sl]);
      else ff_poly_row_reg<NS>(oo, oo + NS, xs[2 * sl], xs[2 * sl + 1], w.md, Dm[sl]);
    }
    gather(Dm, Dfull);
    const double P = ff_det_reg<NS>(Dfull);
    return P * P;
  }
  FF_D double r2sum(const double* xs) const {       // this lane's share of sum_i r_i^2 (absent particles: none)
    double r = 0.0;
#pragma unroll
    for (int sl = 0; sl < NPL; sl++) { const double t = fma(xs[2 * sl], xs[2 * sl], xs[2 * sl + 1] * xs[2 * sl + 1]); r += (pid(sl) < NS) ? t : 0.0; }
    return r;
  }
};

#ifdef FF_MCMC_BUILD_KERNELS   // defined by the one translation unit that owns the entry points (ff_walkers.hip)
template <int NU, int ND, bool NOISE>
__global__ void __launch_bounds__(128)
ff_mcmc_kernel(int64_t B, int nup_rt, int ndn_rt, const int* __restrict__ tab_up, const int* __restrict__ tab_dn,
               const int* __restrict__ wstate, int steps, double tau,
               const double* __restrict__ g0, const double* __restrict__ g, const double* __restrict__ u,
               uint64_t seed, int64_t woff,
               double* __restrict__ x_out, double* __restrict__ logp_out, uint8_t* __restrict__ accept,
               int* __restrict__ acc_count) {
  ff_mc_one_lane<NU, ND> L;
  L.w = ff_mc_preamble<1, NU, ND>(B, tab_up, tab_dn, wstate, woff, L.ou, L.od);
  L.seed = seed;
  ff_mc_logp_chain<NOISE>(L, B, steps, tau, g0, g, u, x_out, logp_out, accept, acc_count);
}

template <int NS, bool NOISE>
__global__ void __launch_bounds__(128)
ff_mcmc_spin_kernel(int64_t B, const int* __restrict__ tab_up, const int* __restrict__ tab_dn, const int* __restrict__ wstate,
                    int steps, double tau, const double* __restrict__ g0, const double* __restrict__ g,
                    const double* __restrict__ u, uint64_t seed, int64_t woff, double* __restrict__ x_out,
                    double* __restrict__ logp_out, uint8_t* __restrict__ accept, int* __restrict__ acc_count) {
  static_assert(NOISE, "the Philox-fed chain of this layout is ff_mcmc_spin_philox_kernel<NS, GROUND>");
  ff_mc_spin_lanes<NS> L;
  L.w = ff_mc_preamble<2, NS, 0>(B, tab_up, tab_dn, wstate, woff, L.oo, nullptr);
  L.seed = seed;
  ff_mc_logp_chain<true>(L, B, steps, tau, g0, g, u, x_out, logp_out, accept, acc_count);
}

// The Philox-fed kernels come in two instantiations, GROUND and not, and the host launches BOTH: each derives the launch's flag
// (ff_mc_is_ground) and the one it does not belong to returns at once -- a few scalar loads per wave.  One kernel with a uniform
// branch would hold the registers of the larger path (156 at NS = 3) while it runs the smaller one (96).
template <int NS, bool GROUND>
__global__ void __launch_bounds__(128)
ff_mcmc_spin_philox_kernel(int64_t B, const int* __restrict__ tab_up, const int* __restrict__ tab_dn, const int* __restrict__ wstate,
                           int steps, double tau, const double* __restrict__ g0, uint64_t seed, int64_t woff,
                           double* __restrict__ x_out, double* __restrict__ logp_out, int* __restrict__ acc_count) {
  if (ff_mc_is_ground<NS>(tab_up, tab_dn, wstate) != GROUND) return;      // wave-uniform, and the same in every wave of the launch
  ff_mc_spin_lanes<NS, GROUND> L;
  if constexpr (GROUND) L.w = ff_mc_preamble_ground<2, NS>(B, woff, L.oo);
  else L.w = ff_mc_preamble<2, NS, 0>(B, tab_up, tab_dn, wstate, woff, L.oo, nullptr);     // excited orbitals, per-walker states, one spin ground only
  L.seed = seed;
  ff_mc_ratio_chain(L, steps, tau, g0, x_out, logp_out, acc_count);
}

template <int NS, bool NOISE, bool GROUND = false>
__global__ void __launch_bounds__(128)
ff_mcmc_pair_kernel(int64_t B, const int* __restrict__ tab_up, const int* __restrict__ wstate, int steps, double tau,
                    const double* __restrict__ g0, const double* __restrict__ g, const double* __restrict__ u, uint64_t seed,
                    int64_t woff, double* __restrict__ x_out, double* __restrict__ logp_out, uint8_t* __restrict__ accept,
                    int* __restrict__ acc_count) {
  static_assert(!(NOISE && GROUND), "the noise-fed chain is the reference's arithmetic for every launch");
  if constexpr (!NOISE) {
    if (ff_mc_is_ground<NS>(tab_up, tab_up, wstate) != GROUND) return;
  }
  ff_mc_pair_lanes<NS, GROUND> L;
  if constexpr (GROUND) L.w = ff_mc_preamble_ground<2, NS>(B, woff, L.oo);
  else L.w = ff_mc_preamble<2, NS, 0>(B, tab_up, tab_up, wstate, woff, L.oo, nullptr);
  L.seed = seed;
  if constexpr (NOISE) ff_mc_logp_chain<true>(L, B, steps, tau, g0, g, u, x_out, logp_out, accept, acc_count);
  else ff_mc_ratio_chain(L, steps, tau, g0, x_out, logp_out, acc_count);
}

// materialise the Philox noise stream of the samplers above
__global__ void __launch_bounds__(128)
ff_rng_fill_kernel(int64_t B, int n, int steps, uint64_t seed, int64_t woff, double* __restrict__ g0,
                   double* __restrict__ g, double* __restrict__ u) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int M = 2 * n;
  const uint64_t wid = (uint64_t)(woff + b);
  for (int q = 0; 2 * q < n; q++) {
    double z4[4];
    ff_normal_quad(seed, wid, 0u, (uint32_t)q, z4);
    for (int k = 0; k < 4; k++) if (4 * q + k < M) g0[b * M + 4 * q + k] = z4[k];
  }
  for (int s = 0; s < steps; s++) {
    double* gs = g + ((int64_t)s * B + b) * M;
    for (int q = 0; 2 * q < n; q++) {
      double z4[4];
      ff_normal_quad(seed, wid, (uint32_t)(s + 1), (uint32_t)q, z4);
      for (int k = 0; k < 4; k++) if (4 * q + k < M) gs[4 * q + k] = z4[k];
    }
    u[(int64_t)s * B + b] = ff_uniform(seed, wid, (uint32_t)(s + 1), (uint32_t)n);
  }
}
#endif
