// ff_adj_direct_body.inc -- body of the direct-evaluation adjoint kernel (ff_cnf_adj.hip), included twice: by ff_ode_adj_kernel
// (LDS arrays declared statically) and by ff_ode_adj_lean_kernel (the same arrays as references into dynamic LDS).  Expects
// N, D, MAXU, M, G, P, R, NV, CH and the arrays s_w, s_z, s_kb, s_err, s_ad, s_rad, s_rinv, s_ca, s_cb, s_ph, s_hd, s_pa, s_pb,
// s_any, s_e2, s_st in scope -- and SCORES (constexpr bool), J0, JN (constexpr int: the launch integrates the parameter gradient of
// the lane's units j = J0 .. J0 + JN - 1 of its MAXU; 0 and MAXU everywhere but in the scores kernels).  SCORES = true is ff_ode_adj_scores_kernel: the same integration
// with the per-walker seeds of ff_cnf_adjoint_scores (a_z = az_in[b], a_Delta = -1), the accepted steps' parameter integrands added
// to row b of the (B, 3He+3Hm) scores -- per WALKER instead of per (workgroup, group-slot); A.rows points at the scores in this
// variant; the per-workgroup rows and A.gx_out are not involved.  Every difference is under `if constexpr (SCORES)`: the SCORES = false instantiations compile to what they were.
  const int lane = threadIdx.x;
  const int g = lane / M, i = lane % M;
  const bool ingrp = g < G;
  const int gg = ingrp ? g : 0;
  const int ai = i / D, ci = i % D;

  ff_load_weights(s_w, A.net, lane);
  ff_fill_exp2_table(s_e2, lane);
  if (lane == 0) {
    int p = 0;
    for (int a = 0; a < N; a++)
      for (int b = a + 1; b < N; b++) { s_pa[p] = a; s_pb[p] = b; p++; }
    for (int a = 0; a < N; a++) { if (P + a < R) { s_pa[P + a] = a; s_pb[P + a] = -1; } }
  }
  __syncthreads();
  const int He = A.net.He, Hm = A.net.Hm;
  const bool has_mu = Hm > 0;
  const int nrad = has_mu ? (P + N) : P;
  const double rtol = A.rtol, atol = A.atol;
  constexpr double NT = 2 * M;
  const int64_t ngroups = (A.B + G - 1) / G;
  if (threadIdx.x < 4) s_st[threadIdx.x] = 0;

  // This lane's slice of the parameter-gradient row of (workgroup, group-slot): entries of its own units only,
  // so accepted steps are added with plain (non-atomic) read-modify-writes.  The lane zeroes its entries itself (this kernel runs
  // only when the tabulated kernel did not serve the call: a 12 MB memset in front of every call was the price of that otherwise).
  double* const myrow = SCORES ? nullptr : A.rows + ((int64_t)blockIdx.x * G + (ingrp ? g : 0)) * (3 * He + 3 * Hm);
  constexpr int UC = M * MAXU;                 // hidden units per gradient chunk
  const int unit0 = A.unit0;
  const int nchunks = ((He > Hm ? He : Hm) + UC - 1) / UC;
  if constexpr (!SCORES) {
  if (ingrp) {
    for (int t = 0; t < 2; t++) {
      const int H = t ? Hm : He;
      for (int j = 0; j < MAXU; j++) {
        const int k = unit0 + i + j * M;
        if (k < H)
          for (int c = 0; c < 3; c++) myrow[(t ? 3 * He : 0) + c * H + k] = 0.0;
      }
    }
  }
  }
  auto row_add = [&](int t, int j, int c, double v) {
    const int k = unit0 + i + j * M, H = t ? Hm : He;
    if (ingrp && k < H) myrow[(t ? 3 * He : 0) + c * H + k] += v;
  };

  for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int64_t bq = grp * G + g;
    const bool valid = ingrp && bq < A.B;
    const int64_t b = ff_opt_load(A.order, valid, bq, A.z_in, (int32_t)bq);
    double y[NV], k0[NV], k1[NV], k2[NV], k3[NV], k4[NV], k5[NV];
    y[0] = ff_opt_load(A.z_in, valid, b * M + i, A.z_in, 0.25 * (i + 1) + 0.125 * ((i * 7) % 5));
    {
      // seeds: given, or formed from the local energies (ff_cnf_adjoint_energy); all loads branch-free (ff_opt_load)
      const bool ws = A.w_e != nullptr;
      const int wi = ff_opt_load(A.w_index, valid && ws, b, A.z_in, (int32_t)0);
      const double wb = (ff_opt_load(A.w_e, valid, b, A.z_in, 0.0) - ff_opt_load(A.w_mean, valid && ws, wi, A.z_in, 0.0)) * A.w_scale;
      const double az0 = ff_opt_load(A.az_in, valid, b * M + i, A.z_in, 0.0), ad0 = ff_opt_load(A.ad_in, valid, b, A.z_in, 0.0);
      y[1] = ws ? wb * az0 : az0;
      if constexpr (SCORES) {
        if (ingrp && i == 0) s_ad[g] = -1.0;
      } else {
        if (ingrp && i == 0) s_ad[g] = ws ? -wb : ad0;
      }
    }
    // SCORES: row b of the output, the lane's entries: zeroed here, accepted steps added by plain read-modify-writes in the order
    // row_add adds them to a workgroup row -- the row is the accumulator, as there (in registers the 6 MAXU sums of a lane put every
    // instantiation that runs at 512 registers into scratch inside the step loop: DESIGN.md 3v)
    double* const srow = SCORES ? A.rows + b * (int64_t)(3 * He + 3 * Hm) : nullptr;
    auto score_entry = [&](int t, int j, int c) -> double* {
      const int k = unit0 + i + (J0 + j) * M, H = t ? Hm : He;
      return (valid && k < H) ? srow + (t ? 3 * He : 0) + c * H + k : nullptr;
    };
    bool rej_last = false;      // SCORES: this walker's own last decision was a rejection (statistics, below)
    if constexpr (SCORES) {
      for (int t = 0; t < 2; t++)
        for (int j = 0; j < JN; j++)
          for (int c = 0; c < 3; c++)
            if (double* q = score_entry(t, j, c)) *q = 0.0;
    }
    // tent = B0*k0_theta + sum_{s=2..5} B_s*k_s_theta of the step under way (dropped if the step is rejected)
    double tent[2][JN][3];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int j = 0; j < JN; j++)
#pragma unroll
        for (int c = 0; c < 3; c++) tent[t][j][c] = 0.0;
    ff_stepper S;
    S.begin(A.ta, A.tb, valid);
    // warm start (ff_ode.walker_h_init): the step size to try first, instead of the probe evaluation of the Hairer start
    const double hwarm = ff_open_step(ff_opt_load(A.h_init, valid, A.h_scale < 0.0 ? 0 : b, A.z_in, 0.0) * fabs(A.h_scale), A.ta, A.tb, A.h_equal);
    const bool warm = hwarm > 0.0;
    double hmax_acc = 0.0;
    int s = -2, nev = 0;
    double h0v = 0.0, d1v = 0.0;

    auto group_sum = [&](double part) -> double {
      if (ingrp) s_err[g][i] = part;
      __syncthreads();
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < M; j++) t += s_err[gg][j];
      __syncthreads();
      return t;
    };

#pragma unroll 1
    for (;;) {
      double in[NV];
      const double h = S.h;
      switch (s) {
        case -2: case 0:
#pragma unroll
          for (int v = 0; v < NV; v++) in[v] = y[v];
          break;
        case -1:
#pragma unroll
          for (int v = 0; v < NV; v++) in[v] = fma(h0v * S.dir, k0[v], y[v]);
          break;
        case 1:
#pragma unroll
          for (int v = 0; v < NV; v++) in[v] = fma(h * FF_A10, k0[v], y[v]);
          break;
        case 2:
#pragma unroll
          for (int v = 0; v < NV; v++) in[v] = fma(h, FF_A20 * k0[v] + FF_A21 * k1[v], y[v]);
          break;
        case 3:
#pragma unroll
          for (int v = 0; v < NV; v++) in[v] = fma(h, FF_A30 * k0[v] + FF_A31 * k1[v] + FF_A32 * k2[v], y[v]);
          break;
        case 4:
#pragma unroll
          for (int v = 0; v < NV; v++)
            in[v] = fma(h, FF_A40 * k0[v] + FF_A41 * k1[v] + FF_A42 * k2[v] + FF_A43 * k3[v], y[v]);
          break;
        case 5:
#pragma unroll
          for (int v = 0; v < NV; v++)
            in[v] = fma(h, FF_A50 * k0[v] + FF_A51 * k1[v] + FF_A52 * k2[v] + FF_A53 * k3[v] + FF_A54 * k4[v], y[v]);
          break;
        default:
#pragma unroll
          for (int v = 0; v < NV; v++)
            in[v] = fma(h, FF_B0 * k0[v] + FF_B2 * k2[v] + FF_B3 * k3[v] + FF_B4 * k4[v] + FF_B5 * k5[v], y[v]);
          break;
      }
      // ------------------------------------------------------------------ publish z_i, a_i
      __syncthreads();
      if (ingrp) { s_z[g][i] = in[0]; s_kb[g][i] = in[1]; }
      __syncthreads();
      // ------------------------------------------------------------------ radius set-up (lane <-> radius)
      for (int q = lane; q < G * nrad; q += FF_WAVE) {
        const int qg = q / nrad, p = q - qg * nrad;
        const int a = s_pa[p], bb = s_pb[p];
        double r2 = 0.0, al = 0.0;
#pragma unroll
        for (int c = 0; c < D; c++) {
          const double rho = s_z[qg][a * D + c] - (bb >= 0 ? s_z[qg][bb * D + c] : 0.0);
          const double dl = s_kb[qg][a * D + c] - (bb >= 0 ? s_kb[qg][bb * D + c] : 0.0);
          r2 = fma(rho, rho, r2);
          al = fma(dl, rho, al);
        }
        const double r = sqrt(r2), ad = s_ad[qg];
        s_rad[qg][p] = r;
        s_rinv[qg][p] = ff_rcp(r);
        // integrand of the parameter adjoint is  ca * df(r)/dtheta + cb * df'(r)/dtheta
        s_ca[qg][p] = bb >= 0 ? -(al - 2.0 * D * ad) : -(al - D * ad);
        s_cb[qg][p] = bb >= 0 ? 2.0 * ad * r : ad * r;
      }
      __syncthreads();
      if constexpr (SCORES) {
        // the evaluations THIS walker would take alone (its group mates' probe and their passes through stage 0 are not its own):
        // stats[0] is then the sum over one-walker calls, whatever the grouping
        nev += (s == -2 || (s == -1 ? (!S.done && !warm) : (s == 0 ? rej_last : !S.done))) ? 1 : 0;
      } else {
        nev++;
      }
      // ------------------------------------------------------------------ unit phase
      double cur[2][JN][3];
#pragma unroll
      for (int t = 0; t < 2; t++)
#pragma unroll
        for (int j = 0; j < JN; j++) cur[t][j][0] = cur[t][j][1] = cur[t][j][2] = 0.0;
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const int H = t ? Hm : He;
        const int p_lo = t ? P : 0, p_hi = t ? nrad : P;
        for (int pc = p_lo; pc < p_hi; pc += CH) {
          const int pe = pc + CH < p_hi ? pc + CH : p_hi;
          for (int p = pc; p < pe; p++) {
          const double r = s_rad[gg][p], ca = s_ca[gg][p], cb = s_cb[gg][p];
          double h0 = 0.0, h1 = 0.0, h2 = 0.0;
          // this lane's units, MAXU side by side (units beyond H are masked: their weights read as zero); every chunk of
          // the net contributes to the heads, the chunk starting at unit0 also to this launch's parameter integrands
          for (int uc = 0; uc < nchunks; uc++) {
            const bool mine = uc * UC == unit0;
            ff_wtab w[MAXU];
            double a[MAXU], sgv[MAXU], mk[MAXU];
#pragma unroll
            for (int j = 0; j < MAXU; j++) {
              const int k = uc * UC + i + j * M;
              w[j] = s_w[t][k < FF_HMAX ? k : FF_HMAX - 1];
              mk[j] = k < H ? 1.0 : 0.0;
              a[j] = fma(w[j].w1, r, w[j].b1);
            }
            ff_sigmoid_n<MAXU, false>(a, sgv, s_e2);
#pragma unroll
            for (int j = 0; j < MAXU; j++) {
              const double sg = sgv[j];
              const double s1 = sg * (1.0 - sg), s2 = s1 * fma(-2.0, sg, 1.0);
              const double w2 = mk[j] * w[j].w2, w2w1 = w2 * w[j].w1;
              h0 = fma(w2, sg, h0);
              h1 = fma(w2w1, s1, h1);
              h2 = fma(w2w1 * w[j].w1, s2, h2);
              if (mine && j >= J0 && j < J0 + JN) {      // (J0 = 0, JN = MAXU except in the scores kernels: all of the lane's units)
                const double w1rs2 = w[j].w1 * r * s2;
                cur[t][j - J0][0] += w2 * fma(ca * r, s1, cb * (s1 + w1rs2));
                cur[t][j - J0][1] += fma(ca * w2, s1, cb * w2w1 * s2);
                cur[t][j - J0][2] += mk[j] * fma(ca, sg, cb * w[j].w1 * s1);
              }
            }
          }
          if (ingrp) { s_ph[g][i][p - pc][0] = h0; s_ph[g][i][p - pc][1] = h1; s_ph[g][i][p - pc][2] = h2; }
          }
          __syncthreads();
          // reduce this chunk's partial heads over the group's lanes
          for (int e = i; e < (pe - pc) * 3; e += M) {
            const int q = e / 3, m = e - 3 * q;
            double tsum = 0.0;
#pragma unroll
            for (int l = 0; l < M; l++) tsum += s_ph[gg][l][q][m];
            if (ingrp) s_hd[g][pc + q][m] = tsum;
          }
          __syncthreads();
        }
      }
      // ------------------------------------------------------------------ component phase
      double out[NV];
      {
        const double* sz = s_z[gg];
        const double* sl = s_kb[gg];
        double vi = 0.0, dvk = 0.0, gdi = 0.0;
        for (int bq = 0; bq < N; bq++) {
          if (bq == ai) continue;
          const int lo = bq < ai ? bq : ai, hi = bq < ai ? ai : bq;
          const int p = ff_pair_index(N, lo, hi);
          const double rc = sz[ai * D + ci] - sz[bq * D + ci];
          const double f0 = s_hd[gg][p][0], f1 = s_hd[gg][p][1], f2 = s_hd[gg][p][2];
          double rdk = 0.0;
#pragma unroll
          for (int c = 0; c < D; c++) rdk = fma(sz[ai * D + c] - sz[bq * D + c], sl[ai * D + c] - sl[bq * D + c], rdk);
          const double ri = s_rinv[gg][p], r1 = rdk * ri;
          vi = fma(f0, rc, vi);
          dvk += fma(f1 * r1, rc, f0 * (sl[ai * D + ci] - sl[bq * D + ci]));
          const double sp = fma(f2, s_rad[gg][p], (1.0 + D) * f1);
          gdi = fma(2.0 * sp * ri, rc, gdi);
        }
        if (has_mu) {
          const int p = P + ai;
          const double rc = sz[ai * D + ci];
          const double f0 = s_hd[gg][p][0], f1 = s_hd[gg][p][1], f2 = s_hd[gg][p][2];
          double rdk = 0.0;
#pragma unroll
          for (int c = 0; c < D; c++) rdk = fma(sz[ai * D + c], sl[ai * D + c], rdk);
          const double ri = s_rinv[gg][p], r1 = rdk * ri;
          vi = fma(f0, rc, vi);
          dvk += fma(f1 * r1, rc, f0 * sl[ai * D + ci]);
          const double sp = fma(f2, s_rad[gg][p], (1.0 + D) * f1);
          gdi = fma(sp * ri, rc, gdi);
        }
        out[0] = vi;
        out[1] = fma(s_ad[gg], gdi, -dvk);
      }
      // ------------------------------------------------------------------ consume
      if (s == -2) {
#pragma unroll
        for (int v = 0; v < NV; v++) k0[v] = out[v];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
          for (int j = 0; j < JN; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) tent[t][j][c] = FF_B0 * cur[t][j][c];
        double p0 = 0.0, p1 = 0.0;
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const double isc = ff_rcp(fma(fabs(y[v]), rtol, atol));
          p0 = fma(y[v] * isc, y[v] * isc, p0);
          p1 = fma(k0[v] * isc, k0[v] * isc, p1);
        }
        const double d0 = sqrt(group_sum(p0) * (1.0 / NT));
        d1v = sqrt(group_sum(p1) * (1.0 / NT));
        h0v = S.h0(d0, d1v);
        s = -1;
        // every walker of the wave brings its own first step: no probe evaluation
        if (!ff_wave_or(&s_any, lane, (!S.done && !warm) ? 1 : 0)) {
          S.habs = fmin(hwarm, S.interval);
          S.plan();
          s = 1;
        }
      } else if (s == -1) {
        double p2 = 0.0;
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const double t = (out[v] - k0[v]) * ff_rcp(fma(fabs(y[v]), rtol, atol));
          p2 = fma(t, t, p2);
        }
        const double d2 = sqrt(group_sum(p2) * (1.0 / NT)) / h0v;
        S.init_habs(h0v, d1v, d2);
        if (warm) S.habs = fmin(hwarm, S.interval);
        S.plan();
        s = 1;
      } else if (s == 0) {   // re-evaluated f(y) after a rejection (k0 and its parameter integrand)
#pragma unroll
        for (int v = 0; v < NV; v++) k0[v] = out[v];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
          for (int j = 0; j < JN; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) tent[t][j][c] = FF_B0 * cur[t][j][c];
        s = 1;
      } else if (s >= 1 && s <= 5) {
        const double bw = s == 1 ? 0.0 : (s == 2 ? FF_B2 : (s == 3 ? FF_B3 : (s == 4 ? FF_B4 : FF_B5)));
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
          for (int j = 0; j < JN; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) tent[t][j][c] = fma(bw, cur[t][j][c], tent[t][j][c]);
        if (s == 1) {
#pragma unroll
          for (int v = 0; v < NV; v++) k1[v] = out[v];
        } else if (s == 2) {
#pragma unroll
          for (int v = 0; v < NV; v++) k2[v] = out[v];
        } else if (s == 3) {
#pragma unroll
          for (int v = 0; v < NV; v++) k3[v] = out[v];
        } else if (s == 4) {
#pragma unroll
          for (int v = 0; v < NV; v++) k4[v] = out[v];
        } else {
#pragma unroll
          for (int v = 0; v < NV; v++) k5[v] = out[v];
        }
        s++;
      } else {
        double pe = 0.0;
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const double e = h * (FF_E0 * k0[v] + FF_E2 * k2[v] + FF_E3 * k3[v] + FF_E4 * k4[v] + FF_E5 * k5[v] + FF_E6 * out[v]);
          const double t = e * ff_rcp(fma(fmax(fabs(y[v]), fabs(in[v])), rtol, atol));
          pe = fma(t, t, pe);
        }
        const double err = sqrt(group_sum(pe) * (1.0 / NT));
        const bool was_active = !S.done;
        const bool acc = S.decide(err, A.max_steps);
        if (acc) hmax_acc = fmax(hmax_acc, fabs(h));
        if (acc) {
#pragma unroll
          for (int v = 0; v < NV; v++) { y[v] = in[v]; k0[v] = out[v]; }
        }
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
          for (int j = 0; j < JN; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
              if constexpr (SCORES) {
                if (acc) {
                  if (double* q = score_entry(t, j, c)) *q += h * tent[t][j][c];
                }
              } else {
                if (acc) row_add(t, j, c, h * tent[t][j][c]);
              }
              tent[t][j][c] = acc ? FF_B0 * cur[t][j][c] : 0.0;   // FSAL: k6_theta opens the next step
            }
        if constexpr (SCORES) rej_last = was_active && !acc;
        S.plan();
        const int any = ff_wave_or(&s_any, lane, S.done ? 0 : ((was_active && !acc) ? 3 : 1));
        if (!any) break;
        s = (any & 2) ? 0 : 1;   // somebody rejected: the whole wave passes through stage 0
      }
    }
    if (valid) {
      // failed integration (NaN error norm, max_steps): NaN into this walker's x-gradient and into the parameter gradient
      const double bad = S.fail ? __builtin_nan("") : 0.0;
      if constexpr (SCORES) {
        if (S.fail) {      // every entry of the row
          for (int t = 0; t < 2; t++)
            for (int j = 0; j < JN; j++)
              for (int c = 0; c < 3; c++)
                if (double* q = score_entry(t, j, c)) *q = bad;
        }
      } else {
        if (A.gx_out) A.gx_out[b * M + i] = y[1] + bad;
      }
      if (i == 0) {
        if constexpr (!SCORES) {
          if (S.fail && unit0 == 0) row_add(0, 0, 0, bad);
        }
        if (A.h_out) A.h_out[b] = hmax_acc > 0.0 ? hmax_acc : hwarm;
        if (A.wcost) A.wcost[b] = S.nacc + S.nrej;
        if (A.stats && unit0 == 0 && J0 == 0) { atomicAdd(&s_st[0], nev); atomicMax(&s_st[1], S.nacc); atomicAdd(&s_st[2], S.nrej); if (S.fail) atomicMax(&s_st[3], 1); }
      }
    }
    __syncthreads();
  }
  // (rows are summed deterministically by ff_rows_reduce_kernel)
  __syncthreads();
  if (A.stats && threadIdx.x == 0 && (s_st[0] || s_st[3])) {
    atomicAdd(&A.stats[0], s_st[0]);
    atomicMax(&A.stats[1], s_st[1]);
    atomicAdd(&A.stats[2], s_st[2]);
    if (s_st[3]) atomicMax(&A.stats[3], 1);
  }
