/* ffo_core.inc -- ORACLE (test infrastructure, not product code).
 *
 * Generic core of the CPU restatement of FermiFlow's VMC hot path, written once over a
 * truncated-Taylor ("jet") number type and included three times by ff_oracle.c with
 * FFO_ORDER = 0 (plain double), 1 (value + first directional derivative) and 2 (+ second).
 * A jet represents f(eps) = v + d1*eps + d2*eps^2/2 along one seeded direction; arithmetic on the
 * value part is exactly the double arithmetic the reference performs, so order-0 results are the
 * reference's numbers and order-1/2 results are what torch.autograd differentiates them to.
 *
 * Every function cites the reference file:line it follows (paths relative to /root/reference).
 */

#if FFO_ORDER == 0
typedef struct { double v; } JN(jet);
#elif FFO_ORDER == 1
typedef struct { double v, d1; } JN(jet);
#else
typedef struct { double v, d1, d2; } JN(jet);
#endif
#define jet JN(jet)

#if FFO_ORDER >= 1
#define D1(x) ((x).d1)
#else
#define D1(x) 0.0
#endif
#if FFO_ORDER >= 2
#define D2(x) ((x).d2)
#else
#define D2(x) 0.0
#endif

static inline jet JN(jc)(double c) { jet r; r.v = c;
#if FFO_ORDER >= 1
  r.d1 = 0.0;
#endif
#if FFO_ORDER >= 2
  r.d2 = 0.0;
#endif
  return r; }
static inline jet JN(jmk)(double v, double d1, double d2) { jet r; r.v = v; (void)d1; (void)d2;
#if FFO_ORDER >= 1
  r.d1 = d1;
#endif
#if FFO_ORDER >= 2
  r.d2 = d2;
#endif
  return r; }
static inline jet JN(jadd)(jet a, jet b) { return JN(jmk)(a.v + b.v, D1(a) + D1(b), D2(a) + D2(b)); }
static inline jet JN(jsub)(jet a, jet b) { return JN(jmk)(a.v - b.v, D1(a) - D1(b), D2(a) - D2(b)); }
static inline jet JN(jneg)(jet a) { return JN(jmk)(-a.v, -D1(a), -D2(a)); }
static inline jet JN(jmul)(jet a, jet b) {
  return JN(jmk)(a.v * b.v, D1(a) * b.v + a.v * D1(b), D2(a) * b.v + 2.0 * D1(a) * D1(b) + a.v * D2(b)); }
static inline jet JN(jscale)(double c, jet a) { return JN(jmk)(c * a.v, c * D1(a), c * D2(a)); }
static inline jet JN(jaddc)(jet a, double c) { return JN(jmk)(a.v + c, D1(a), D2(a)); }
static inline jet JN(jdiv)(jet a, jet b) {
  double q = a.v / b.v;
  double q1 = (D1(a) - q * D1(b)) / b.v;
  double q2 = (D2(a) - 2.0 * q1 * D1(b) - q * D2(b)) / b.v;
  return JN(jmk)(q, q1, q2); }
static inline jet JN(jsqrt)(jet a) {
  double s = sqrt(a.v);
  double s1 = D1(a) / (2.0 * s);
  double s2 = (D2(a) - 2.0 * s1 * s1) / (2.0 * s);
  return JN(jmk)(s, s1, s2); }
static inline jet JN(jexp)(jet a) {
  double e = exp(a.v);
  return JN(jmk)(e, e * D1(a), e * (D2(a) + D1(a) * D1(a))); }
static inline jet JN(jlogabs)(jet a) {
  double l1 = D1(a) / a.v;
  return JN(jmk)(log(fabs(a.v)), l1, D2(a) / a.v - l1 * l1); }
/* torch.sigmoid(a) = 1/(1+exp(-a)) */
static inline jet JN(jsigmoid)(jet a) {
  double s = 1.0 / (1.0 + exp(-a.v));
  double s1 = s * (1.0 - s), s2 = s1 * (1.0 - 2.0 * s);
  return JN(jmk)(s, s1 * D1(a), s2 * D1(a) * D1(a) + s1 * D2(a)); }
/* x**k as torch evaluates it on CPU: k=2 -> x*x, k=3 -> x*x*x, otherwise std::pow */
static inline jet JN(jpowi)(jet a, int k) {
  double x = a.v, p, p1, p2;
  if (k == 0) return JN(jc)(1.0);
  if (k == 1) return a;
  if (k == 2) { p = x * x; p1 = 2.0 * x; p2 = 2.0; }
  else if (k == 3) { p = x * x * x; p1 = 3.0 * x * x; p2 = 6.0 * x; }
  else { p = pow(x, (double)k); p1 = k * pow(x, (double)(k - 1)); p2 = (double)k * (k - 1) * pow(x, (double)(k - 2)); }
  return JN(jmk)(p, p1 * D1(a), p2 * D1(a) * D1(a) + p1 * D2(a)); }

/* ------------------------------------------------------------------------------------------
 * 1-D normalised Hermite functions h_0..h_7, written term by term as src/orbitals.py:65-74.   */
static jet JN(herm1d)(int n, jet x) {
#define P(k) JN(jpowi)(x, k)
#define S(c, a) JN(jscale)(c, a)
  switch (n) {
    case 0: return JN(jc)(1.0);
    case 1: return S(sqrt(2.0), x);
    case 2: return S(1.0 / sqrt(2.0), JN(jaddc)(S(2.0, P(2)), -1.0));
    case 3: return S(1.0 / sqrt(3.0), JN(jsub)(S(2.0, P(3)), S(3.0, x)));
    case 4: return S(1.0 / sqrt(6.0), JN(jaddc)(JN(jsub)(S(2.0, P(4)), S(6.0, P(2))), 1.5));
    case 5: return S(1.0 / sqrt(15.0), JN(jadd)(JN(jsub)(S(2.0, P(5)), S(10.0, P(3))), S(7.5, x)));
    case 6: return S(1.0 / sqrt(5.0),
                     JN(jaddc)(JN(jadd)(JN(jsub)(S(2.0 / 3.0, P(6)), S(5.0, P(4))), S(7.5, P(2))), -1.25));
    default: return S(1.0 / sqrt(70.0),
                      JN(jsub)(JN(jadd)(JN(jsub)(S(4.0 / 3.0, P(7)), S(14.0, P(5))), S(35.0, P(3))), S(17.5, x)));
  }
#undef P
#undef S
}

/* orbital k of HO2D().orbitals: list order "for n in range(8) for nx in range(n+1): (nx, n-nx)"
 * (src/orbitals.py:81);  phi = pi^-1/2 * exp(-0.5*(x^2+y^2)) * h_nx(x) * h_ny(y)  (:76-79).     */
static jet JN(orbital2d)(int k, jet x, jet y) {
  int shell = 0;
  while ((shell + 1) * (shell + 2) / 2 <= k) shell++;
  int nx = k - shell * (shell + 1) / 2, ny = shell - nx;
  jet r2 = JN(jadd)(JN(jmul)(x, x), JN(jmul)(y, y));
  jet g = JN(jscale)(1.0 / sqrt(M_PI), JN(jexp)(JN(jscale)(-0.5, r2)));
  jet hx = JN(herm1d)(nx, x), hy = JN(herm1d)(ny, y);
  if (nx == 0 && ny == 0) return g;           /* "* 1 * 1" */
  if (nx == 0) return JN(jmul)(g, hy);
  if (ny == 0) return JN(jmul)(g, hx);
  return JN(jmul)(JN(jmul)(g, hx), hy);
}

/* HO3D (no upstream counterpart: the reference hard-codes two dimensions, src/orbitals.py:56, src/base_dist.py:62;
 * SURVEY 8(f).4): the same construction one dimension up -- orbital k of the list "for n in range(..) for nx in
 * range(n+1) for ny in range(n+1-nx): (nx, ny, n-nx-ny)", phi = pi^-3/4 exp(-r^2/2) h_nx(x) h_ny(y) h_nz(z), E = n + 3/2. */
static void JN(ho3d_decode)(int k, int* nx, int* ny, int* nz) {
  int shell = 0;
  while ((shell + 1) * (shell + 2) * (shell + 3) / 6 <= k) shell++;
  int idx = k - shell * (shell + 1) * (shell + 2) / 6;
  for (int a = 0; a <= shell; a++) {
    int cnt = shell - a + 1;
    if (idx < cnt) { *nx = a; *ny = idx; *nz = shell - a - idx; return; }
    idx -= cnt;
  }
  *nx = *ny = *nz = 0;
}
static jet JN(orbital3d)(int k, jet x, jet y, jet z) {
  int nx, ny, nz;
  JN(ho3d_decode)(k, &nx, &ny, &nz);
  jet r2 = JN(jadd)(JN(jadd)(JN(jmul)(x, x), JN(jmul)(y, y)), JN(jmul)(z, z));
  jet g = JN(jscale)(pow(M_PI, -0.75), JN(jexp)(JN(jscale)(-0.5, r2)));
  return JN(jmul)(JN(jmul)(JN(jmul)(g, JN(herm1d)(nx, x)), JN(herm1d)(ny, y)), JN(herm1d)(nz, z));
}

/* log|det D|, D[i][j] = phi_{orb[j]}(r_i)  (src/slater.py:28-36); LU with partial pivoting by
 * |value| as LAPACK getrf does behind torch.slogdet; logabsdet = sum log|U_ii|, -inf at an exactly zero pivot.  d = 2: HO2D, d = 3: HO3D. */
static jet JN(slater_logabsdet_d)(int n, int d, const int* orb, const jet* xy /* n*d */) {
  jet D[FFO_MAXN * FFO_MAXN];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      D[i * n + j] = d == 2 ? JN(orbital2d)(orb[j], xy[2 * i], xy[2 * i + 1])
                            : JN(orbital3d)(orb[j], xy[3 * i], xy[3 * i + 1], xy[3 * i + 2]);
  jet acc = JN(jc)(0.0);
  for (int c = 0; c < n; c++) {
    int p = c; double best = fabs(D[c * n + c].v);
    for (int r = c + 1; r < n; r++) if (fabs(D[r * n + c].v) > best) { best = fabs(D[r * n + c].v); p = r; }
    if (p != c) for (int j = 0; j < n; j++) { jet t = D[c * n + j]; D[c * n + j] = D[p * n + j]; D[p * n + j] = t; }
    jet piv = D[c * n + c];
    acc = JN(jadd)(acc, JN(jlogabs)(piv));
    if (piv.v == 0.0) continue;   /* getf2: a zero pivot is det = 0, the column (all zero below it) is not eliminated */
    for (int r = c + 1; r < n; r++) {
      jet f = JN(jdiv)(D[r * n + c], piv);
      for (int j = c + 1; j < n; j++) D[r * n + j] = JN(jsub)(D[r * n + j], JN(jmul)(f, D[c * n + j]));
    }
  }
  return acc;
}
static jet JN(slater_logabsdet)(int n, const int* orb, const jet* xy /* n*2 */) { return JN(slater_logabsdet_d)(n, 2, orb, xy); }

/* FreeFermion.log_prob: 2*(log|det up| + log|det down|), x[..., :nup, :] is spin-up
 * (src/base_dist.py:49-56).                                                                      */
static jet JN(logprob_d)(int nup, int ndn, int d, const int* orb_up, const int* orb_dn, const jet* xy) {
  jet s = JN(jc)(0.0);
  if (nup) s = JN(jadd)(s, JN(slater_logabsdet_d)(nup, d, orb_up, xy));
  if (ndn) s = JN(jadd)(s, JN(slater_logabsdet_d)(ndn, d, orb_dn, xy + d * nup));
  return JN(jscale)(2.0, s);
}
static jet JN(logprob)(int nup, int ndn, const int* orb_up, const int* orb_dn, const jet* xy) {
  return JN(logprob_d)(nup, ndn, 2, orb_up, orb_dn, xy);
}

/* MLP.forward (src/MLP.py:30-32): fc2(sigmoid(fc1(r)));  MLP.grad (:37-45). */
static void JN(mlp)(int H, const double* w1, const double* b1, const double* w2, jet r, jet* val, jet* dval) {
  jet s = JN(jc)(0.0), g = JN(jc)(0.0);
  for (int h = 0; h < H; h++) {
    jet a = JN(jsigmoid)(JN(jaddc)(JN(jscale)(w1[h], r), b1[h]));
    s = JN(jadd)(s, JN(jscale)(w2[h], a));
    if (dval) {
      jet da = JN(jmul)(a, JN(jaddc)(JN(jneg)(a), 1.0));              /* d_sigmoid(output) = output*(1-output) */
      g = JN(jadd)(g, JN(jscale)(w1[h], JN(jscale)(w2[h], da)));      /* (fc2.weight*dsig) @ fc1.weight */
    }
  }
  *val = s;
  if (dval) *dval = g;
}

/* Backflow.forward and .divergence (src/equivariant_funs.py:17-102) for one walker.
 * z: n*d jets.  v: n*d jets (may be NULL), div: jet (may be NULL).                               */
static void JN(backflow)(const ffo_net* net, int n, int d, const jet* z, jet* v, jet* div) {
  if (v) {
    /* _e_e with the reference's "+eye" diagonal and the eta(sqrt(d)) correction (:26-31) */
    jet diag;
    { jet one = JN(jc)(0.0); for (int c = 0; c < d; c++) one = JN(jaddc)(one, 1.0);
      JN(mlp)(net->He, net->ew1, net->eb1, net->ew2, JN(jsqrt)(one), &diag, NULL); }
    for (int i = 0; i < n; i++) {
      jet acc[3]; for (int c = 0; c < d; c++) acc[c] = JN(jc)(0.0);
      for (int j = 0; j < n; j++) {
        jet rij[3], r2 = JN(jc)(0.0);
        for (int c = 0; c < d; c++) {
          rij[c] = JN(jsub)(z[i * d + c], z[j * d + c]);
          if (i == j) rij[c] = JN(jaddc)(rij[c], 1.0);
          r2 = JN(jadd)(r2, JN(jmul)(rij[c], rij[c]));
        }
        jet eta; JN(mlp)(net->He, net->ew1, net->eb1, net->ew2, JN(jsqrt)(r2), &eta, NULL);
        for (int c = 0; c < d; c++) acc[c] = JN(jadd)(acc[c], JN(jmul)(eta, rij[c]));
      }
      for (int c = 0; c < d; c++) v[i * d + c] = JN(jsub)(acc[c], diag);
    }
    if (net->Hm > 0) {                                               /* _e_n (:63-64) */
      for (int i = 0; i < n; i++) {
        jet r2 = JN(jc)(0.0);
        for (int c = 0; c < d; c++) r2 = JN(jadd)(r2, JN(jmul)(z[i * d + c], z[i * d + c]));
        jet mu; JN(mlp)(net->Hm, net->mw1, net->mb1, net->mw2, JN(jsqrt)(r2), &mu, NULL);
        for (int c = 0; c < d; c++) v[i * d + c] = JN(jadd)(v[i * d + c], JN(jmul)(mu, z[i * d + c]));
      }
    }
  }
  if (div) {
    jet s = JN(jc)(0.0);
    for (int i = 0; i < n; i++)                                      /* _e_e_divergence (:44-50), pairs i<j */
      for (int j = i + 1; j < n; j++) {
        jet r2 = JN(jc)(0.0);
        for (int c = 0; c < d; c++) { jet t = JN(jsub)(z[i * d + c], z[j * d + c]); r2 = JN(jadd)(r2, JN(jmul)(t, t)); }
        jet r = JN(jsqrt)(r2), eta, deta;
        JN(mlp)(net->He, net->ew1, net->eb1, net->ew2, r, &eta, &deta);
        s = JN(jadd)(s, JN(jadd)(JN(jmul)(deta, r), JN(jscale)((double)d, eta)));
      }
    s = JN(jscale)(2.0, s);
    if (net->Hm > 0) {                                               /* _e_n_divergence (:78-81) */
      jet t = JN(jc)(0.0);
      for (int i = 0; i < n; i++) {
        jet r2 = JN(jc)(0.0);
        for (int c = 0; c < d; c++) r2 = JN(jadd)(r2, JN(jmul)(z[i * d + c], z[i * d + c]));
        jet r = JN(jsqrt)(r2), mu, dmu;
        JN(mlp)(net->Hm, net->mw1, net->mb1, net->mw2, r, &mu, &dmu);
        t = JN(jadd)(t, JN(jadd)(JN(jmul)(dmu, r), JN(jscale)((double)d, mu)));
      }
      s = JN(jadd)(s, t);
    }
    *div = s;
  }
}

/* flat-double RHS adaptors: the state handed to the RK45 driver is a flat double vector made of
 * jets laid out component-major: [v parts | d1 parts | d2 parts], each of length (n*d [+1]).     */
static void JN(unpack)(const double* y, int len, jet* out) {
  for (int i = 0; i < len; i++) out[i] = JN(jmk)(y[i], FFO_ORDER >= 1 ? y[len + i] : 0.0, FFO_ORDER >= 2 ? y[2 * len + i] : 0.0);
}
static void JN(pack)(const jet* in, int len, double* y) {
  for (int i = 0; i < len; i++) {
    y[i] = in[i].v;
#if FFO_ORDER >= 1
    y[len + i] = in[i].d1;
#endif
#if FFO_ORDER >= 2
    y[2 * len + i] = in[i].d2;
#endif
  }
}

/* CNF.F.forward (src/flow.py:34-36): d/dt (x, logp-accumulator) = (v(x), -div v(x)); one walker. */
static void JN(rhs_xlogp)(const ffo_net* net, int n, int d, const double* y, double* dy) {
  int M = n * d, len = M + 1;
  jet z[FFO_MAXM + 1], f[FFO_MAXM + 1];
  JN(unpack)(y, len, z);
  jet div;
  JN(backflow)(net, n, d, z, f, &div);
  f[M] = JN(jneg)(div);
  JN(pack)(f, len, dy);
}

#undef jet
#undef D1
#undef D2
