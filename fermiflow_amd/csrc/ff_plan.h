// ff_plan.h -- which kernel serves a shape (n particles, d dimensions), and with what geometry: stated ONCE.  The forward dispatch
// (ff_cnf_fwd.hip, ff_wide.hip), the adjoint's and its workspace sizing (ff_cnf_adj.hip) and the query of the C ABI (ff_kernel_plan,
// ff_api.hip: read by fermiflow_amd/VMC.py and by the tests' batch sizing) all switch on the ff_plan these functions return.
// constexpr and free of run-time state: the environment knobs and ff_set_kernel_family reach it as ff_plan_knobs.
//
// Families.  Several walkers per wave ("narrow": n = 1..12 in d = 2, n = 2..4 in d = 3) or one walker per workgroup ("wide":
// n <= 24 with n d <= 60, ff_wide.hip / ff_adj_wide.h).  The narrow local-energy pass has four kernels: the column sweep
// (ff_ode_fwd_kernel MODE 2), its two-lanes-per-direction variant (ff_eloc_split_kernel), the row layout (ff_eloc_rows.h) and the
// matrix-core kernel (ff_eloc_mfma.h).  Every call is a table kernel and, behind it, its off-table fallback (`fallback`).
#pragma once
#include <stdint.h>
#include "../../include/fermiflow.h"

#ifndef FF_WAVE
#define FF_WAVE 64
#endif
#define FF_WIDE_NMAX 24
#define FF_WIDE_MMAX 60

// --- the build's knobs (A/B builds set them with -D; the host simulator builds with FF_MFMA_FROM=99: no matrix cores there)
#ifndef FF_MFMA_FROM
#define FF_MFMA_FROM 4      // matrix-core local-energy kernel from this many particles (2-3 tie with the column sweep and keep it: DESIGN.md 3g)
#endif
#ifndef FF_MFMA_WPS
#define FF_MFMA_WPS 2       // waves per SIMD the matrix-core kernel is compiled for
#endif
#ifndef FF_ADJ_WPW
#define FF_ADJ_WPW 2        // waves per workgroup of the tabulated adjoint (1: the single-wave workgroups of rounds 1-3)
#endif
// Walkers per wave of the tabulated adjoint at 12 coordinates.  The forward kernels pack 64 / M walkers into a wave; here every lane
// also carries the six stage records of its radii, and at 6 particles (5 walkers x 21 radii = 105 radii: two per lane) that
// put the kernel at 360 registers.  With THREE walkers (63 radii: one per lane) it takes 292 and is exactly as fast
// (0.67 ms per 65 536 walkers either way: the radius phase is what a wave-evaluation waits for) -- and 292 + 164 <= 512:
// a wave of the Metropolis kernel now fits the same SIMD, so the next sweep's walkers are sampled BESIDE the adjoint
// (GSVMC prefetch, DESIGN.md 6: 1.11 -> 0.78 ms for the two together; tools/probes/overlap.py).
#ifndef FF_ADJ_G12
#define FF_ADJ_G12 3
#endif
// one walker per workgroup, both products on v_mfma_f64_16x16x4 (ff_wide.hip): measured faster than the row layout from 11 particles
// on (tools/probes/wide_c5.py; 16 384 walkers: 11 particles 2.12 against 2.68 ms, 12 particles 2.25 against 2.91; 10 particles 2.04 against 1.88)
#define FF_ELOC_WIDE_FROM 11
#define FF_GRID_CAP ((int64_t)1 << 20)      // without a work queue: one workgroup per walker group, up to this many
// behind a table kernel the direct column kernel is a fallback that almost always finds nothing to do: a grid-stride launch of at most
// this many workgroups instead of one per walker group (13 108 workgroups at config 2: 6 us just to start and retire them)
#define FF_FALLBACK_GRID_CAP 2048

// --- the shapes each family is instantiated for (X-macros: a launch needs N, D at compile time)
// narrow shapes X(N, D, SPLIT): flow and adjoint kernels take (N, D); SPLIT = lanes per row of the row-layout local-energy kernel,
// chosen so that a walker group fills the wave and the workgroup's LDS stays under 40 KB (four single-wave workgroups per CU)
#define FF_NARROW_SHAPES(X) \
  X(6, 2, 1) X(3, 2, 1) X(12, 2, 2) X(2, 2, 1) X(4, 2, 1) X(5, 2, 1) X(8, 2, 2) X(10, 2, 3) X(1, 2, 1) X(7, 2, 2) X(9, 2, 3) X(11, 2, 2) \
  X(2, 3, 1) X(3, 3, 1) X(4, 3, 1)
#define FF_ELOC_COLUMNS(X) X(6, 2) X(3, 2) X(2, 2) X(4, 2) X(5, 2)       // ff_ode_fwd_kernel<N, D, 2, .>: at most 12 coordinates
#define FF_ELOC_SPLIT(X) X(8, 2) X(10, 2) X(12, 2)                       // ff_eloc_split_kernel
#define FF_ELOC_MFMA(X) X(6, 2) X(2, 2) X(3, 2) X(4, 2) X(5, 2)          // ff_eloc_mfma_kernel
#define FF_SHAPE_IS(N_, D_, ...) || (n == N_ && d == D_)
#define FF_SHAPE_SPLIT(N_, D_, S_) + (n == N_ && d == D_ ? S_ : 0)
constexpr bool ff_narrow_shape(int n, int d) { return false FF_NARROW_SHAPES(FF_SHAPE_IS); }
constexpr int ff_rows_split(int n, int d) { return 0 FF_NARROW_SHAPES(FF_SHAPE_SPLIT); }      // 0: no row-layout kernel
constexpr bool ff_columns_shape(int n, int d) { return false FF_ELOC_COLUMNS(FF_SHAPE_IS); }
constexpr bool ff_split_shape(int n, int d) { return false FF_ELOC_SPLIT(FF_SHAPE_IS); }
constexpr bool ff_mfma_shape(int n, int d) { return false FF_ELOC_MFMA(FF_SHAPE_IS); }
#undef FF_SHAPE_IS
#undef FF_SHAPE_SPLIT
constexpr bool ff_wide_shape(int n, int d) { return (d == 2 || d == 3) && n >= 1 && n <= FF_WIDE_NMAX && n * d <= FF_WIDE_MMAX; }

// --- geometry
// walkers per wave of the narrow flow, column and direct-adjoint kernels (at most 16: the radius ids carry 4 bits of it); 0: a walker
// does not fit one wave
constexpr int ff_geom_G(int n, int d) {
  const int M = n * d;
  return M > 0 && M <= FF_WAVE ? (FF_WAVE / M > 16 ? 16 : FF_WAVE / M) : 0;
}
// ... of the row layout with `split` lanes per row (split = 2 on the column layout: ff_eloc_split_kernel)
constexpr int ff_rows_G(int n, int d, int split) { return ff_geom_G(n * split, d); }
// ... of the tabulated adjoint.  (4, 5, 7, 9, 10 and 11 particles -- round 6: with 64 / M walkers their 80-165 radii per wave took two
// or three record slots per lane, 144-556 B of scratch at two waves per SIMD where the allocator had no AGPRs left; as many walkers
// as keep the radii at one per lane -- at least one walker -- instead.  Measured: 8 and 12 particles are faster at 64 / M.)
constexpr int ff_adjtab_G(int n, int d, int g12 = FF_ADJ_G12) {
  const int M = n * d, g = ff_geom_G(n, d);
  if (g == 0) return 0;
  if (M == 12) return g12;
  if (d == 2 && (n == 4 || n == 5 || n == 7 || n == 9 || n == 10 || n == 11)) {
    const int gr = FF_WAVE / (n * (n + 1) / 2);
    return gr < 1 ? 1 : (gr < g ? gr : g);
  }
  return g;
}
// waves per workgroup of the wide local-energy kernel: the padded size 16 T >= n d + 4
constexpr int ff_wide_T(int n, int d) { return (n * d + 4 + 15) / 16; }

// --- the plan
struct ff_plan {
  int family;       // FF_FAMILY_* (include/fermiflow.h); FF_FAMILY_NONE: no kernel serves the shape
  int group;        // walkers a wave (narrow) or a workgroup (wide) takes at a time; for the local energy also the lockstep count
  int param;        // rows: SPLIT; wide local energy: T; matrix-core kernel: waves per SIMD; tabulated adjoint: waves per workgroup, each
                    // with walker groups of its own; 0: the family has none
  int per_cu;       // workgroups per compute unit of the persistent grid ...
  bool queue_only;  // ... which the launch takes only with a work queue (without: one workgroup per group)
  int64_t max_grid; // and never more workgroups than this
  constexpr int64_t wg_walkers() const { return family == FF_FAMILY_TABULATED ? (int64_t)group * param : group; }
  constexpr int64_t cap(int64_t cus, bool queue) const {
    const int64_t c = (queue || !queue_only) ? per_cu * cus : max_grid;
    return c < max_grid ? c : max_grid;
  }
};
enum { FF_ELOC_AUTO = 0, FF_ELOC_MFMA, FF_ELOC_ROWS, FF_ELOC_COLUMNS, FF_ELOC_WIDE };      // FF_ELOC_KERNEL in the environment
struct ff_plan_knobs {
  int eloc_kind = FF_ELOC_AUTO;
  bool wide_forced = false;      // FF_WIDE=1 / ff_set_kernel_family(1): the wide family for every shape (A/B and parity testing)
  int mfma_from = FF_MFMA_FROM, mfma_wps = FF_MFMA_WPS, adj_wpw = FF_ADJ_WPW, adj_g12 = FF_ADJ_G12;
};
constexpr ff_plan FF_NO_PLAN = {FF_FAMILY_NONE, 0, 0, 0, false, 0};
// four waves per CU = one per SIMD, behind a table kernel at most FF_FALLBACK_GRID_CAP workgroups
constexpr ff_plan ff_plan_columns(int family, int n, int d, bool fallback) {
  return {family, ff_geom_G(n, d), 0, 4, true, fallback ? FF_FALLBACK_GRID_CAP : FF_GRID_CAP};
}

// CNF.generate / CNF.delta_logp (MODE 0 / 1)
constexpr ff_plan ff_plan_flow(int n, int d, bool fallback, ff_plan_knobs k = {}) {
  if (ff_wide_shape(n, d) && (k.wide_forced || !ff_narrow_shape(n, d))) return {FF_FAMILY_WIDE, 1, 0, 64, false, INT64_MAX};
  return ff_narrow_shape(n, d) ? ff_plan_columns(FF_FAMILY_NARROW, n, d, fallback) : FF_NO_PLAN;
}

// Local-energy sensitivities (MODE 2).  Three narrow kernels compute them (tests/test_hostsim.py::test_three_local_energy_kernels_agree);
// FF_ELOC_KERNEL = auto (default) | mfma | rows | columns | wide forces one where it is instantiated.  auto takes the fastest measured
// on MI355X (tools/probes/eloc_ab.py): in d = 2 the row layout at 1, the column sweep at 2-3 particles, the matrix cores at 4-6, the
// row layout at 7, 9 and 10, the split column sweep at 8, the wide family from 11 on; in d = 3 the row layout at 2-4, wide elsewhere.
// A forced kind that is not instantiated at a shape falls through to the lines below it -- "rows" at 13 particles is the wide
// kernel, "mfma" at 10 the split sweep, "columns" at 7 the row layout: what the dispatch has always done there, kept as it is.
constexpr ff_plan ff_plan_eloc(int n, int d, bool fallback, ff_plan_knobs k = {}) {
  const bool is_auto = k.eloc_kind == FF_ELOC_AUTO;
  const ff_plan wide = {FF_FAMILY_WIDE, 1, ff_wide_T(n, d), ff_wide_T(n, d) >= 3 ? 1 : (ff_wide_T(n, d) == 2 ? 2 : 4), true, FF_GRID_CAP};
  // (persistent grid: as many workgroups as stay resident -- one per CU at T = 4)
  if (ff_wide_shape(n, d) && (k.wide_forced || (d == 2 && (k.eloc_kind == FF_ELOC_WIDE || (is_auto && n >= FF_ELOC_WIDE_FROM))))) return wide;
  if ((k.eloc_kind == FF_ELOC_MFMA || (is_auto && d == 2 && n >= k.mfma_from && n <= 6)) && ff_mfma_shape(n, d))
    return {FF_FAMILY_MFMA, 4, k.mfma_wps, fallback ? 4 : 4 * k.mfma_wps, true, FF_GRID_CAP};      // four walkers per wave, M = n d <= 12
  const bool rows_only = ff_narrow_shape(n, d) && !ff_columns_shape(n, d) && !ff_split_shape(n, d);
  if ((k.eloc_kind == FF_ELOC_ROWS || rows_only || (is_auto && n >= 9)) && ff_rows_split(n, d))
    return {FF_FAMILY_ROWS, ff_rows_G(n, d, ff_rows_split(n, d)), ff_rows_split(n, d), 4, true, FF_GRID_CAP};
  // n >= 8: the two-lanes-per-direction kernel (measured, 32768 walkers: n = 8 6.5 -> 4.5 ms, n = 10 48 -> 9.3 ms, n = 12 95 -> 14.7 ms)
  if (ff_split_shape(n, d)) return {FF_FAMILY_SPLIT, ff_rows_G(n, d, 2), 0, 4, true, FF_GRID_CAP};
  if (ff_columns_shape(n, d)) return ff_plan_columns(FF_FAMILY_COLUMNS, n, d, fallback);
  return ff_wide_shape(n, d) ? wide : FF_NO_PLAN;
}

// The adjoint: a persistent grid of one workgroup per SIMD with or without a work queue.  Every walker takes the same few steps here,
// so a static split is balanced, and each workgroup flushes a private deposit table (25 KB) at its end -- the fewer workgroups the
// less HBM traffic (measured, 65536 walkers: 4096 workgroups 1.09 ms, 1024 workgroups 0.92 ms).
constexpr ff_plan ff_plan_adjoint(int n, int d, bool fallback, ff_plan_knobs k = {}) {
  if (ff_wide_shape(n, d) && (k.wide_forced || !ff_narrow_shape(n, d))) return {FF_FAMILY_WIDE, 1, 0, 4, false, INT64_MAX};
  if (!ff_narrow_shape(n, d)) return FF_NO_PLAN;
  if (fallback) return {FF_FAMILY_DIRECT, ff_geom_G(n, d), 0, 4, false, INT64_MAX};
  return {FF_FAMILY_TABULATED, ff_adjtab_G(n, d, k.adj_g12), k.adj_wpw, 4, false, INT64_MAX};
}

// --- every plan names a kernel that exists, and every list entry is one some plan names
constexpr bool ff_plan_instantiated(ff_plan p, int n, int d) {
  switch (p.family) {
    case FF_FAMILY_NONE: return !ff_wide_shape(n, d) && !ff_narrow_shape(n, d);
    case FF_FAMILY_COLUMNS: return ff_columns_shape(n, d) && p.group == ff_geom_G(n, d);
    case FF_FAMILY_SPLIT: return ff_split_shape(n, d);
    case FF_FAMILY_ROWS: return ff_rows_split(n, d) == p.param && p.group >= 1;
    case FF_FAMILY_MFMA: return ff_mfma_shape(n, d);
    case FF_FAMILY_WIDE: return ff_wide_shape(n, d) && (p.param == 0 || (p.param >= 1 && p.param <= 4));
    default: return ff_narrow_shape(n, d) && p.group >= 1;      // narrow flow, tabulated and direct adjoint
  }
}
constexpr bool ff_plans_are_instantiated() {
  for (int d = 1; d <= 4; d++)
    for (int n = 0; n <= 33; n++)
      for (int fb = 0; fb < 2; fb++)
        for (int forced = 0; forced < 2; forced++) {
          ff_plan_knobs k;
          k.wide_forced = forced != 0;
          if (!ff_plan_instantiated(ff_plan_flow(n, d, fb, k), n, d) || !ff_plan_instantiated(ff_plan_adjoint(n, d, fb, k), n, d)) return false;
          for (int kind = FF_ELOC_AUTO; kind <= FF_ELOC_WIDE; kind++) {
            k.eloc_kind = kind;
            if (!ff_plan_instantiated(ff_plan_eloc(n, d, fb, k), n, d)) return false;
          }
        }
  return true;
}
constexpr bool ff_eloc_family_reachable(int family, int n, int d) {
  for (int kind = FF_ELOC_AUTO; kind <= FF_ELOC_WIDE; kind++) {
    ff_plan_knobs k;
    k.eloc_kind = kind;
    if (ff_plan_eloc(n, d, false, k).family == family) return true;
  }
  return false;
}
static_assert(ff_plans_are_instantiated(), "a plan names a kernel that is not in its family's list");
#define FF_REACH_ROWS(N_, D_, S_) static_assert(ff_eloc_family_reachable(FF_FAMILY_ROWS, N_, D_), "unreachable row-layout instantiation");
#define FF_REACH_COLUMNS(N_, D_) static_assert(ff_eloc_family_reachable(FF_FAMILY_COLUMNS, N_, D_), "unreachable column-sweep instantiation");
#define FF_REACH_SPLIT(N_, D_) static_assert(ff_eloc_family_reachable(FF_FAMILY_SPLIT, N_, D_), "unreachable split-sweep instantiation");
#define FF_REACH_MFMA(N_, D_) static_assert(ff_eloc_family_reachable(FF_FAMILY_MFMA, N_, D_), "unreachable matrix-core instantiation");
FF_NARROW_SHAPES(FF_REACH_ROWS) FF_ELOC_COLUMNS(FF_REACH_COLUMNS) FF_ELOC_SPLIT(FF_REACH_SPLIT) FF_ELOC_MFMA(FF_REACH_MFMA)
#undef FF_REACH_ROWS
#undef FF_REACH_COLUMNS
#undef FF_REACH_SPLIT
#undef FF_REACH_MFMA
