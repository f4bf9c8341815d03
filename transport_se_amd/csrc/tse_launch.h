// tse_launch.h -- from the run-time options of a context to the kernel instantiation that serves them.
//
// limiter_option and vert_remap_q_alg are fields of tse_ctx, the kernels take them as template parameters (LIM and LOPT of k_advance,
// LIM of k_lap1; NT, ALG2 and FUSED of k_remap).  The mapping from the one to the other is written here once: a new limiter is one
// more row of with_limiter, a new remap variant one more row of with_remap.  The kernels that work on a resident host's own arrays take the
// path of the view and whether a lane moves 16 bytes as <PATH, WIDE>: with_view_path.  Host code only: no kernel's signature or arguments change.
#pragma once
#include <type_traits>

#include "tse_kernels.h"

namespace tse {

// limiter_option -> <LIM, LOPT>, handed to f as two integral constants.  Unlimited keeps LOPT = 8, the default of the templates: there
// is one kernel without the limiter, not one per option.
template <class F>
inline void with_limiter(bool lim, int limiter_option, F&& f) {
  if (!lim) f(std::false_type{}, std::integral_constant<int, 8>{});
  else if (limiter_option == 9) f(std::true_type{}, std::integral_constant<int, 9>{});
  else f(std::true_type{}, std::integral_constant<int, 8>{});
}

// One launch of a stage's slab kernel (k_advance, k_lap1): where it runs, the kernel's own arguments in the kernel's order, and the two
// options that choose the instantiation.  k_lap1 takes dt (its rdt), Qn0, out, dp, divdp_proj, the bounds and ga of these.
struct StageArgs {
  hipStream_t stream; dim3 grid, block;
  int nelemd; Dvv_t D; GeoPtrs G; int qsize; double dt, nu_q;
  const double *Qn0, *lap; double* out;
  const double *vn0, *dp, *divdp, *divdp_proj;
  double *qmin, *qmax; const double* dp0;
  GatherArgs ga;
  bool lim; int limiter_option;
};

// Unlimited (LIM = false) means that no bounds are read or written: the kernel gets null pointers.
template <int RHS, int GIN, bool DB>
inline void launch_advance(const StageArgs& a) {
  with_limiter(a.lim, a.limiter_option, [&](auto lim, auto lopt) {
    constexpr bool LIM = decltype(lim)::value;
    hipLaunchKernelGGL((k_advance<RHS, GIN, DB, LIM, decltype(lopt)::value>), a.grid, a.block, 0, a.stream, a.nelemd, a.D, a.G, a.qsize, a.dt, a.nu_q,
                       a.Qn0, a.lap, a.out, a.vn0, a.dp, a.divdp, a.divdp_proj, LIM ? a.qmin : nullptr, LIM ? a.qmax : nullptr, a.dp0, a.ga);
  });
}
template <int GIN>
inline void launch_lap1(const StageArgs& a) {
  with_limiter(a.lim, a.limiter_option, [&](auto lim, auto) {
    constexpr bool LIM = decltype(lim)::value;
    hipLaunchKernelGGL((k_lap1<GIN, LIM>), a.grid, a.block, 0, a.stream, a.nelemd, a.D, a.G, a.qsize, a.dt, a.Qn0, a.out, a.dp, a.divdp_proj,
                       LIM ? a.qmin : nullptr, LIM ? a.qmax : nullptr, a.ga);
  });
}
// launch_advance<2, 3, true>, the stage-3 kernel: instantiated in tse_stage3.hip alone, which is built with another scheduler strategy
// (a second instantiation elsewhere would put the same kernels into two code objects, scheduled differently)
void launch_advance23(const StageArgs& a);

// (tracers per thread, vert_remap_q_alg == 2, final DSS assembled on read) -> f(k_remap instantiation, threads per block); returns what f
// returns.  The fused remap exists for one tracer per thread only: its callers refuse fused with nt != 1 before they come here.
template <class F>
inline int with_remap(int nt, bool alg2, bool fused, F&& f) {
  if (fused) return alg2 ? f(k_remap<1, true, true>, REMAP_THREADS) : f(k_remap<1, false, true>, REMAP_THREADS);
  if (nt == 1) return alg2 ? f(k_remap<1, true>, REMAP_THREADS) : f(k_remap<1, false>, REMAP_THREADS);
  return alg2 ? f(k_remap<2, true>, REMAP_THREADS / 2) : f(k_remap<2, false>, REMAP_THREADS / 2);
}
// every instantiation with_remap can hand out, once each; stops at the first f that does not return 0
template <class F>
inline int with_every_remap(F&& f) {
  for (int fused = 0; fused < 2; fused++)
    for (int nt = 1; nt <= (fused ? 1 : 2); nt++)
      for (int alg2 = 0; alg2 < 2; alg2++)
        if (int rc = with_remap(nt, alg2 != 0, fused != 0, f)) return rc;
  return 0;
}

// tse_remap_view: (vert_remap_q_alg == 2, the field is a layer mean, 16 bytes per lane) -> f(k_remap_view instantiation, bytes of dynamic
// LDS); returns what f returns.  A layer-mean field keeps its target thicknesses in LDS behind RemapLds.
constexpr size_t REMAP_VIEW_LDS = sizeof(RemapLds), REMAP_VIEW_LDS_MEAN = sizeof(RemapLds) + sizeof(double) * NLEV * 16;
static_assert(REMAP_VIEW_LDS_MEAN <= 160 * 1024, "RemapLds and the target thicknesses of a layer-mean field fit a CU's LDS");
template <class F>
inline int with_remap_view(bool alg2, bool mean, bool wide, F&& f) {
  if (mean) {
    if (alg2) return wide ? f(k_remap_view<true, true, true>, REMAP_VIEW_LDS_MEAN) : f(k_remap_view<true, true, false>, REMAP_VIEW_LDS_MEAN);
    return wide ? f(k_remap_view<false, true, true>, REMAP_VIEW_LDS_MEAN) : f(k_remap_view<false, true, false>, REMAP_VIEW_LDS_MEAN);
  }
  if (alg2) return wide ? f(k_remap_view<true, false, true>, REMAP_VIEW_LDS) : f(k_remap_view<true, false, false>, REMAP_VIEW_LDS);
  return wide ? f(k_remap_view<false, false, true>, REMAP_VIEW_LDS) : f(k_remap_view<false, false, false>, REMAP_VIEW_LDS);
}

// (path of a view's plan, view_wide of that path and view: tse_views.h) -> <PATH, WIDE>, handed to f as two integral constants: the five
// pairs (0, t) (0, f) (1, t) (1, f) (2, f).  The generic path moves one double per lane whatever `wide` says: <2, true> is never instantiated.
template <class F>
inline void with_view_path(int path, bool wide, F&& f) {
  const std::integral_constant<int, 0> p0{}; const std::integral_constant<int, 1> p1{}; const std::integral_constant<int, 2> p2{};
  const std::true_type w{}; const std::false_type n{};
  if (path == 0) { if (wide) f(p0, w); else f(p0, n); }
  else if (path == 1) { if (wide) f(p1, w); else f(p1, n); }
  else f(p2, n);
}

// tse_stats_view: (has a reference view, has a weight view) -> f(k_stats_view instantiation).  The paths of the views are no template
// parameters: each view's loader is chosen inside the kernel by stats_form.
template <class F>
inline void with_stats_view(bool ref, bool weight, F&& f) {
  if (ref) { if (weight) f(k_stats_view<true, true>); else f(k_stats_view<true, false>); }
  else { if (weight) f(k_stats_view<false, true>); else f(k_stats_view<false, false>); }
}
// (path of a view's plan, view_wide of that path and view) -> the loader of that view in k_stats_view; the generic loader also serves a
// point-fastest view that may not move 16 bytes per lane
inline int stats_form(int path, bool wide) {
  if (path == 1) return wide ? STATS_ROWS_WIDE : STATS_ROWS;
  return path == 0 && wide ? STATS_LINES_WIDE : STATS_POINTS;
}

// tse_column_view: (op, p is a view of the host's, path and view_wide of `out`) -> f(k_column_view instantiation).  The paths of the
// inputs are no template parameters (stats_form, as in k_stats_view).  PINT's out has NLEVP levels and never takes path 1 (dss_view_plan).
// Used by launch_column_view alone: the instantiations live in tse_column.hip, which says why.
template <class F>
inline void with_column_view(int op, bool pgiven, int path, bool wide, F&& f) {
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    constexpr bool W = decltype(wc)::value;
    if (op == COL_PINT) { if constexpr (PATH != 1) f(k_column_view<COL_PINT, false, PATH, W>); }
    else if (op == COL_PMID) f(k_column_view<COL_PMID, false, PATH, W>);
    else if (op == COL_PHI) { if (pgiven) f(k_column_view<COL_PHI, true, PATH, W>); else f(k_column_view<COL_PHI, false, PATH, W>); }
    else { if (pgiven) f(k_column_view<COL_OMEGA, true, PATH, W>); else f(k_column_view<COL_OMEGA, false, PATH, W>); }
  });
}
void launch_column_view(hipStream_t stream, int nelemd, int op, bool pgiven, int path, bool wide, const ColumnViewArgs& a, double* out);

}  // namespace tse
