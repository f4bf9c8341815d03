// tse_view_launch.h -- from the plan of a view to the instantiation of a view kernel (tse_view_kernels.h) that serves it: the
// selectors of tse_views_api.hip and tse_column.hip, in the idiom of tse_launch.h.  The kernels that work on a resident host's own arrays take the
// path of the view and whether a lane moves 16 bytes as <PATH, WIDE>: with_view_path.  Host code only.
#pragma once
#include <type_traits>

#include "tse_view_kernels.h"

namespace tse {

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
