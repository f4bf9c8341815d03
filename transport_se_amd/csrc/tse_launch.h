// tse_launch.h -- from the run-time options of a context to the kernel instantiation that serves them.
//
// limiter_option and vert_remap_q_alg are fields of tse_ctx, the kernels take them as template parameters (LIM and LOPT of k_advance,
// LIM of k_lap1; NT, ALG2 and FUSED of k_remap).  The mapping from the one to the other is written here once: a new limiter is one
// more row of with_limiter, a new remap variant one more row of with_remap.  The selectors of the view kernels are tse_view_launch.h's:
// this header sees no view kernel.  Host code only: no kernel's signature or arguments change.
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

}  // namespace tse
