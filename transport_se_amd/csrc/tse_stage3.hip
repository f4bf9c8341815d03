// tse_stage3.hip -- the stage-3 kernel k_advance<2,3> (tse_kernels.h) in a translation unit of its own, because it is built with
// another instruction scheduler than the rest of the library: -mllvm -amdgpu-sched-strategy=max-ilp.
//
// k_advance<2,3> is the one kernel that holds two waves per SIMD (224 registers) AND keeps the vector units busy for more than half of
// its run time (19 000 VALU instructions per wave): with so little to interleave, the latency of its dependent fp64 chains shows.
// LLVM's default AMDGPU strategy schedules for occupancy first; "max-ilp" orders for instruction-level parallelism inside the
// register budget the launch bounds allow: 22.55 -> 22.08 ms per launch on one box, interleaved runs, same bits
// (profiles/r03_ab_sched_strategy.txt).  The strategy is a per-module compiler option, and for the three-wave kernels it is a loss
// (k_advance<0,0> 142 -> 196 registers, 11.5 -> 12.2 ms; k_advance<1,1> 168 -> 204, 14.5 -> 15.4), hence this file.
#include "tse_launch.h"

namespace tse {

// k_advance<2,3,true> with the limiter the arguments ask for (tse_launch.h); unlimited: no bounds image, no dp_star, qmin/qmax not touched
void launch_advance23(const StageArgs& a) { launch_advance<2, 3, true>(a); }

}  // namespace tse
