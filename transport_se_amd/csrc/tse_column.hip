// tse_column.hip -- the instantiations of k_column_view (tse_view_kernels.h) in a translation unit of their own, so that the code of
// the other view kernels stays what it is.
//
// k_column_view shares its loaders and stores with the other view kernels: stats_load_image, dss_rows_to_tile, dss_tile_to_rows,
// lap_view_store_row.  The code of a view kernel depends on which kernels share its code object: instantiated beside the others, the
// column kernel changed the instructions of the 30 that call the same helpers (the instantiations of k_lap_view_stage,
// k_lap_view_out<., ., 2> and k_sphere_op_stage; tools/kernel_digest.py against the build before), and so did taking the tracer
// path's kernels away from them ("Two products, two code objects").  Folded into tse_views_api.hip it would move the same 30 again.
#include "tse_view_launch.h"

namespace tse {

// one block per element on `stream`; the instantiation is with_column_view's (tse_view_launch.h)
void launch_column_view(hipStream_t stream, int nelemd, int op, bool pgiven, int path, bool wide, const ColumnViewArgs& a, double* out) {
  with_column_view(op, pgiven, path, wide, [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)nelemd), dim3(VIEW_THREADS), 0, stream, a, out); });
}

}  // namespace tse
