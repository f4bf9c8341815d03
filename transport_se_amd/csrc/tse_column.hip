// tse_column.hip -- the instantiations of k_column_view (tse_kernels.h) in a translation unit of their own, so that the code of every
// other kernel stays what it was.
//
// k_column_view shares its loaders and stores with the other view kernels: stats_load_image, dss_rows_to_tile, dss_tile_to_rows,
// lap_view_store_row.  Device functions are internal to a code object, and the interprocedural passes that run before inlining look at
// every caller of one: with k_column_view instantiated beside them in tse_api.hip, the 30 kernels that call the same helpers came out
// with other instructions (k_lap_view_stage<1, false> 73 -> 79 registers; tools/kernel_digest.py against the build before).  In a code
// object of its own the column kernel is the helpers' only caller here and no caller there.
#include "tse_launch.h"

namespace tse {

// one block per element on `stream`; the instantiation is with_column_view's (tse_launch.h)
void launch_column_view(hipStream_t stream, int nelemd, int op, bool pgiven, int path, bool wide, const ColumnViewArgs& a, double* out) {
  with_column_view(op, pgiven, path, wide, [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)nelemd), dim3(VIEW_THREADS), 0, stream, a, out); });
}

}  // namespace tse
