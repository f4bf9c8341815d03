// tse_remap_check.h -- the precondition of remap_Q_ppm's bracket search for ONE column, as one function for the host
// (check_remap_grids, tse_tables.cpp) and the device (k_remap_view_check, tse_view_kernels.h).  No HIP include: a host C++ unit
// compiles it as plain C++.  tse_tables.h says what is refused and why.
#pragma once

#if defined(__HIP__)   // compiled as HIP (the .hip units); a host C++ unit sees a plain inline function
#define TSE_HOST_DEVICE __host__ __device__
#else
#define TSE_HOST_DEVICE
#endif

namespace tse {

enum RemapGridCode {
  REMAP_GRID_OK = 0,
  REMAP_GRID_SRC = 1,       // a dp_src that is not a finite positive number
  REMAP_GRID_SRC_SUM = 2,   // sum(dp_src) not finite, or sum + 1 == sum
  REMAP_GRID_TGT = 3,       // a dp_tgt that is negative or not finite (mean: or zero)
  REMAP_GRID_TGT_SUM = 4,   // a partial sum of dp_tgt below the last level reaches sum(dp_src) + 1
};

struct RemapGridFault {
  int code = 0, level = 0;   // level counted from 0
  double value = 0.0;        // the offending thickness or sum
  double limit = 0.0;        // with has_limit: sum(dp_src) + 1
  int has_limit = 0;         // codes 2 (sum + 1 == sum) and 4
};

// false for NaN and +-inf.  By the exponent bits: the library is compiled with -fno-honor-nans, under which a floating-point
// comparison may be rewritten as if no NaN existed
TSE_HOST_DEVICE inline bool remap_finite(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, sizeof u);
  return ((u >> 52) & 0x7ffull) != 0x7ffull;
}

// One column: src[k * ss], tgt[k * st], k < nlev (a stride of 0 broadcasts one layer).  The serial sums of the kernel's phase 1a:
// pio(k+1) = pio(k) + src(k), pin(k+1) = pin(k) + tgt(k), both from 0.  mean: the field is a layer mean and is divided by tgt on
// write, so a zero target layer is refused as well.  Returns the code of the first offence in the order src levels, source sum,
// tgt levels; 0 and *f untouched for a column the search ends on.  Two loops of nlev trips, no search.
TSE_HOST_DEVICE inline int remap_column_check(const double* src, long long ss, const double* tgt, long long st, int nlev, bool mean, RemapGridFault* f) {
  double pio = 0.0;
  for (int k = 0; k < nlev; k++) {
    const double d = src[(long long)k * ss];
    if (!(d > 0.0) || !remap_finite(d)) { f->code = REMAP_GRID_SRC; f->level = k; f->value = d; return f->code; }
    pio = pio + d;
  }
  if (!remap_finite(pio)) { f->code = REMAP_GRID_SRC_SUM; f->level = nlev - 1; f->value = pio; return f->code; }
  const double end = pio + 1.0;   // pio(nlev+2)
  // the sentinel must lie above the column: the search of the LAST level compares pin(nlev+1) = pio(nlev+1) with it, and from
  // sum(dp1) = 2^53 on the + 1 is absorbed (pio(nlev+2) == pio(nlev+1)) and that search would not end either
  if (!(end > pio)) { f->code = REMAP_GRID_SRC_SUM; f->level = nlev - 1; f->value = pio; f->limit = end; f->has_limit = 1; return f->code; }
  double pin = 0.0;
  for (int k = 0; k < nlev; k++) {
    const double d = tgt[(long long)k * st];
    if (!(d >= 0.0) || !remap_finite(d) || (mean && d == 0.0)) { f->code = REMAP_GRID_TGT; f->level = k; f->value = d; return f->code; }
    pin = pin + d;
    if (k + 1 < nlev && !(pin < end)) { f->code = REMAP_GRID_TGT_SUM; f->level = k; f->value = pin; f->limit = end; f->has_limit = 1; return f->code; }
  }
  return REMAP_GRID_OK;
}

}  // namespace tse
