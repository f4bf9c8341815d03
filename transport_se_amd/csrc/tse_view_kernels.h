// tse_view_kernels.h -- the gfx950 kernels that work on a resident host's own arrays through strided views: view put / get, forcing,
// remap_view, dss_view, biharmonic_view, vlaplace_view, sphere_op_view, stats_view, column_view.  Memory-bound kernels of many
// instantiations, one family per entry.  Included by tse_views_api.hip and tse_column.hip (through tse_view_launch.h), never by
// tse_api.hip: a view kernel lives in their code objects and no kernel of the tracer path does (DESIGN.md says why).  tse_kernels.h
// comes along for the remap and DSS device functions the view kernels reuse; a template nobody instantiates costs nothing.
#pragma once
#include "../../include/transport_se_hip.h"   // (TSE_HYPERVIS_MAX_FIELDS)
#include "tse_kernels.h"

namespace tse {

// ---- strided device views (tse_view_put / tse_view_get): bit copies between a host's own device array and the library's dense one ----
// ext: extents of (element, q, level, j, i); lib / vs: the strides in doubles of the library's array and of the view (tse_views.h).
// PUT: view -> library, otherwise library -> view.  The host side has checked that every address of the view lies inside one allocation
// and, for a destination view, that no two index tuples share an address (tse_views.cpp).
struct ViewDims { int ext[5]; long long lib[5]; long long vs[5]; };
constexpr int VIEW_THREADS = 256;

// path 2, any strides: one address computation per entry
template <bool PUT>
__global__ __launch_bounds__(VIEW_THREADS) void k_view_generic(ViewDims d, double* __restrict__ lib, double* __restrict__ view) {
  const size_t t = (size_t)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (t >= (size_t)d.ext[0] * d.ext[1] * d.ext[2] * 16) return;
  const int i = (int)(t & 3), j = (int)((t >> 2) & 3);
  size_t r = t >> 4;
  const int k = (int)(r % d.ext[2]); r /= d.ext[2];
  const int q = (int)(r % d.ext[1]);
  const long long e = (long long)(r / d.ext[1]);
  const long long lo = e * d.lib[0] + q * d.lib[1] + k * d.lib[2] + j * 4 + i;
  const long long vo = e * d.vs[0] + q * d.vs[1] + k * d.vs[2] + j * d.vs[3] + i * d.vs[4];
  if (PUT) lib[lo] = view[vo]; else view[vo] = lib[lo];
}

// path 0, point-fastest (stride i = 1, j = 4): every (element, q, level) slab is one 128-byte line on both sides.  W = 2: 16 bytes per lane
// (view base 16-byte aligned, even element / q / level strides), W = 1: 8 bytes per lane.
template <bool PUT, int W>
__global__ __launch_bounds__(VIEW_THREADS) void k_view_lines(ViewDims d, double* __restrict__ lib, double* __restrict__ view) {
  constexpr int PARTS = 16 / W;
  const size_t t = (size_t)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (t >= (size_t)d.ext[0] * d.ext[1] * d.ext[2] * PARTS) return;
  const int part = (int)(t % PARTS);
  size_t r = t / PARTS;
  const int k = (int)(r % d.ext[2]); r /= d.ext[2];
  const int q = (int)(r % d.ext[1]);
  const long long e = (long long)(r / d.ext[1]);
  double* L = lib + e * d.lib[0] + q * d.lib[1] + k * d.lib[2] + part * W;
  double* V = view + e * d.vs[0] + q * d.vs[1] + k * d.vs[2] + part * W;
  if (W == 2) { if (PUT) *(double2*)L = *(const double2*)V; else *(double2*)V = *(const double2*)L; }
  else { if (PUT) *L = *V; else *V = *L; }
}

// path 1, level-fastest (stride level = 1, i = S, j = 4S, S >= K): the view holds, per (element, q), 16 rows of K consecutive levels at
// pitch S; the library holds K lines of its 16 points at pitch lib_k (16; vn0, [k][c][p]: 32 -- a component is a tile of its own).  One
// block moves one tile: it reads the source with whole-line accesses (along the levels of the view's rows, or the library's 128-byte
// lines), passes it through an LDS image tile[p][k] and writes whole lines on the other side.
// The image's row pitch is VIEW_PITCH = NLEV + 2 doubles: even, so that a level pair of the view side is 16-byte aligned in the image and
// moves as one conflict-free ds_read_b128 / ds_write_b128 per lane, and NOT a multiple of 8.  The library side touches the image 16 bytes
// of points per lane, the two doubles at (2h) * PITCH + k and (2h + 1) * PITCH + k with h = lane % 8, k = lane / 8 + const (the compiler
// pairs them into one ds_read2_b64 / ds_write2_b64: 16-lane groups over 32 four-byte banks, i.e. 16 eight-byte ones).  With a pitch of
// K = 72 all eight h of a group would sit on the same bank (2 * 72 = 0 mod 16): 8-way.  With 2 * PITCH = 4 (mod 8) (NLEV is a multiple of
// 8) they spread over four banks, the two k of the group over the neighbours: 2-way.  An odd pitch would make that side conflict-free and
// give the conflict to the view side instead (no 16-byte LDS access; pairs of consecutive doubles at stride 2).  Either way the LDS work of
// a tile is a few hundred cycles against the ~2000 its 2 x 9 KB take at a CU's share of the HBM rate: the 2-way side is left as it is.
// WIDE: 16 bytes per lane on the view side too (view base 16-byte aligned, S and the element and q strides even); otherwise the view side
// moves 8 bytes per lane -- a row of 73 levels at an odd pitch cannot be 16-byte aligned.
constexpr int VIEW_PITCH = NLEV + 2;
// An empty statement that uses the loaded value where it stands: without it the compiler sinks each load of a lane next to the (guarded)
// image store that consumes it and the lane waits for its loads one after the other.
__device__ __forceinline__ void view_keep(double& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void view_keep(double2& x) { asm volatile("" : "+v"(x.x), "+v"(x.y)); }
static_assert(VIEW_PITCH >= NLEVP && VIEW_PITCH % 4 == 2, "rows of up to NLEVP levels; an even pitch with 2 * pitch = 4 (mod 8)");
template <bool PUT, bool WIDE, int K>
__global__ __launch_bounds__(VIEW_THREADS) void k_view_levels(int nq, long long lib_e, long long lib_q, long long lib_k, long long vs_e, long long vs_q,
                                                              long long S, double* __restrict__ lib, double* __restrict__ view) {
  __shared__ __attribute__((aligned(16))) double tile[16 * VIEW_PITCH];
  const int q = (int)(blockIdx.x % (unsigned)nq);
  const long long e = (long long)(blockIdx.x / (unsigned)nq);
  double* L = lib + e * lib_e + q * lib_q;
  double* V = view + e * vs_e + q * vs_q;
  const int tid = threadIdx.x;
  constexpr int KP = K / 2;   // whole level pairs of a row; an odd K leaves the last level to 16 lanes
  // Every lane issues all its global loads before it touches the image, so that a wave has its whole share of the tile in flight at once.
  constexpr int NV = WIDE ? (16 * KP + VIEW_THREADS - 1) / VIEW_THREADS : (16 * K + VIEW_THREADS - 1) / VIEW_THREADS;
  constexpr int NL = (8 * K + VIEW_THREADS - 1) / VIEW_THREADS;
  auto view_side = [&]() {   // PUT: view -> image, else image -> view
    constexpr bool load = PUT;
    if (WIDE) {
      double2 r[NV];
      double tail = 0;
      const bool has_tail = (K & 1) && tid < 16;
      if (load) {
#pragma unroll
        for (int u = 0; u < NV; u++) { const int it = min(u * VIEW_THREADS + tid, 16 * KP - 1); r[u] = *(const double2*)(V + (it / KP) * S + 2 * (it % KP)); }   // (a lane past the end reloads the last item)
        if (has_tail) tail = V[tid * S + K - 1];
#pragma unroll
        for (int u = 0; u < NV; u++) view_keep(r[u]);
      }
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int it = u * VIEW_THREADS + tid;
        if (it < 16 * KP) {
          double2* s = (double2*)(tile + (it / KP) * VIEW_PITCH + 2 * (it % KP));
          if (load) *s = r[u]; else *(double2*)(V + (it / KP) * S + 2 * (it % KP)) = *s;
        }
      }
      if (has_tail) { if (load) tile[tid * VIEW_PITCH + K - 1] = tail; else V[tid * S + K - 1] = tile[tid * VIEW_PITCH + K - 1]; }
    } else {
      double r[NV];
      if (load) {
#pragma unroll
        for (int u = 0; u < NV; u++) { const int it = min(u * VIEW_THREADS + tid, 16 * K - 1); r[u] = V[(it / K) * S + it % K]; }
#pragma unroll
        for (int u = 0; u < NV; u++) view_keep(r[u]);
      }
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int it = u * VIEW_THREADS + tid;
        if (it < 16 * K) { if (load) tile[(it / K) * VIEW_PITCH + it % K] = r[u]; else V[(it / K) * S + it % K] = tile[(it / K) * VIEW_PITCH + it % K]; }
      }
    }
  };
  auto lib_side = [&]() {    // PUT: image -> library, else library -> image
    constexpr bool load = !PUT;
    double2 r[NL];
    if (load) {
#pragma unroll
      for (int u = 0; u < NL; u++) { const int it = min(u * VIEW_THREADS + tid, 8 * K - 1); r[u] = *(const double2*)(L + (it >> 3) * lib_k + 2 * (it & 7)); }
#pragma unroll
      for (int u = 0; u < NL; u++) view_keep(r[u]);
    }
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int it = u * VIEW_THREADS + tid;
      if (it < 8 * K) {
        double* s = tile + 2 * (it & 7) * VIEW_PITCH + (it >> 3);
        if (load) { s[0] = r[u].x; s[VIEW_PITCH] = r[u].y; }
        else *(double2*)(L + (it >> 3) * lib_k + 2 * (it & 7)) = make_double2(s[0], s[VIEW_PITCH]);
      }
    }
  };
  if (PUT) { view_side(); __syncthreads(); lib_side(); }
  else { lib_side(); __syncthreads(); view_side(); }
}

// ---- tracer forcing (tse_apply_forcing): Qdp(nt) += the host's source term FQ, read through a strided view, never below zero ----
// The rule of E3SM's applyCAMforcing_tracers for one value, these operations in this order, none contracted (tests/forcing_model.py
// restates it in numpy):
//   MODE 0 (tendency)  v = dt * FQ
//   MODE 1 (adjust)    dpk = level_dp(k, ps_v);  Q = Qdp / dpk;  v = dpk * (FQ - Q)      (FQ is the new mixing ratio; a true division)
//   asked = v;  if (Qdp + v < 0 && v < 0) v = (Qdp < 0) ? 0.0 : -Qdp;  Qdp = Qdp + v
// so a tracer mass is never made negative and one that is negative already (a limiter-sized undershoot) is left alone.
// applied = v, withheld = asked - v (bit-zero where nothing was clipped).
template <int MODE>
__device__ __forceinline__ void forcing_rule(double dt, double dpk, double fq, double& qdp, double& applied, double& withheld) {
#pragma clang fp contract(off)
  double v;
  if (MODE == 0) v = dt * fq;
  else { const double Q = mixing_ratio(qdp, dpk); v = dpk * (fq - Q); }
  const double asked = v;
  if (qdp + v < 0.0 && v < 0.0) v = (qdp < 0.0) ? 0.0 : -qdp;
  applied = v;
  withheld = asked - v;
  qdp = qdp + v;
}

// One block per (element, tracer) tile of NLEV x 16 values, the shape of k_view_levels.  A lane owns FORCING_NL items (level k = item / 8,
// point pair 2h = 2 * (item % 8)): the Qdp side is read and written in place in whole 128-byte lines, 16 bytes per lane.  The FQ side has one
// loader per path of tse_view_plan("qdp"):
//   PATH 0  point-fastest: the view's own 128-byte lines, 16 bytes per lane (WIDE: view base 16-byte aligned, even element / q / level
//           strides) or two 8-byte loads;
//   PATH 1  level-fastest: the rows of consecutive levels go through the LDS image tile[p][VIEW_PITCH] as in k_view_levels<true> (WIDE as
//           there), the only barrier of the kernel without a budget;
//   PATH 2  any strides: two address computations per lane and item.
// Every lane issues all its global loads -- Qdp, FQ, ps_v, spheremp -- before the first use of any of them.
// BUDGET: out[(e * nq + q) * 2 + {0, 1}] = sum spheremp[p] * applied, sum spheremp[p] * withheld over the tile, every term formed without
// contraction and added in THE ORDER of k_norm_partials (lane (p, g) adds the levels of group g ascending; column p = ((s0 + s1) + s2) + s3;
// then the points 0..15 ascending, all sixteen), so a share is a function of the element's own data alone.  The terms pass through LDS;
// without BUDGET there is neither that work nor its two barriers.
constexpr int FORCING_NL = (8 * NLEV + VIEW_THREADS - 1) / VIEW_THREADS;
template <int MODE, int PATH, bool WIDE, bool BUDGET>
__global__ __launch_bounds__(VIEW_THREADS) void k_forcing(int nq, long long vs_e, long long vs_q, long long vs_k, long long vs_j, long long vs_i, double dt,
                                                          const double* __restrict__ ps_v, const double* __restrict__ hyai, const double* __restrict__ hybi, double ps0,
                                                          const double* __restrict__ spheremp, double* __restrict__ Qdp, const double* __restrict__ view,
                                                          double* __restrict__ budget) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double tile[PATH == 1 ? 16 * VIEW_PITCH : 2];
  __shared__ __attribute__((aligned(16))) double term[BUDGET ? 2 * NLEV * 16 : 2];
  __shared__ double part[BUDGET ? 2 * NORM_THREADS : 2];
  const int q = (int)(blockIdx.x % (unsigned)nq);
  const long long e = (long long)(blockIdx.x / (unsigned)nq);
  double* L = Qdp + ((size_t)e * nq + q) * NLEV * 16;
  const double* V = view + e * vs_e + q * vs_q;
  const int tid = threadIdx.x, h = tid & 7;
  constexpr int K = NLEV, KP = K / 2, NL = FORCING_NL;
  double2 x[NL], f[NL];
  double2 ps = make_double2(0.0, 0.0), w = make_double2(0.0, 0.0);
#pragma unroll
  for (int u = 0; u < NL; u++) { const int it = min(u * VIEW_THREADS + tid, 8 * K - 1); x[u] = *(const double2*)(L + (it >> 3) * 16 + 2 * (it & 7)); }   // (a lane past the end reloads the last item)
  if (MODE == 1) ps = *(const double2*)(ps_v + (size_t)e * 16 + 2 * h);
  if (BUDGET) w = *(const double2*)(spheremp + (size_t)e * 16 + 2 * h);
  if (PATH == 0) {
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int it = min(u * VIEW_THREADS + tid, 8 * K - 1);
      const double* s = V + (it >> 3) * vs_k + 2 * h;
      if (WIDE) f[u] = *(const double2*)s; else f[u] = make_double2(s[0], s[1]);
    }
  } else if (PATH == 2) {
    const long long o = (h >> 1) * vs_j + 2 * (h & 1) * vs_i;
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int it = min(u * VIEW_THREADS + tid, 8 * K - 1);
      const double* s = V + (it >> 3) * vs_k + o;
      f[u] = make_double2(s[0], s[vs_i]);
    }
  } else {
    const long long S = vs_i;
    if (WIDE) {
      constexpr int NV = (16 * KP + VIEW_THREADS - 1) / VIEW_THREADS;
      double2 r[NV];
#pragma unroll
      for (int u = 0; u < NV; u++) { const int it = min(u * VIEW_THREADS + tid, 16 * KP - 1); r[u] = *(const double2*)(V + (it / KP) * S + 2 * (it % KP)); }
#pragma unroll
      for (int u = 0; u < NV; u++) view_keep(r[u]);
#pragma unroll
      for (int u = 0; u < NL; u++) view_keep(x[u]);
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int it = u * VIEW_THREADS + tid;
        if (it < 16 * KP) *(double2*)(tile + (it / KP) * VIEW_PITCH + 2 * (it % KP)) = r[u];
      }
    } else {
      constexpr int NV = (16 * K + VIEW_THREADS - 1) / VIEW_THREADS;
      double r[NV];
#pragma unroll
      for (int u = 0; u < NV; u++) { const int it = min(u * VIEW_THREADS + tid, 16 * K - 1); r[u] = V[(it / K) * S + it % K]; }
#pragma unroll
      for (int u = 0; u < NV; u++) view_keep(r[u]);
#pragma unroll
      for (int u = 0; u < NL; u++) view_keep(x[u]);
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int it = u * VIEW_THREADS + tid;
        if (it < 16 * K) tile[(it / K) * VIEW_PITCH + it % K] = r[u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int it = min(u * VIEW_THREADS + tid, 8 * K - 1);
      const double* s = tile + 2 * h * VIEW_PITCH + (it >> 3);
      f[u] = make_double2(s[0], s[VIEW_PITCH]);
    }
  }
  if (PATH != 1) {
#pragma unroll
    for (int u = 0; u < NL; u++) { view_keep(x[u]); view_keep(f[u]); }
  }
#pragma unroll
  for (int u = 0; u < NL; u++) {
    const int it = u * VIEW_THREADS + tid;
    if (it < 8 * K) {
      const int k = it >> 3;
      double dx = 0.0, dy = 0.0;
      if (MODE == 1) { dx = level_dp(hyai, hybi, ps0, k, ps.x); dy = level_dp(hyai, hybi, ps0, k, ps.y); }
      double2 y = x[u], a, r;
      forcing_rule<MODE>(dt, dx, f[u].x, y.x, a.x, r.x);
      forcing_rule<MODE>(dt, dy, f[u].y, y.y, a.y, r.y);
      *(double2*)(L + k * 16 + 2 * h) = y;
      if (BUDGET) {
        *(double2*)(term + k * 16 + 2 * h) = make_double2(w.x * a.x, w.y * a.y);
        *(double2*)(term + (K + k) * 16 + 2 * h) = make_double2(w.x * r.x, w.y * r.y);
      }
    }
  }
  if (BUDGET) {
    __syncthreads();
    if (tid < NORM_THREADS) {
      const int p = tid & 15, g = tid >> 4;
      double s0 = 0.0, s1 = 0.0;
      for (int k = g * NORM_LPG; k < (g + 1) * NORM_LPG; k++) { s0 = s0 + term[k * 16 + p]; s1 = s1 + term[(K + k) * 16 + p]; }
      part[tid] = s0; part[NORM_THREADS + tid] = s1;
    }
    __syncthreads();
    if (tid < 2) {
      const double* v = part + tid * NORM_THREADS;
      double a = 0.0;
      for (int i = 0; i < 16; i++) a = a + (((v[i] + v[16 + i]) + v[32 + i]) + v[48 + i]);
      budget[((size_t)e * nq + q) * 2 + tid] = a;
    }
  }
}

// ---- remap of a host's own level fields through strided views (tse_remap_view) ---------------------------------------------------
// remap_Q_ppm(field, np, nf, dp_src, dp_tgt) for every element, in place in the host's own device array, on the host's own two grids.
// All three arrays are strided views (strides in doubles for element, q, level, j, i; the two grids have no q axis).  Nothing of the
// library's state is read or written.
struct RemapViewArgs {
  double* field;
  const double *src, *tgt;
  long long fs[5], ss[5], ts[5];
  int spath, tpath;   // path of tse_view_plan of the two grids (1: a block reads along the levels of a row)
};
constexpr int REMAP_STATUS = 4;   // ints per element of the status array: code (RemapGridCode), column, level, whether detail holds a limit

// The precondition of the bracket search, decided on the device (the grids of a resident host never reach the host): block = element,
// lane p < 16 runs remap_column_check (tse_remap_check.h: two loops of NLEV trips, no search) on column p, lane 0 takes the lowest
// column that offends -- check_remap_grids' order -- and writes status[e] = {code, column, level, has_limit} and detail[e] = {value, limit}.
// acc (null: a call that reports on return): acc[0] += 1 per refused element, acc[1] = min over them of
// seq << 40 | e << 16 | column << 12 | level << 4 | code, i.e. the lowest element of the earliest call (seq) not read yet.
constexpr int REMAP_CHECK_THREADS = 64;
template <int = 0>   // (a template: the header is included by two translation units)
__global__ __launch_bounds__(REMAP_CHECK_THREADS) void k_remap_view_check(RemapViewArgs a, int mean, int* __restrict__ status, double* __restrict__ detail,
                                                                          unsigned long long* __restrict__ acc, unsigned seq) {
  __shared__ int code[16], lev[16], hasl[16];
  __shared__ double val[16], lim[16];
  const long long e = blockIdx.x;
  const int p = threadIdx.x;
  if (p < 16) {
    RemapGridFault f;
    remap_column_check(a.src + e * a.ss[0] + (p >> 2) * a.ss[3] + (p & 3) * a.ss[4], a.ss[2],
                       a.tgt + e * a.ts[0] + (p >> 2) * a.ts[3] + (p & 3) * a.ts[4], a.ts[2], NLEV, mean != 0, &f);
    code[p] = f.code; lev[p] = f.level; hasl[p] = f.has_limit; val[p] = f.value; lim[p] = f.limit;
  }
  __syncthreads();
  if (p == 0) {
    int c = 0;
    while (c < 15 && code[c] == 0) c++;
    int* st = status + e * REMAP_STATUS;
    st[0] = code[c]; st[1] = code[c] ? c : 0; st[2] = code[c] ? lev[c] : 0; st[3] = code[c] ? hasl[c] : 0;
    detail[e * 2] = val[c]; detail[e * 2 + 1] = lim[c];
    if (code[c] && acc) {
      atomicAdd(acc, 1ull);
      atomicMin(acc + 1, (unsigned long long)seq << 40 | (unsigned long long)e << 16 | (unsigned long long)c << 12 | (unsigned long long)lev[c] << 4 |
                             (unsigned long long)code[c]);
    }
  }
}

// The column loop of remap_columns_generic (any kid(k) >= k - 1; the same operations in the same order: the same bits) on a column that
// is addressed through the view: col = the column's first level, sk = its level stride.  Thread = (field slot f, point p).
//   point-fastest view  the 16 lanes of a slot read one 128-byte line per level (sk = the level stride);
//   level-fastest view  a lane walks along its own row; WIDE (view base 16-byte aligned; even element, q and point strides): the CL = 4
//                       levels of a chunk are two 16-byte loads and, on the way back, two 16-byte stores; otherwise 8 bytes per level;
//   any other strides   one address per entry (the same code as point-fastest: only the strides differ).
// Loads run REMAP_PF levels ahead (WIDE: four to eight), as in the generic loop; a cell is stored after it has been consumed (kid(k) >=
// k - 1: by level k the window has taken cell k + 1), so the field is remapped in place.
// MEAN: the field holds layer means a.  m = a * dp_src as the cell is consumed (one product; S.dsel holds dp_src), the mass arithmetic
// unchanged, a' = m' / dp_tgt (a true division; dpt holds dp_tgt) as it is stored.
#pragma clang fp contract(off)
template <bool ALG2, bool MEAN, bool WIDE>
__device__ __forceinline__ void remap_columns_view(const RemapLds& S, const double (*__restrict__ dpt)[16], double* __restrict__ col, long long sk, int p) {
  int R = 0;                                   // highest cell consumed so far (ghost cells continue past NLEV)
  double pf[REMAP_PF];
  if (WIDE) {
#pragma unroll
    for (int t = 0; t < REMAP_PF; t += 2) { const double2 v = *reinterpret_cast<const double2*>(col + t); pf[t] = v.x; pf[t + 1] = v.y; }
  } else {
#pragma unroll
    for (int t = 0; t < REMAP_PF; t++) pf[t] = col[t * sk];
  }
  double pm1 = 0, pa1 = 0, pm2 = 0, pa2 = 0;   // the last two real cells (mass, mean) for the bottom mirror
#define TSE_READ_NEXT(m_, a_)                                                                          \
  do {                                                                                                 \
    R++;                                                                                               \
    if (R <= NLEV) {                                                                                   \
      m_ = MEAN ? pf[0] * S.dsel[R + 1][p] : pf[0];                                                    \
      _Pragma("unroll") for (int t = 0; t + 1 < REMAP_PF; t++) pf[t] = pf[t + 1];                      \
      if (WIDE) {                                                                                      \
        if ((R & (CL - 1)) == 0 && R + REMAP_PF <= NLEV) { /* cells R+5 .. R+8: the FIFO's upper half */ \
          const double2 v0 = *reinterpret_cast<const double2*>(col + R + CL);                          \
          const double2 v1 = *reinterpret_cast<const double2*>(col + R + CL + 2);                      \
          pf[CL] = v0.x; pf[CL + 1] = v0.y; pf[CL + 2] = v1.x; pf[CL + 3] = v1.y;                      \
        }                                                                                              \
      } else if (R + REMAP_PF <= NLEV) pf[REMAP_PF - 1] = col[(long long)(R + REMAP_PF - 1) * sk];     \
      a_ = m_ * S.rdpo[R + 1][p];                                                                      \
      pm2 = pm1; pa2 = pa1; pm1 = m_; pa1 = a_;                                                        \
    } else if (R == NLEV + 1) { m_ = pm1; a_ = pa1; } /* a(nlev+1) = a(nlev)   */                      \
    else { m_ = pm2; a_ = pa2; }                      /* a(nlev+2) = a(nlev-1) */                      \
  } while (0)
  double m1, a1, m2, a2, m3, a3;
  TSE_READ_NEXT(m1, a1); TSE_READ_NEXT(m2, a2); TSE_READ_NEXT(m3, a3);
  int kk = 1;
  double am2 = a2, am1 = a1, a0 = a1, ap1 = a2, ap2 = a3;  // a(-1)=a(2), a(0)=a(1)
  double m0 = m1, mp1 = m2, mp2 = m3;
  double dma_m1 = remap_dma_at(S, 0, p, am2, am1, a0), dma_0 = remap_dma_at(S, 1, p, am1, a0, ap1), dma_p1 = remap_dma_at(S, 2, p, a0, ap1, ap2);
  double ai_m1 = remap_ai_at(S, 0, p, am1, a0, dma_0, dma_m1), ai_0 = remap_ai_at(S, 1, p, a0, ap1, dma_p1, dma_0);
  double masso_kk = 0.0, massn1 = 0.0;
  double c0, c1, c2;
  remap_coefs(ai_m1, ai_0, a0, c0, c1, c2);
  ppm_alg2<ALG2>(kk, a0, c0, c1, c2);
  static_assert(REMAP_PF == 2 * CL && NLEV % CL == 0, "WIDE: the FIFO is two chunks of CL levels, a column whole chunks");
  for (int k0 = 1; k0 <= NLEV; k0 += CL) {
    double out[CL];
#pragma unroll
    for (int i = 0; i < CL; i++) {
      const int k = k0 + i;
      const int kt = S.kid[k - 1][p];   // <= NLEV: the window advances by at most NLEV - 1 cells per column
      while (kk < kt) {
        masso_kk = masso_kk + m0;
        am2 = am1; am1 = a0; a0 = ap1; ap1 = ap2; m0 = mp1; mp1 = mp2;
        TSE_READ_NEXT(mp2, ap2);
        kk++;
        dma_m1 = dma_0; dma_0 = dma_p1; dma_p1 = remap_dma_at(S, kk + 1, p, a0, ap1, ap2);
        ai_m1 = ai_0; ai_0 = remap_ai_at(S, kk, p, a0, ap1, dma_p1, dma_0);
        remap_coefs(ai_m1, ai_0, a0, c0, c1, c2);
        ppm_alg2<ALG2>(kk, a0, c0, c1, c2);
      }
      double z1, zz2, z3;
      ppm_zterms(S.z2[k - 1][p], z1, zz2, z3);
      const double massn2 = fma(ppm_integ(c0, c1, c2, z1, zz2, z3), S.dsel[kk + 1][p] /* = dpo(kk) */, masso_kk);
      const double qnew = massn2 - massn1;
      massn1 = massn2;
      out[i] = MEAN ? qnew / dpt[k - 1][p] : qnew;
      if (!WIDE) col[(long long)(k - 1) * sk] = out[i];
    }
    if (WIDE) {
      *reinterpret_cast<double2*>(col + k0 - 1) = make_double2(out[0], out[1]);
      *reinterpret_cast<double2*>(col + k0 + 1) = make_double2(out[2], out[3]);
    }
  }
#undef TSE_READ_NEXT
}
#pragma clang fp contract(fast)

// One block per element, RemapLds as in k_remap: phase 1a (thicknesses through the views, the serial interface sums on 16 lanes), the
// bracket search, phase 1b (remap_grid_coefs), then remap_columns_view on every (field slot, point).  No bounds, no dp3d / ps_v / bad, no
// DSS on read.  An element the check kernel refused (status) is left by the WHOLE block before the first barrier and before any search:
// its field keeps every bit.  The search is bounded besides: pio has NLEV + 2 rows.
// Dynamic LDS: RemapLds, and for MEAN behind it dpt[NLEV][16], the target thicknesses the new masses are divided by.
template <bool ALG2, bool MEAN, bool WIDE>
__global__ __launch_bounds__(REMAP_THREADS) void k_remap_view(int nf, RemapViewArgs a, const int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  RemapLds& S = *reinterpret_cast<RemapLds*>(smem_raw);
  double (*const dpt)[16] = reinterpret_cast<double (*)[16]>(smem_raw + sizeof(RemapLds));   // MEAN only
  const long long e = blockIdx.x;
  if (status[e * REMAP_STATUS] != 0) return;   // (uniform over the block)
  const int tid = threadIdx.x, nthreads = blockDim.x;
  double (*const pio)[16] = S.pio();
  double (*const dpo)[16] = S.dsel;
  double (*const tgt)[16] = S.rdpo;   // phase 1a parks dp_tgt (index k) where phase 1b puts 1/dpo
  // ---- phase 1a: the two grids through their views; a level-fastest view is read along its rows
  for (int w = tid; w < NLEV * 16; w += nthreads) {
    const int ks = a.spath == 1 ? w % NLEV : w >> 4, ps = a.spath == 1 ? w / NLEV : w & 15;
    dpo[ks + 2][ps] = a.src[e * a.ss[0] + ks * a.ss[2] + (ps >> 2) * a.ss[3] + (ps & 3) * a.ss[4]];
    const int kt = a.tpath == 1 ? w % NLEV : w >> 4, pt = a.tpath == 1 ? w / NLEV : w & 15;
    const double d = a.tgt[e * a.ts[0] + kt * a.ts[2] + (pt >> 2) * a.ts[3] + (pt & 3) * a.ts[4]];
    tgt[kt][pt] = d;
    if (MEAN) dpt[kt][pt] = d;
  }
  __syncthreads();
  if (tid < 16) {   // the serial sums of k_remap's phase 1a (their roundings are part of the result)
    const int p = tid;
    double run = 0.0;
    pio[0][p] = 0.0;
    for (int k = 0; k < NLEV; k++) { run = run + dpo[k + 2][p]; pio[k + 1][p] = run; }
    const double pio_prev = run;
    pio[NLEV + 1][p] = pio_prev + 1.;
    for (int k = 1; k <= 2; k++) { dpo[2 - k][p] = dpo[k + 1][p]; dpo[NLEV + k + 1][p] = dpo[NLEV + 2 - k][p]; }
    double pin = 0.0;
    for (int k = 1; k <= NLEV; k++) {
      pin = pin + tgt[k - 1][p];
      S.z2[k - 1][p] = (k == NLEV) ? pio_prev : pin;  // pin(nlev+1) = pio(nlev+1)
    }
  }
  __syncthreads();
  // bracket search (:160-172), one (k,p) per work item; ends at pio(nlev+2) = pio(nlev+1) + 1 at the latest on a grid that passed the
  // check, and at the last row of pio on any other
  for (int w = tid; w < NLEV * 16; w += nthreads) {
    const int k = (w >> 4) + 1, p = w & 15;
    const double pin_k1 = S.z2[k - 1][p];
    int kk = k;
    while (kk < NLEV + 2 && pio[kk - 1][p] <= pin_k1) kk++;
    kk--;
    if (kk == NLEV + 1) kk = NLEV;
    S.kid[k - 1][p] = (unsigned char)kk;
    S.z2[k - 1][p] = (pin_k1 - (pio[kk - 1][p] + pio[kk][p]) * 0.5) / dpo[kk + 1][p];
  }
  __syncthreads();   // pio and the parked dp_tgt are dead: the coefficients go where they were
  remap_grid_coefs(S, tid, nthreads);
  __syncthreads();
  // ---- phase 2
  const int p = tid & 15;
  double* const base = a.field + e * a.fs[0] + (p >> 2) * a.fs[3] + (p & 3) * a.fs[4];
  for (int f = tid >> 4; f < nf; f += nthreads >> 4) remap_columns_view<ALG2, MEAN, WIDE>(S, dpt, base + f * a.fs[1], a.fs[2], p);
}

// ---- DSS of a host's own fields through a strided view (tse_dss_view) -------------------------------------------------------------
// f <- rspheremp * DSS(w), w = spheremp * f (MODE 0, a stored product) or w = f (MODE 1), for nf fields of nk levels in the host's own
// array, in place.  12 of an element's 16 points are shared, so a pass that read its neighbours from the host's array would race with
// their writers: the field crosses twice through a dense staging field stage[e][layer][16], layer = f * nk + k.
//   k_dss_view_stage   view -> w -> stage, whole 128-byte lines on the stage side
//   (k_pack from the stage, halo_exchange: on a rank with neighbours)
//   k_dss_view_sum     own w and the up to three contributions of dss_tab[e][p][0..2] from the stage (local) or the receive buffer
//                      (remote, [column][layer]), added in table order, times rspheremp, -> view
// The three paths of a view (tse_views.h) address the view side only:
//   PATH 0  point-fastest: thread = (element, layer, part of the 128-byte line), 16 bytes per lane (WIDE: view base 16-byte aligned, even
//           element / q / level strides) or 8;
//   PATH 2  any strides: thread = (element, layer, point), one address per entry;
//   PATH 1  level-fastest, nk == NLEV: block = (element, field), the rows of consecutive levels pass through the LDS image tile[p][VIEW_PITCH]
//           with the lane mapping of k_view_levels (WIDE as there).
// Every sum is ((w + c0) + c1) + c2 with +0.0 for an absent contribution and nothing contracted: the three paths, and any cut of the mesh
// into ranks, give the same bits.
// base, nl: where a stage kernel that shares the staging field with another (tse_hypervis_view) puts its layers -- layer base + f * nk + k
// of nl per element; every other call has base 0 and nl = nf * nk.  Read by k_lap_view_stage, k_vlap_view_stage and k_dss_view_final alone.
struct DssViewArgs { long long vs[5]; int nf, nk, base, nl; };

// the view side of a level-fastest tile, as k_view_levels moves it: 16 rows of K consecutive levels at pitch S <-> tile[p][VIEW_PITCH]
template <bool WIDE, int K>
__device__ __forceinline__ void dss_rows_to_tile(const double* __restrict__ V, long long S, double* __restrict__ tile, int tid) {
  constexpr int KP = K / 2;
  static_assert(K % 2 == 0, "whole level pairs");
  if (WIDE) {
    constexpr int NV = (16 * KP + VIEW_THREADS - 1) / VIEW_THREADS;
    double2 r[NV];
#pragma unroll
    for (int u = 0; u < NV; u++) { const int it = min(u * VIEW_THREADS + tid, 16 * KP - 1); r[u] = *(const double2*)(V + (it / KP) * S + 2 * (it % KP)); }   // (a lane past the end reloads the last item)
#pragma unroll
    for (int u = 0; u < NV; u++) view_keep(r[u]);
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int it = u * VIEW_THREADS + tid;
      if (it < 16 * KP) *(double2*)(tile + (it / KP) * VIEW_PITCH + 2 * (it % KP)) = r[u];
    }
  } else {
    constexpr int NV = (16 * K + VIEW_THREADS - 1) / VIEW_THREADS;
    double r[NV];
#pragma unroll
    for (int u = 0; u < NV; u++) { const int it = min(u * VIEW_THREADS + tid, 16 * K - 1); r[u] = V[(it / K) * S + it % K]; }
#pragma unroll
    for (int u = 0; u < NV; u++) view_keep(r[u]);
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int it = u * VIEW_THREADS + tid;
      if (it < 16 * K) tile[(it / K) * VIEW_PITCH + it % K] = r[u];
    }
  }
}
template <bool WIDE, int K>
__device__ __forceinline__ void dss_tile_to_rows(const double* __restrict__ tile, double* __restrict__ V, long long S, int tid) {
  constexpr int KP = K / 2;
  if (WIDE) {
    for (int it = tid; it < 16 * KP; it += VIEW_THREADS) *(double2*)(V + (it / KP) * S + 2 * (it % KP)) = *(const double2*)(tile + (it / KP) * VIEW_PITCH + 2 * (it % KP));
  } else {
    for (int it = tid; it < 16 * K; it += VIEW_THREADS) V[(it / K) * S + it % K] = tile[(it / K) * VIEW_PITCH + it % K];
  }
}

template <int PATH, bool WIDE, int MODE>
__global__ __launch_bounds__(VIEW_THREADS) void k_dss_view_stage(int nelemd, DssViewArgs a, const double* __restrict__ spheremp, const double* __restrict__ view,
                                                                 double* __restrict__ stage) {
#pragma clang fp contract(off)
  const int nl = a.nf * a.nk;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[16 * VIEW_PITCH];
    constexpr int K = NLEV, NL = (8 * K + VIEW_THREADS - 1) / VIEW_THREADS;
    const int f = (int)(blockIdx.x % (unsigned)a.nf), tid = threadIdx.x, h = tid & 7;
    const long long e = (long long)(blockIdx.x / (unsigned)a.nf);
    const double2 m = *(const double2*)(spheremp + (size_t)e * 16 + 2 * h);
    dss_rows_to_tile<WIDE, K>(view + e * a.vs[0] + f * a.vs[1], a.vs[4], tile, tid);
    __syncthreads();
    double* L = stage + ((size_t)e * nl + (size_t)f * K) * 16;
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int it = u * VIEW_THREADS + tid;
      if (it < 8 * K) {
        const double* s = tile + 2 * h * VIEW_PITCH + (it >> 3);
        double2 x = make_double2(s[0], s[VIEW_PITCH]);
        if (MODE == 0) { x.x = m.x * x.x; x.y = m.y * x.y; }
        *(double2*)(L + (it >> 3) * 16 + 2 * h) = x;
      }
    }
  } else {
    constexpr int W = (PATH == 0 && WIDE) ? 2 : 1, PARTS = 16 / W;
    const size_t t = (size_t)blockIdx.x * VIEW_THREADS + threadIdx.x;
    if (t >= (size_t)nelemd * nl * PARTS) return;
    const int part = (int)(t % PARTS);
    const size_t r = t / PARTS;
    const int layer = (int)(r % (unsigned)nl);
    const long long e = (long long)(r / (unsigned)nl);
    const int f = layer / a.nk, k = layer - f * a.nk;
    const double* V = view + e * a.vs[0] + f * a.vs[1] + k * a.vs[2];
    double* S = stage + ((size_t)e * nl + layer) * 16 + part * W;
    if (W == 2) {
      double2 x = *(const double2*)(V + 2 * part);
      if (MODE == 0) { const double2 m = *(const double2*)(spheremp + (size_t)e * 16 + 2 * part); x.x = m.x * x.x; x.y = m.y * x.y; }
      *(double2*)S = x;
    } else {
      double x = V[(part >> 2) * a.vs[3] + (part & 3) * a.vs[4]];
      if (MODE == 0) x = spheremp[(size_t)e * 16 + part] * x;
      *S = x;
    }
  }
}

// ((w + c0) + c1) + c2 of point p of element e in one layer.  Every slot is one unconditional load, as in k_dss_lvl: an empty slot re-reads
// the point's own w and adds +0.0 whatever it read, a local one reads the neighbour's line of the stage, a remote one the receive buffer.
__device__ __forceinline__ double dss_view_point(const int2* __restrict__ tab, const double* __restrict__ stage, const double* __restrict__ recvbuf, int nl,
                                                 int e, int p, int layer, double& rs, const double* __restrict__ rspheremp) {
#pragma clang fp contract(off)
  const double* own = stage + ((size_t)e * nl + layer) * 16 + p;
  const int2* tt = tab + ((size_t)e * 16 + p) * 3;
  const double* ap[3];
  bool has[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int2 t = tt[s];
    ap[s] = own; has[s] = false;
    if (t.x >= 0) { ap[s] = stage + ((size_t)t.x * nl + layer) * 16 + t.y; has[s] = true; }
    else if (t.x <= -2) { ap[s] = recvbuf + (size_t)(-(t.x + 2)) * nl + layer; has[s] = true; }
  }
  double w = *own, c[3];
  rs = rspheremp[(size_t)e * 16 + p];
#pragma unroll
  for (int s = 0; s < 3; s++) c[s] = *ap[s];
#pragma unroll
  for (int s = 0; s < 3; s++) c[s] = has[s] ? c[s] : 0.0;
  w = w + c[0]; w = w + c[1]; w = w + c[2];
  return w;
}

// Blocks are dealt to the XCDs in contiguous ranges of `order` (blockIdx & 7 = the XCD, as in dss_lane), so that the lines of a
// neighbour come from the L2 that holds the block's own.  PATH 0 / 2: lanes flattened over (element slot, layer, part) within a range;
// PATH 1: block = (element slot, field).
template <int PATH, bool WIDE>
__global__ __launch_bounds__(VIEW_THREADS) void k_dss_view_sum(int nelemd, DssViewArgs a, const int2* __restrict__ tab, const double* __restrict__ rspheremp,
                                                               const double* __restrict__ stage, const double* __restrict__ recvbuf, const int* __restrict__ order,
                                                               double* __restrict__ view) {
#pragma clang fp contract(off)
  const int nl = a.nf * a.nk;
  const int S8 = (nelemd + 7) >> 3, xcd = blockIdx.x & 7;
  const unsigned it = blockIdx.x >> 3;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[16 * VIEW_PITCH];
    constexpr int K = NLEV, NL = (8 * K + VIEW_THREADS - 1) / VIEW_THREADS;
    const int idx = (int)(it / (unsigned)a.nf), f = (int)(it % (unsigned)a.nf), slot = xcd * S8 + idx;
    if (idx >= S8 || slot >= nelemd) return;   // (uniform over the block: before the barrier)
    const int e = order[slot], tid = threadIdx.x, h = tid & 7;
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int i2 = u * VIEW_THREADS + tid;
      if (i2 < 8 * K) {
        const int k = i2 >> 3;
        double r0, r1;
        const double x0 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * h, f * K + k, r0, rspheremp);
        const double x1 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * h + 1, f * K + k, r1, rspheremp);
        double* s = tile + 2 * h * VIEW_PITCH + k;
        s[0] = r0 * x0; s[VIEW_PITCH] = r1 * x1;
      }
    }
    __syncthreads();
    dss_tile_to_rows<WIDE, K>(tile, view + (long long)e * a.vs[0] + f * a.vs[1], a.vs[4], tid);
  } else {
    constexpr int W = (PATH == 0 && WIDE) ? 2 : 1, PARTS = 16 / W;
    const long long units = (long long)nl * PARTS;
    const long long g = (long long)it * VIEW_THREADS + threadIdx.x;
    const long long idx = g / units;
    const int r = (int)(g - idx * units);
    const long long slot = (long long)xcd * S8 + idx;
    if (idx >= S8 || slot >= nelemd) return;
    const int e = order[slot], layer = r / PARTS, part = r - layer * PARTS;
    const int f = layer / a.nk, k = layer - f * a.nk;
    double* V = view + (long long)e * a.vs[0] + f * a.vs[1] + k * a.vs[2];
    if (W == 2) {
      double r0, r1;
      const double x0 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * part, layer, r0, rspheremp);
      const double x1 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * part + 1, layer, r1, rspheremp);
      *(double2*)(V + 2 * part) = make_double2(r0 * x0, r1 * x1);
    } else {
      double r0;
      const double x0 = dss_view_point(tab, stage, recvbuf, nl, e, part, layer, r0, rspheremp);
      V[(part >> 2) * a.vs[3] + (part & 3) * a.vs[4]] = r0 * x0;
    }
  }
}
// blocks of k_dss_view_sum<0 | 2>: 8 XCD ranges of ceil(nelemd / 8) element slots, `units` lanes per element
inline long long dss_view_sum_blocks(int nelemd, long long units) { return 8 * ((((long long)((nelemd + 7) >> 3)) * units + VIEW_THREADS - 1) / VIEW_THREADS); }

// ---- weak Laplacian and biharmonic of a host's own scalar fields through strided views (tse_biharmonic_view) ------------------------
// ORDER 1: out = laplace_sphere_wk(in) (weak, not summed).  ORDER 2: out = laplace_sphere_wk(rspheremp * DSS(laplace_sphere_wk(in))),
// biharmonic_wk_scalar / biharmonic_wk_dp3d's scalar part (viscosity_mod.F90:229-279,315-344) before the final DSS, for nf fields of nk
// levels.  The Laplacian is k_elem_op<1>'s -- load_row_geo, make_lap_geo, laplace_lean_row, a quad of lanes per slab, lane = row j -- and
// the sum is k_dss_view_sum's (dss_view_point, then one product with rspheremp), so order 2 has the bits of
// tse_laplace_sphere_wk -> tse_dss_view(WEAK) -> tse_laplace_sphere_wk.  Two launches for either order, four passes over the field:
//   k_lap_view_stage<PATH, WIDE>       in -> lap -> stage[e][layer][16], a quad writes one 128-byte line
//   (k_pack from the stage, halo_exchange: ORDER 2 on a rank with neighbours)
//   k_lap_view_out<PATH, WIDE, ORDER>  ORDER 2: every lane gathers the four points of its row (own line, the neighbours' lines, the receive
//                                      buffer), times rspheremp; the quad applies the second Laplacian -> out.  ORDER 1: own line -> out.
// PATH and WIDE are those of the kernel's own view (the stage kernel's of `in`, the out kernel's of `out`), as in k_dss_view_stage:
//   PATH 0  a lane's row is one 32-byte access (WIDE) or four 8-byte ones, a quad's slab one line;
//   PATH 2  one address per entry;
//   PATH 1  block = (element, field): the view side passes through the LDS image tile[p][VIEW_PITCH] (dss_rows_to_tile /
//           dss_tile_to_rows), quad q of the block takes the levels q, q + 64, ...
// On paths 0 and 2 a thread keeps its LapGeo (20 doubles, formed from 36 loaded ones) over LAP_VIEW_LAYERS consecutive layers of its
// element.  Whole quads stay active (quad_matvec moves data across the quad): element and layer indices are clamped and only the
// store is predicated; every predicate is the same for the four lanes of a quad.
#ifndef TSE_LAP_VIEW_LAYERS
#define TSE_LAP_VIEW_LAYERS 4   // (profiles/biharmonic_view_rate.txt holds the comparison of 1, 2, 4 and 8)
#endif
constexpr int LAP_VIEW_LAYERS = TSE_LAP_VIEW_LAYERS;

template <int PATH, bool WIDE>
__device__ __forceinline__ void lap_view_load_row(const double* __restrict__ V, const DssViewArgs& a, int j, double s[4]) {
  if (PATH == 0 && WIDE) load4(V + 4 * j, s);
  else if (PATH == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = V[4 * j + i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = V[j * a.vs[3] + i * a.vs[4]];
  }
}
template <int PATH, bool WIDE>
__device__ __forceinline__ void lap_view_store_row(double* __restrict__ V, const DssViewArgs& a, int j, const double r[4]) {
  if (PATH == 0 && WIDE) store4(V + 4 * j, r);
  else if (PATH == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) V[4 * j + i] = r[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) V[j * a.vs[3] + i * a.vs[4]] = r[i];
  }
}
inline long long lap_view_groups(long long nl) { return (nl + LAP_VIEW_LAYERS - 1) / LAP_VIEW_LAYERS; }

template <int PATH, bool WIDE>
__global__ __launch_bounds__(VIEW_THREADS) void k_lap_view_stage(int nelemd, DssViewArgs a, Dvv_t D, GeoPtrs G, const double* __restrict__ view,
                                                                 double* __restrict__ stage) {
#pragma clang fp contract(off)
  const int nl = a.nf * a.nk, tid = threadIdx.x, j = tid & 3;
  RowGeo g;
  LapGeo L;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[16 * VIEW_PITCH];
    constexpr int K = NLEV;
    const int f = (int)(blockIdx.x % (unsigned)a.nf), e = (int)(blockIdx.x / (unsigned)a.nf);   // (the grid is nelemd * nf blocks)
    load_row_geo(g, G.dvv, G.Dinv, G.metdet, G.rmetdet, G.spheremp, e, j);
    make_lap_geo(L, g);
    dss_rows_to_tile<WIDE, K>(view + (long long)e * a.vs[0] + f * a.vs[1], a.vs[4], tile, tid);
    __syncthreads();
    double* S = stage + ((size_t)e * a.nl + a.base + (size_t)f * K) * 16 + 4 * j;
    for (int k = tid >> 2; k < K; k += VIEW_THREADS / 4) {
      double s[4], r[4];
#pragma unroll
      for (int i = 0; i < 4; i++) s[i] = tile[(4 * j + i) * VIEW_PITCH + k];
      laplace_lean_row(D, L, s, r);
      store4(S + (size_t)k * 16, r);
    }
  } else {
    const int groups = (nl + LAP_VIEW_LAYERS - 1) / LAP_VIEW_LAYERS;
    const size_t qd = ((size_t)blockIdx.x * VIEW_THREADS + tid) >> 2;
    const size_t eraw = qd / (unsigned)groups;
    const int grp = (int)(qd - eraw * (unsigned)groups);
    const bool live = eraw < (size_t)nelemd;
    const int e = live ? (int)eraw : nelemd - 1;
    load_row_geo(g, G.dvv, G.Dinv, G.metdet, G.rmetdet, G.spheremp, e, j);
    make_lap_geo(L, g);
    const int l0 = grp * LAP_VIEW_LAYERS;
#pragma unroll
    for (int u = 0; u < LAP_VIEW_LAYERS; u++) {
      const int layer = min(l0 + u, nl - 1);
      const int f = layer / a.nk, k = layer - f * a.nk;
      double s[4], r[4];
      lap_view_load_row<PATH, WIDE>(view + (long long)e * a.vs[0] + f * a.vs[1] + k * a.vs[2], a, j, s);
      laplace_lean_row(D, L, s, r);
      if (live && l0 + u < nl) store4(stage + ((size_t)e * a.nl + a.base + layer) * 16 + 4 * j, r);
    }
  }
}

template <int PATH, bool WIDE, int ORDER>
__global__ __launch_bounds__(VIEW_THREADS) void k_lap_view_out(int nelemd, DssViewArgs a, Dvv_t D, GeoPtrs G, const int2* __restrict__ tab,
                                                               const double* __restrict__ stage, const double* __restrict__ recvbuf,
                                                               const int* __restrict__ order, double* __restrict__ view) {
#pragma clang fp contract(off)
  const int nl = a.nf * a.nk, tid = threadIdx.x, j = tid & 3;
  const int S8 = (nelemd + 7) >> 3, xcd = blockIdx.x & 7;   // contiguous ranges of `order` per XCD, as in k_dss_view_sum
  const unsigned it = blockIdx.x >> 3;
  RowGeo g;
  LapGeo L;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[16 * VIEW_PITCH];
    constexpr int K = NLEV;
    const int idx = (int)(it / (unsigned)a.nf), f = (int)(it % (unsigned)a.nf), slot = xcd * S8 + idx;
    if (idx >= S8 || slot >= nelemd) return;   // (uniform over the block: before the barrier)
    const int e = order[slot];
    if (ORDER == 2) {
      load_row_geo(g, G.dvv, G.Dinv, G.metdet, G.rmetdet, G.spheremp, e, j);
      make_lap_geo(L, g);
    }
    for (int k = tid >> 2; k < K; k += VIEW_THREADS / 4) {
      double m[4], r[4];
      if (ORDER == 2) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          double rs;
          const double x = dss_view_point(tab, stage, recvbuf, nl, e, 4 * j + i, f * K + k, rs, G.rspheremp);
          m[i] = rs * x;
        }
        laplace_lean_row(D, L, m, r);
      } else load4(stage + ((size_t)e * nl + (size_t)f * K + k) * 16 + 4 * j, r);
#pragma unroll
      for (int i = 0; i < 4; i++) tile[(4 * j + i) * VIEW_PITCH + k] = r[i];
    }
    __syncthreads();
    dss_tile_to_rows<WIDE, K>(tile, view + (long long)e * a.vs[0] + f * a.vs[1], a.vs[4], tid);
  } else {
    const int groups = (nl + LAP_VIEW_LAYERS - 1) / LAP_VIEW_LAYERS;
    const long long qd = ((long long)it * VIEW_THREADS + tid) >> 2;
    const long long idx = qd / groups;
    const int grp = (int)(qd - idx * groups);
    const long long slot = (long long)xcd * S8 + idx;
    const bool live = idx < S8 && slot < nelemd;
    const int e = order[live ? slot : nelemd - 1];
    if (ORDER == 2) {
      load_row_geo(g, G.dvv, G.Dinv, G.metdet, G.rmetdet, G.spheremp, e, j);
      make_lap_geo(L, g);
    }
    const int l0 = grp * LAP_VIEW_LAYERS;
#pragma unroll
    for (int u = 0; u < LAP_VIEW_LAYERS; u++) {
      const int layer = min(l0 + u, nl - 1);
      const int f = layer / a.nk, k = layer - f * a.nk;
      double m[4], r[4];
      if (ORDER == 2) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          double rs;
          const double x = dss_view_point(tab, stage, recvbuf, nl, e, 4 * j + i, layer, rs, G.rspheremp);
          m[i] = rs * x;
        }
        laplace_lean_row(D, L, m, r);
      } else load4(stage + ((size_t)e * nl + layer) * 16 + 4 * j, r);
      if (live && l0 + u < nl) lap_view_store_row<PATH, WIDE>(view + (long long)e * a.vs[0] + f * a.vs[1] + k * a.vs[2], a, j, r);
    }
  }
}
// blocks of k_lap_view_out<0 | 2>: 8 XCD ranges of ceil(nelemd / 8) element slots, one quad per LAP_VIEW_LAYERS layers of an element
inline long long lap_view_out_blocks(int nelemd, long long nl) { return dss_view_sum_blocks(nelemd, 4 * lap_view_groups(nl)); }

// ---- weak vector Laplacian and biharmonic of a host's own wind through strided views (tse_vlaplace_view) -----------------------------
// ORDER 1: out = vlaplace_sphere_wk(in) (weak, not summed).  ORDER 2: out = vlaplace_sphere_wk(rspheremp * DSS(vlaplace_sphere_wk(in))),
// the wind's line of biharmonic_wk_dp3d (viscosity_mod.F90:177-286) before the final DSS, for nk levels of the two components of one view
// (q axis = component).  The operator is vlaplace_row (tse_device.h) on the tables k_vec_fold leaves; the sum is k_dss_view_sum's
// (dss_view_point over 2 * nk layers, then one product with rspheremp).  The kernels are k_lap_view_stage / k_lap_view_out with both
// components of a level in one quad, because the operator couples them: layer c * nk + k of the staging field is component c of level k.
//   PATH 0, 2  a quad takes VLAP_VIEW_LEVELS consecutive levels of its element (2 levels = 4 layers, the scalar kernels' 4 layers per thread)
//   PATH 1     block = element; both components pass through LDS images of their own
// k_vec_fold: one thread per point, tab[e][VEC_TABS][16] from the library's Dinv, metdet, rmetdet, spheremp and the host's D, metinv, mp
// (src[e][p][9] = D(a + 2b), metinv(a + 2b), mp).  Every product is rounded once, in the order written here.
constexpr int VLAP_VIEW_LEVELS = 2;
template <int = 0>
__global__ __launch_bounds__(256) void k_vec_fold(int nelemd, GeoPtrs G, const double* __restrict__ src, double* __restrict__ tab) {
#pragma clang fp contract(off)
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nelemd * 16) return;
  const size_t e = t >> 4;
  const int p = (int)(t & 15);
  const double* s = src + t * 9;
  double* o = tab + e * VEC_TABS * 16 + p;
  const double g = G.metdet[t], rg = RREARTH * g;
  double Dr[4], mg[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    o[k * 16] = rg * G.Dinv[t * 4 + k];
    Dr[k] = RREARTH * s[k];
    mg[k] = g * s[4 + k];
    o[(4 + k) * 16] = Dr[k];
  }
#pragma unroll
  for (int c = 0; c < 2; c++) {
    o[(8 + c) * 16] = -fma(Dr[c + 2], mg[2], Dr[c] * mg[0]);    // G(c,1) = -rrearth * metdet * (D(c,1) metinv(1,1) + D(c,2) metinv(1,2))
    o[(10 + c) * 16] = -fma(Dr[c + 2], mg[3], Dr[c] * mg[1]);   // G(c,2) = -rrearth * metdet * (D(c,1) metinv(2,1) + D(c,2) metinv(2,2))
  }
  o[12 * 16] = s[8] * G.rmetdet[t];
  o[13 * 16] = (2.0 * G.spheremp[t]) * (RREARTH * RREARTH);
}

template <int PATH, bool WIDE>
__global__ __launch_bounds__(VIEW_THREADS) void k_vlap_view_stage(int nelemd, DssViewArgs a, Dvv_t D, GeoPtrs G, const double* __restrict__ vtab, double nu_ratio,
                                                                  const double* __restrict__ view, double* __restrict__ stage) {
#pragma clang fp contract(off)
  const int nk = a.nk, nl = a.nl, tid = threadIdx.x, j = tid & 3;   // (nl = 2 * nk unless the call shares the staging field: DssViewArgs)
  VecGeo V;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[2][16 * VIEW_PITCH];
    constexpr int K = NLEV;
    const int e = (int)blockIdx.x;   // (the grid is nelemd blocks)
    load_vec_geo(V, G.dvv, vtab, e, j);
    dss_rows_to_tile<WIDE, K>(view + (long long)e * a.vs[0], a.vs[4], tile[0], tid);
    dss_rows_to_tile<WIDE, K>(view + (long long)e * a.vs[0] + a.vs[1], a.vs[4], tile[1], tid);
    __syncthreads();
    double* S = stage + ((size_t)e * nl + a.base) * 16 + 4 * j;
    for (int k = tid >> 2; k < K; k += VIEW_THREADS / 4) {
      double v1[4], v2[4], r1[4], r2[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { v1[i] = tile[0][(4 * j + i) * VIEW_PITCH + k]; v2[i] = tile[1][(4 * j + i) * VIEW_PITCH + k]; }
      vlaplace_row(D, V, nu_ratio, v1, v2, r1, r2);
      store4(S + (size_t)k * 16, r1);
      store4(S + (size_t)(K + k) * 16, r2);
    }
  } else {
    const int groups = (nk + VLAP_VIEW_LEVELS - 1) / VLAP_VIEW_LEVELS;
    const size_t qd = ((size_t)blockIdx.x * VIEW_THREADS + tid) >> 2;
    const size_t eraw = qd / (unsigned)groups;
    const int grp = (int)(qd - eraw * (unsigned)groups);
    const bool live = eraw < (size_t)nelemd;
    const int e = live ? (int)eraw : nelemd - 1;
    load_vec_geo(V, G.dvv, vtab, e, j);
    const int k0 = grp * VLAP_VIEW_LEVELS;
#pragma unroll
    for (int u = 0; u < VLAP_VIEW_LEVELS; u++) {
      const int k = min(k0 + u, nk - 1);
      double v1[4], v2[4], r1[4], r2[4];
      const double* P = view + (long long)e * a.vs[0] + k * a.vs[2];
      lap_view_load_row<PATH, WIDE>(P, a, j, v1);
      lap_view_load_row<PATH, WIDE>(P + a.vs[1], a, j, v2);
      vlaplace_row(D, V, nu_ratio, v1, v2, r1, r2);
      if (live && k0 + u < nk) {
        store4(stage + ((size_t)e * nl + a.base + k) * 16 + 4 * j, r1);
        store4(stage + ((size_t)e * nl + a.base + nk + k) * 16 + 4 * j, r2);
      }
    }
  }
}

template <int PATH, bool WIDE, int ORDER>
__global__ __launch_bounds__(VIEW_THREADS) void k_vlap_view_out(int nelemd, DssViewArgs a, Dvv_t D, GeoPtrs G, const double* __restrict__ vtab, double nu_ratio,
                                                                const int2* __restrict__ tab, const double* __restrict__ stage, const double* __restrict__ recvbuf,
                                                                const int* __restrict__ order, double* __restrict__ view) {
#pragma clang fp contract(off)
  const int nk = a.nk, nl = 2 * nk, tid = threadIdx.x, j = tid & 3;
  const int S8 = (nelemd + 7) >> 3, xcd = blockIdx.x & 7;   // contiguous ranges of `order` per XCD, as in k_dss_view_sum
  const unsigned it = blockIdx.x >> 3;
  VecGeo V;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[2][16 * VIEW_PITCH];
    constexpr int K = NLEV;
    const int idx = (int)it, slot = xcd * S8 + idx;
    if (idx >= S8 || slot >= nelemd) return;   // (uniform over the block: before the barrier)
    const int e = order[slot];
    if (ORDER == 2) load_vec_geo(V, G.dvv, vtab, e, j);
    for (int k = tid >> 2; k < K; k += VIEW_THREADS / 4) {
      double r1[4], r2[4];
      if (ORDER == 2) {
        double m1[4], m2[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          double rs;
          const double x1 = dss_view_point(tab, stage, recvbuf, nl, e, 4 * j + i, k, rs, G.rspheremp);
          const double x2 = dss_view_point(tab, stage, recvbuf, nl, e, 4 * j + i, K + k, rs, G.rspheremp);
          m1[i] = rs * x1; m2[i] = rs * x2;
        }
        vlaplace_row(D, V, nu_ratio, m1, m2, r1, r2);
      } else {
        load4(stage + ((size_t)e * nl + k) * 16 + 4 * j, r1);
        load4(stage + ((size_t)e * nl + K + k) * 16 + 4 * j, r2);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) { tile[0][(4 * j + i) * VIEW_PITCH + k] = r1[i]; tile[1][(4 * j + i) * VIEW_PITCH + k] = r2[i]; }
    }
    __syncthreads();
    dss_tile_to_rows<WIDE, K>(tile[0], view + (long long)e * a.vs[0], a.vs[4], tid);
    dss_tile_to_rows<WIDE, K>(tile[1], view + (long long)e * a.vs[0] + a.vs[1], a.vs[4], tid);
  } else {
    const int groups = (nk + VLAP_VIEW_LEVELS - 1) / VLAP_VIEW_LEVELS;
    const long long qd = ((long long)it * VIEW_THREADS + tid) >> 2;
    const long long idx = qd / groups;
    const int grp = (int)(qd - idx * groups);
    const long long slot = (long long)xcd * S8 + idx;
    const bool live = idx < S8 && slot < nelemd;
    const int e = order[live ? slot : nelemd - 1];
    if (ORDER == 2) load_vec_geo(V, G.dvv, vtab, e, j);
    const int k0 = grp * VLAP_VIEW_LEVELS;
#pragma unroll
    for (int u = 0; u < VLAP_VIEW_LEVELS; u++) {
      const int k = min(k0 + u, nk - 1);
      double r1[4], r2[4];
      if (ORDER == 2) {
        double m1[4], m2[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          double rs;
          const double x1 = dss_view_point(tab, stage, recvbuf, nl, e, 4 * j + i, k, rs, G.rspheremp);
          const double x2 = dss_view_point(tab, stage, recvbuf, nl, e, 4 * j + i, nk + k, rs, G.rspheremp);
          m1[i] = rs * x1; m2[i] = rs * x2;
        }
        vlaplace_row(D, V, nu_ratio, m1, m2, r1, r2);
      } else {
        load4(stage + ((size_t)e * nl + k) * 16 + 4 * j, r1);
        load4(stage + ((size_t)e * nl + nk + k) * 16 + 4 * j, r2);
      }
      if (live && k0 + u < nk) {
        double* P = view + (long long)e * a.vs[0] + k * a.vs[2];
        lap_view_store_row<PATH, WIDE>(P, a, j, r1);
        lap_view_store_row<PATH, WIDE>(P + a.vs[1], a, j, r2);
      }
    }
  }
}
inline long long vlap_view_groups(long long nk) { return (nk + VLAP_VIEW_LEVELS - 1) / VLAP_VIEW_LEVELS; }
// blocks of k_vlap_view_out<0 | 2>: 8 XCD ranges of ceil(nelemd / 8) element slots, one quad per VLAP_VIEW_LEVELS levels of an element
inline long long vlap_view_out_blocks(int nelemd, long long nk) { return dss_view_sum_blocks(nelemd, 4 * vlap_view_groups(nk)); }

// ---- one hyperviscosity sub-step of a host's own scalars and wind through strided views (tse_hypervis_view) --------------------------
// x <- x + rspheremp * DSS(coef * biharmonic(x)) for nf scalar fields and the wind, both halves through ONE staging field of
// nl = (nf + 2) * nk layers -- the scalars' layers f * nk + k first, then the wind's nf * nk + c * nk + k -- so that a sub-step costs two
// exchanges of nl layers, biharmonic_wk_dp3d's one and advance_hypervis_dp's one, whatever it holds:
//   k_lap_view_stage, k_vlap_view_stage   x -> lap -> stage (DssViewArgs::base / nl place each half)
//   (pack, halo_exchange)
//   k_lap_view_mid, k_vlap_view_mid           stage -> [sum, rspheremp, second Laplacian, times coef] -> stage2: k_lap_view_out<., ., 2> and
//                                         k_vlap_view_out<., ., 2> on their flattened path with a dense destination and one product more.
//                                         A second field, not the first in place: the neighbours' lines of the first are still being read.
//   (pack, halo_exchange)
//   k_dss_view_final<ADD>                       stage2 -> [sum, rspheremp] -> x + d (ADD: in place, x is read and written once) or -> the out views;
//                                         ONE launch for both halves: blocks [0, blocks0) serve side 0, the others side 1, and each side
//                                         brings the form of its own view (HvForm: the view side of k_dss_view_sum's three paths).
// Every step is the statement of the kernel it is taken from, so a point's result has the bits of tse_biharmonic_view / tse_vlaplace_view
// (order 2) -> one product -> tse_dss_view(TSE_DSS_WEAK) -> one addition.
constexpr int HV_MAX_FIELDS = TSE_HYPERVIS_MAX_FIELDS;
struct HvCoef { double c[HV_MAX_FIELDS]; };   // the scalars' factors, by value: no buffer to fill, nothing for a later call to overwrite

template <int = 0>
__global__ __launch_bounds__(VIEW_THREADS) void k_lap_view_mid(int nelemd, int nf, int nk, int nlt, HvCoef cf, Dvv_t D, GeoPtrs G, const int2* __restrict__ tab,
                                                             const double* __restrict__ stage, const double* __restrict__ recvbuf,
                                                             const int* __restrict__ order, double* __restrict__ stage2) {
#pragma clang fp contract(off)
  const int nl = nf * nk, tid = threadIdx.x, j = tid & 3;
  const int S8 = (nelemd + 7) >> 3, xcd = blockIdx.x & 7;   // contiguous ranges of `order` per XCD, as in k_dss_view_sum
  const unsigned it = blockIdx.x >> 3;
  RowGeo g;
  LapGeo L;
  const int groups = (nl + LAP_VIEW_LAYERS - 1) / LAP_VIEW_LAYERS;
  const long long qd = ((long long)it * VIEW_THREADS + tid) >> 2;
  const long long idx = qd / groups;
  const int grp = (int)(qd - idx * groups);
  const long long slot = (long long)xcd * S8 + idx;
  const bool live = idx < S8 && slot < nelemd;
  const int e = order[live ? slot : nelemd - 1];
  load_row_geo(g, G.dvv, G.Dinv, G.metdet, G.rmetdet, G.spheremp, e, j);
  make_lap_geo(L, g);
  const int l0 = grp * LAP_VIEW_LAYERS;
#pragma unroll
  for (int u = 0; u < LAP_VIEW_LAYERS; u++) {
    const int layer = min(l0 + u, nl - 1);
    const double cl = cf.c[layer / nk];
    double m[4], r[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      double rs;
      const double x = dss_view_point(tab, stage, recvbuf, nlt, e, 4 * j + i, layer, rs, G.rspheremp);
      m[i] = rs * x;
    }
    laplace_lean_row(D, L, m, r);
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = cl * r[i];
    if (live && l0 + u < nl) store4(stage2 + ((size_t)e * nlt + layer) * 16 + 4 * j, r);
  }
}

template <int = 0>
__global__ __launch_bounds__(VIEW_THREADS) void k_vlap_view_mid(int nelemd, int nk, int base, int nlt, double cv, Dvv_t D, GeoPtrs G, const double* __restrict__ vtab,
                                                              double nu_ratio, const int2* __restrict__ tab, const double* __restrict__ stage,
                                                              const double* __restrict__ recvbuf, const int* __restrict__ order, double* __restrict__ stage2) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, j = tid & 3;
  const int S8 = (nelemd + 7) >> 3, xcd = blockIdx.x & 7;
  const unsigned it = blockIdx.x >> 3;
  VecGeo V;
  const int groups = (nk + VLAP_VIEW_LEVELS - 1) / VLAP_VIEW_LEVELS;
  const long long qd = ((long long)it * VIEW_THREADS + tid) >> 2;
  const long long idx = qd / groups;
  const int grp = (int)(qd - idx * groups);
  const long long slot = (long long)xcd * S8 + idx;
  const bool live = idx < S8 && slot < nelemd;
  const int e = order[live ? slot : nelemd - 1];
  load_vec_geo(V, G.dvv, vtab, e, j);
  const int k0 = grp * VLAP_VIEW_LEVELS;
#pragma unroll
  for (int u = 0; u < VLAP_VIEW_LEVELS; u++) {
    const int k = min(k0 + u, nk - 1);
    double m1[4], m2[4], r1[4], r2[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      double rs;
      const double x1 = dss_view_point(tab, stage, recvbuf, nlt, e, 4 * j + i, base + k, rs, G.rspheremp);
      const double x2 = dss_view_point(tab, stage, recvbuf, nlt, e, 4 * j + i, base + nk + k, rs, G.rspheremp);
      m1[i] = rs * x1; m2[i] = rs * x2;
    }
    vlaplace_row(D, V, nu_ratio, m1, m2, r1, r2);
#pragma unroll
    for (int i = 0; i < 4; i++) { r1[i] = cv * r1[i]; r2[i] = cv * r2[i]; }
    if (live && k0 + u < nk) {
      store4(stage2 + ((size_t)e * nlt + base + k) * 16 + 4 * j, r1);
      store4(stage2 + ((size_t)e * nlt + base + nk + k) * 16 + 4 * j, r2);
    }
  }
}

// the view side of k_dss_view_final, chosen per side at run time (uniform over a block): 16-byte parts of a point-fastest line, one address per
// entry (path 2, and path 0 without the alignment), the rows of a level-fastest tile with 16 or 8 bytes per lane
enum HvForm { HV_LINES_WIDE = 0, HV_POINTS = 1, HV_ROWS_WIDE = 2, HV_ROWS = 3 };
struct HvSide { DssViewArgs a; int form; double* x; };   // a.nf fields of a.nk levels on layers a.base + f * a.nk + k of a.nl; x: s / v (ADD) or the out view
struct HvFinalArgs { HvSide side[2]; unsigned blocks0; };

template <bool ADD>
__global__ __launch_bounds__(VIEW_THREADS) void k_dss_view_final(int nelemd, HvFinalArgs A, const int2* __restrict__ tab, const double* __restrict__ rspheremp,
                                                           const double* __restrict__ stage, const double* __restrict__ recvbuf, const int* __restrict__ order) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double tile[16 * VIEW_PITCH];
  const bool second = blockIdx.x >= A.blocks0;   // (blocks0 is a multiple of 8: the XCD of a block is that of its index within the side)
  const HvSide& S = A.side[second ? 1 : 0];
  const DssViewArgs& a = S.a;
  const unsigned bid = blockIdx.x - (second ? A.blocks0 : 0u);
  const int nl = a.nl, own = a.nf * a.nk, form = S.form;
  const int S8 = (nelemd + 7) >> 3, xcd = bid & 7;
  const unsigned it = bid >> 3;
  double* __restrict__ view = S.x;
  if (form >= HV_ROWS_WIDE) {
    constexpr int K = NLEV, NL = (8 * K + VIEW_THREADS - 1) / VIEW_THREADS;
    const int idx = (int)(it / (unsigned)a.nf), f = (int)(it % (unsigned)a.nf), slot = xcd * S8 + idx;
    if (idx >= S8 || slot >= nelemd) return;   // (uniform over the block: before the barrier)
    const int e = order[slot], tid = threadIdx.x, h = tid & 7;
    double* V = view + (long long)e * a.vs[0] + f * a.vs[1];
    if (ADD) {
      if (form == HV_ROWS_WIDE) dss_rows_to_tile<true, K>(V, a.vs[4], tile, tid); else dss_rows_to_tile<false, K>(V, a.vs[4], tile, tid);
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int i2 = u * VIEW_THREADS + tid;
      if (i2 < 8 * K) {
        const int k = i2 >> 3;
        double r0, r1;
        const double x0 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * h, a.base + f * K + k, r0, rspheremp);
        const double x1 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * h + 1, a.base + f * K + k, r1, rspheremp);
        double* s = tile + 2 * h * VIEW_PITCH + k;
        const double d0 = r0 * x0, d1 = r1 * x1;
        if (ADD) { s[0] = s[0] + d0; s[VIEW_PITCH] = s[VIEW_PITCH] + d1; }
        else { s[0] = d0; s[VIEW_PITCH] = d1; }
      }
    }
    __syncthreads();
    if (form == HV_ROWS_WIDE) dss_tile_to_rows<true, K>(tile, V, a.vs[4], tid); else dss_tile_to_rows<false, K>(tile, V, a.vs[4], tid);
  } else {
    const int PARTS = form == HV_LINES_WIDE ? 8 : 16;
    const long long units = (long long)own * PARTS;
    const long long gl = (long long)it * VIEW_THREADS + threadIdx.x;
    const long long idx = gl / units;
    const int r = (int)(gl - idx * units);
    const long long slot = (long long)xcd * S8 + idx;
    if (idx >= S8 || slot >= nelemd) return;
    const int e = order[slot], layer = r / PARTS, part = r - layer * PARTS;
    const int f = layer / a.nk, k = layer - f * a.nk;
    double* V = view + (long long)e * a.vs[0] + f * a.vs[1] + k * a.vs[2];
    if (form == HV_LINES_WIDE) {
      double r0, r1;
      const double x0 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * part, a.base + layer, r0, rspheremp);
      const double x1 = dss_view_point(tab, stage, recvbuf, nl, e, 2 * part + 1, a.base + layer, r1, rspheremp);
      double2 d = make_double2(r0 * x0, r1 * x1);
      if (ADD) { const double2 x = *(const double2*)(V + 2 * part); d.x = x.x + d.x; d.y = x.y + d.y; }
      *(double2*)(V + 2 * part) = d;
    } else {
      double r0;
      const double x0 = dss_view_point(tab, stage, recvbuf, nl, e, part, a.base + layer, r0, rspheremp);
      double* P = V + (part >> 2) * a.vs[3] + (part & 3) * a.vs[4];
      double d = r0 * x0;
      if (ADD) d = *P + d;
      *P = d;
    }
  }
}

// ---- first-order sphere operators of a host's own fields through strided views (tse_sphere_op_view) ---------------------------------
// OP 0: gradient_sphere of a scalar (1 field -> 2 components), OP 1: divergence_sphere, OP 2: vorticity_sphere of a wind (2 components ->
// 1 field), on nk levels; LOCAL: out = op(in), C0: out = rspheremp * DSS(spheremp * op(in)), make_C0 / make_C0_vector
// (viscosity_mod.F90:445-535).  One new kernel:
//   k_sphere_op_stage<PATH, WIDE, OP, C0>  in -> op -> (C0: one product with spheremp) -> stage[e][f_out * nk + k][16]; lane = row j of a
//                                          quad, a quad writes one 128-byte line per output layer
// and then C0: k_dss_view_sum on `out` with nf_out fields (tse_dss_view's sum: C0 has the bits of LOCAL -> tse_dss_view(AVERAGE)),
// LOCAL: k_lap_view_out<PATH, WIDE, 1>, the own-line copy.  PATH and WIDE are those of `in`, as in k_lap_view_stage / k_vlap_view_stage:
//   PATH 0, 2  a quad keeps its geometry over SPHERE_OP_LEVELS consecutive levels of its element
//   PATH 1     block = element; every input field passes through an LDS image of its own, quad q takes the levels q, q + 64, ...
// Whole quads stay active; only the stores are predicated.  a: the args of `in` (a.nf = 1 for OP 0, 2 otherwise).
#ifndef TSE_SPHERE_OP_LEVELS
#define TSE_SPHERE_OP_LEVELS 4   // (profiles/sphere_op_rate.txt holds the comparison)
#endif
constexpr int SPHERE_OP_LEVELS = TSE_SPHERE_OP_LEVELS;
struct SphereOpGeo { RowGeo g; VorGeo V; double sm[4]; };   // what an instantiation does not use is never loaded
template <int OP, bool C0>
__device__ __forceinline__ void load_sphere_op_geo(SphereOpGeo& S, const GeoPtrs& G, const double* __restrict__ vtab, int e, int j) {
  if (OP == 2) load_vor_geo(S.V, G.dvv, vtab, G.rmetdet, e, j);
  else load_row_geo(S.g, G.dvv, G.Dinv, G.metdet, G.rmetdet, G.spheremp, e, j);
  if (C0) load4(G.spheremp + (size_t)e * 16 + 4 * j, S.sm);
}
// x1 (, x2): the lane's row of the input field(s); r1 (, r2): of the output field(s)
template <int OP, bool C0>
__device__ __forceinline__ void sphere_op_row(const Dvv_t& D, const SphereOpGeo& S, const double x1[4], const double x2[4], double r1[4], double r2[4]) {
#pragma clang fp contract(off)
  if (OP == 0) gradient_sphere_row(D, S.g, x1, r1, r2);
  else if (OP == 1) divergence_sphere_row_spelled(D, S.g, x1, x2, r1);
  else vorticity_row(D, S.V, x1, x2, r1);
  if (C0) {
#pragma unroll
    for (int i = 0; i < 4; i++) { r1[i] = S.sm[i] * r1[i]; if (OP == 0) r2[i] = S.sm[i] * r2[i]; }
  }
}

template <int PATH, bool WIDE, int OP, bool C0>
__global__ __launch_bounds__(VIEW_THREADS) void k_sphere_op_stage(int nelemd, DssViewArgs a, Dvv_t D, GeoPtrs G, const double* __restrict__ vtab,
                                                                  const double* __restrict__ view, double* __restrict__ stage) {
#pragma clang fp contract(off)
  constexpr int NIN = OP == 0 ? 1 : 2, NOUT = OP == 0 ? 2 : 1;
  const int nk = a.nk, nl = NOUT * nk, tid = threadIdx.x, j = tid & 3;
  SphereOpGeo S;
  if (PATH == 1) {
    __shared__ __attribute__((aligned(16))) double tile[NIN][16 * VIEW_PITCH];
    constexpr int K = NLEV;
    const int e = (int)blockIdx.x;   // (the grid is nelemd blocks)
    load_sphere_op_geo<OP, C0>(S, G, vtab, e, j);
#pragma unroll
    for (int c = 0; c < NIN; c++) dss_rows_to_tile<WIDE, K>(view + (long long)e * a.vs[0] + c * a.vs[1], a.vs[4], tile[c], tid);
    __syncthreads();
    double* L = stage + (size_t)e * nl * 16 + 4 * j;
    for (int k = tid >> 2; k < K; k += VIEW_THREADS / 4) {
      double x1[4], x2[4], r1[4], r2[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { x1[i] = tile[0][(4 * j + i) * VIEW_PITCH + k]; x2[i] = tile[NIN - 1][(4 * j + i) * VIEW_PITCH + k]; }
      sphere_op_row<OP, C0>(D, S, x1, x2, r1, r2);
      store4(L + (size_t)k * 16, r1);
      if (NOUT == 2) store4(L + (size_t)(K + k) * 16, r2);
    }
  } else {
    const int groups = (nk + SPHERE_OP_LEVELS - 1) / SPHERE_OP_LEVELS;
    const size_t qd = ((size_t)blockIdx.x * VIEW_THREADS + tid) >> 2;
    const size_t eraw = qd / (unsigned)groups;
    const int grp = (int)(qd - eraw * (unsigned)groups);
    const bool live = eraw < (size_t)nelemd;
    const int e = live ? (int)eraw : nelemd - 1;
    load_sphere_op_geo<OP, C0>(S, G, vtab, e, j);
    const int k0 = grp * SPHERE_OP_LEVELS;
#pragma unroll
    for (int u = 0; u < SPHERE_OP_LEVELS; u++) {
      const int k = min(k0 + u, nk - 1);
      double x1[4], x2[4], r1[4], r2[4];
      const double* P = view + (long long)e * a.vs[0] + k * a.vs[2];
      lap_view_load_row<PATH, WIDE>(P, a, j, x1);
      if (NIN == 2) lap_view_load_row<PATH, WIDE>(P + a.vs[1], a, j, x2);
      sphere_op_row<OP, C0>(D, S, x1, x2, r1, r2);
      if (live && k0 + u < nk) {
        store4(stage + ((size_t)e * nl + k) * 16 + 4 * j, r1);
        if (NOUT == 2) store4(stage + ((size_t)e * nl + nk + k) * 16 + 4 * j, r2);
      }
    }
  }
}
inline long long sphere_op_groups(long long nk) { return (nk + SPHERE_OP_LEVELS - 1) / SPHERE_OP_LEVELS; }

// ---- min, max, sums and integrals of a host's own fields through strided views (tse_stats_view) -----------------------------------
// The element shares of prim_printstate's MIN / MAX / SUM lines and of global_integral, global_maximum, l1_snorm, l2_snorm and linf_snorm
// (prim_state_mod.F90:186-348, global_norms_mod.F90) for nf fields of nk levels: STATS_N = TSE_STATS doubles per (element, field, level)
// slab, or per (element, field).  h the field, ht the reference (REF), d = h - ht, m = spheremp[e][p] (or spheremp[e][p] * w: WGT), every
// term one rounded operation per arithmetic sign, nothing contracted:
//   0 min h   1 max h   2 sum h   3 sum m*h   4 sum m*fabs(h)   5 sum m*(h*h)   6 max fabs(h)   7 count of NaN / +-inf   14 sum m
//   8 sum m*fabs(d)   9 sum m*fabs(ht)   10 sum m*(d*d)   11 sum m*(ht*ht)   12 max fabs(d)   13 max fabs(ht)   (0 without REF)   15: 0
// A NaN does not enter an extremum (it enters as the extremum's identity: +inf for 0, -inf for 1, 0 for 6, 12 and 13); it does enter the
// sums.  NaN and +-inf are told by their bits, so the extrema never see a NaN whatever the compiler assumes about them.
//
// THE ORDER (tests/stats_model.py adds in the same one).
//   1. level share L(k): the 16 terms t0..t15 of the slab, points in memory order p = 4j + i, as the pairwise tree
//        (((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7))) + (((t8 + t9) + (t10 + t11)) + ((t12 + t13) + (t14 + t15)))
//      -- what an xor-butterfly over the lane strides 1, 2, 4, 8 gives in every lane.  Here one lane adds the whole tree of its level.
//   2. element share (per_level = 0): S = L(0); S = S + L(1); ... ascending in k.
// Extrema take the same route.  Every number is a function of the element's own values and of spheremp[e] alone: not of the path of a
// view, of wide or narrow, of the block index, of the other elements or of how elements are dealt to ranks; and the element share is the
// ascending sum of the level shares in every bit.
//
// block = (element, field).  Each view's nk x 16 slab is brought into the LDS image img[v][p][VIEW_PITCH] by that view's own loader, chosen
// by a block-uniform switch on StatsViewArgs::form: the rows of path 1 by dss_rows_to_tile (nk == NLEV), the lines of path 0 and the
// single entries of path 2 with the addressing of k_dss_view_stage.  The arithmetic is one body over the image: lane = level, lanes
// 0..127 the entries without the reference, lanes 128..255 (REF) entries 8 to 13.  One pass over each input; only `out` is written.
constexpr int STATS_N = 16;
enum StatsForm { STATS_LINES_WIDE = 0, STATS_POINTS = 1, STATS_ROWS_WIDE = 2, STATS_ROWS = 3 };
struct StatsViewArgs { const double* ptr[3]; long long vs[3][5]; int form[3]; int nf, nk, per_level; };   // 0 field, 1 ref, 2 weight

__device__ __forceinline__ void stats_load_image(const double* __restrict__ V, const long long* vs, int form, int nk, double* __restrict__ img, int tid) {
  if (form == STATS_ROWS_WIDE) dss_rows_to_tile<true, NLEV>(V, vs[4], img, tid);
  else if (form == STATS_ROWS) dss_rows_to_tile<false, NLEV>(V, vs[4], img, tid);
  else if (form == STATS_LINES_WIDE) {
    constexpr int NI = (NLEVP * 8 + VIEW_THREADS - 1) / VIEW_THREADS;
    const int n = nk * 8;
    double2 r[NI];
#pragma unroll
    for (int u = 0; u < NI; u++) { const int it = min(u * VIEW_THREADS + tid, n - 1); r[u] = *(const double2*)(V + (it >> 3) * vs[2] + 2 * (it & 7)); }
#pragma unroll
    for (int u = 0; u < NI; u++) view_keep(r[u]);
#pragma unroll
    for (int u = 0; u < NI; u++) {
      const int it = u * VIEW_THREADS + tid;
      if (it < n) { double* s = img + 2 * (it & 7) * VIEW_PITCH + (it >> 3); s[0] = r[u].x; s[VIEW_PITCH] = r[u].y; }
    }
  } else {
    constexpr int NI = (NLEVP * 16 + VIEW_THREADS - 1) / VIEW_THREADS;
    const int n = nk * 16;
    double r[NI];
#pragma unroll
    for (int u = 0; u < NI; u++) { const int it = min(u * VIEW_THREADS + tid, n - 1), p = it & 15; r[u] = V[(it >> 4) * vs[2] + (p >> 2) * vs[3] + (p & 3) * vs[4]]; }
#pragma unroll
    for (int u = 0; u < NI; u++) view_keep(r[u]);
#pragma unroll
    for (int u = 0; u < NI; u++) {
      const int it = u * VIEW_THREADS + tid;
      if (it < n) img[(it & 15) * VIEW_PITCH + (it >> 4)] = r[u];
    }
  }
}

// Whether x is NaN or +-inf / whether it is NaN, from its bits.  The library is built with -fno-honor-nans, and the compiler reads an
// exponent test of a double's bits as a floating-point class test, from which it then drops the NaN: the two words pass through an empty
// statement (as view_keep) so that they are integers of unknown origin.
__device__ __forceinline__ void stats_words(double x, unsigned& hi, unsigned& lo) {
  hi = (unsigned)__double2hiint(x); lo = (unsigned)__double2loint(x);
  asm volatile("" : "+v"(hi), "+v"(lo));
}
__device__ __forceinline__ bool stats_nonfinite(double x) {
  unsigned hi, lo;
  stats_words(x, hi, lo);
  return (hi & 0x7ff00000u) == 0x7ff00000u;
}
__device__ __forceinline__ bool stats_nan(double x) {
  unsigned hi, lo;
  stats_words(x, hi, lo);
  return (hi & 0x7ff00000u) == 0x7ff00000u && ((hi & 0x000fffffu) | lo) != 0u;
}
// entry i of a group of N: 0 a sum, 1 a minimum, 2 a maximum
template <int N>
struct StatsAcc {
  double v[N];
  template <class Kind>
  __device__ __forceinline__ StatsAcc plus(const StatsAcc& b, Kind kind) const {
#pragma clang fp contract(off)
    StatsAcc r;
#pragma unroll
    for (int i = 0; i < N; i++) r.v[i] = kind(i) == 0 ? v[i] + b.v[i] : kind(i) == 1 ? fmin(v[i], b.v[i]) : fmax(v[i], b.v[i]);
    return r;
  }
};
// the tree of THE ORDER over the 16 points of one level; term(p) gives the N terms of point p
template <int N, class Term, class Kind>
__device__ __forceinline__ StatsAcc<N> stats_tree(Term term, Kind kind) {
  StatsAcc<N> o[2];
#pragma unroll
  for (int hf = 0; hf < 2; hf++) {
    StatsAcc<N> q[2];
#pragma unroll
    for (int qd = 0; qd < 2; qd++) {
      const int p = 8 * hf + 4 * qd;
      q[qd] = term(p).plus(term(p + 1), kind).plus(term(p + 2).plus(term(p + 3), kind), kind);
    }
    o[hf] = q[0].plus(q[1], kind);
  }
  return o[0].plus(o[1], kind);
}
constexpr int STATS_RED_PITCH = NLEVP;   // the level shares of one entry in the LDS image of the element sum (odd: entries on different banks)
static_assert(9 * STATS_RED_PITCH <= 16 * VIEW_PITCH && 15 * STATS_RED_PITCH <= 2 * 16 * VIEW_PITCH, "the level shares fit the images they replace");
static_assert(NLEVP <= 128, "one lane per level in each half of the block");

template <bool REF, bool WGT>
__global__ __launch_bounds__(VIEW_THREADS) void k_stats_view(StatsViewArgs a, const double* __restrict__ spheremp, double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int NV = 1 + (REF ? 1 : 0) + (WGT ? 1 : 0), IMG = 16 * VIEW_PITCH, IW = REF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) double img[NV * IMG];
  const int tid = threadIdx.x, nk = a.nk;
  const int f = (int)(blockIdx.x % (unsigned)a.nf);
  const long long e = (long long)(blockIdx.x / (unsigned)a.nf);
  stats_load_image(a.ptr[0] + e * a.vs[0][0] + f * a.vs[0][1], a.vs[0], a.form[0], nk, img, tid);
  if (REF) stats_load_image(a.ptr[1] + e * a.vs[1][0] + f * a.vs[1][1], a.vs[1], a.form[1], nk, img + IMG, tid);
  if (WGT) stats_load_image(a.ptr[2] + e * a.vs[2][0], a.vs[2], a.form[2], nk, img + IW * IMG, tid);
  __syncthreads();

  const double inf = __builtin_huge_val();
  const double* sm = spheremp + (size_t)e * 16;
  const int k = tid & 127, half = tid >> 7;
  const bool live = k < nk && (half == 0 || REF);
  const int kc = min(k, nk - 1);
  auto mass = [&](int p) { const double s = sm[p]; return WGT ? s * img[IW * IMG + p * VIEW_PITCH + kc] : s; };
  // entries 0..7 and 14 (lanes 0..127), entries 8..13 (lanes 128..255)
  auto kind0 = [](int i) { return i == 0 ? 1 : (i == 1 || i == 6) ? 2 : 0; };
  auto kind1 = [](int i) { return i >= 4 ? 2 : 0; };
  StatsAcc<9> s0;
  StatsAcc<6> s1;
  if (half == 0) {
    s0 = stats_tree<9>([&](int p) {
#pragma clang fp contract(off)
      const double h = img[p * VIEW_PITCH + kc], m = mass(p), ah = fabs(h);
      const bool nan = stats_nan(h);
      StatsAcc<9> t;
      t.v[0] = nan ? inf : h; t.v[1] = nan ? -inf : h; t.v[2] = h; t.v[3] = m * h; t.v[4] = m * ah; t.v[5] = m * (h * h);
      t.v[6] = nan ? 0.0 : ah; t.v[7] = stats_nonfinite(h) ? 1.0 : 0.0; t.v[8] = m;
      return t;
    }, kind0);
  } else if (REF) {
    s1 = stats_tree<6>([&](int p) {
#pragma clang fp contract(off)
      const double h = img[p * VIEW_PITCH + kc], ht = img[IMG + p * VIEW_PITCH + kc], m = mass(p);
      const double d = h - ht, ad = fabs(d), at = fabs(ht);
      StatsAcc<6> t;
      t.v[0] = m * ad; t.v[1] = m * at; t.v[2] = m * (d * d); t.v[3] = m * (ht * ht);
      t.v[4] = stats_nan(d) ? 0.0 : ad; t.v[5] = stats_nan(ht) ? 0.0 : at;
      return t;
    }, kind1);
  }

  if (a.per_level) {
    if (!live) return;
    double* o = out + (((size_t)e * a.nf + f) * nk + k) * STATS_N;
    if (half == 0) {
#pragma unroll
      for (int i = 0; i < 8; i++) o[i] = s0.v[i];
      o[14] = s0.v[8]; o[15] = 0.0;
      if (!REF) {
#pragma unroll
        for (int i = 8; i < 14; i++) o[i] = 0.0;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 6; i++) o[8 + i] = s1.v[i];
    }
    return;
  }
  // the element share: the level shares go where the images were, red[entry][k]; lane i < 16 adds entry i ascending in k
  __syncthreads();
  double* red = img;
  if (live) {
    if (half == 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) red[i * STATS_RED_PITCH + k] = s0.v[i];
    } else {
#pragma unroll
      for (int i = 0; i < 6; i++) red[(9 + i) * STATS_RED_PITCH + k] = s1.v[i];
    }
  }
  __syncthreads();
  if (tid < STATS_N) {
    // entry tid sits in row: 0..7 -> 0..7, 14 -> 8, 8..13 -> 9..14 (REF), 15 and the absent ones: none
    const int row = tid < 8 ? tid : tid == 14 ? 8 : (REF && tid < 14) ? tid + 1 : -1;
    const int kd = tid == 0 ? 1 : (tid == 1 || tid == 6 || tid == 12 || tid == 13) ? 2 : 0;
    double S = 0.0;
    if (row >= 0) {
      const double* L = red + row * STATS_RED_PITCH;
      S = L[0];
#pragma unroll 8
      for (int kk = 1; kk < nk; kk++) S = kd == 0 ? S + L[kk] : kd == 1 ? fmin(S, L[kk]) : fmax(S, L[kk]);   // (unrolled: eight LDS reads in flight, the additions in order)
    }
    out[((size_t)e * a.nf + f) * STATS_N + tid] = S;
  }
}

// ---- pressure, geopotential and omega / p of a host's columns through strided views (tse_column_view) ------------------------------
// The three vertical scans of the primitive equations, levels from 0 at the model top, n = NLEV (include/transport_se_hip.h states the
// arithmetic; one rounded operation per sign, nothing contracted, tests/column_model.py follows the same lines):
//   COL_PINT   pi[0] = ptop;  pi[k+1] = pi[k] + dp[k]
//   COL_PMID   p[0] = ptop + dp[0]*0.5;  p[k] = (p[k-1] + dp[k-1]*0.5) + dp[k]*0.5
//   COL_PHI    preq_hydrostatic: hkk = (dp*0.5)/p, hkl = 2*hkk, t = rgas*T_v;  phii[n-1] = t*hkl, phii[k] = phii[k+1] + t*hkl;
//              phi[n-1] = phis + t*hkk, phi[k] = (phis + phii[k+1]) + t*hkk
//   COL_OMEGA  preq_omega_ps: ckk = 0.5/p, ckl = 2*ckk;  om[0] = vgrad_p/p - ckk*divdp;  om[k] = (vgrad_p/p - ckl*s) - ckk*divdp with
//              s = divdp[0] + ... + divdp[k-1] added ascending
// PGIVEN: p is a view of the host's; otherwise PHI and OMEGA form PMID's p in LDS with PMID's roundings and it never reaches memory.
//
// block = element.  Each input slab enters an LDS image img[p][VIEW_PITCH] through the loader of its own path (stats_load_image and its
// block-uniform `form`); phis, one level, goes to column NLEV + 1 of the third image.  The work is split by dependence:
//   scans    lanes 0..15, one per point, walk the levels in the image: the additions of pi / p, of phii (upward from the bottom, in place
//            over t*hkl) and of s (an exclusive prefix in place over divdp), eight LDS reads in flight (the rows are read in chunks);
//   points   all 256 lanes, item = p * NLEV + k (consecutive lanes on consecutive doubles of a row: no bank conflict), before a scan the
//            divisions and products -- t*hkl into the image, t*hkk, vgrad_p/p, ckl and ckk*divdp kept in registers across the barrier --
//            and behind it the final combination into the image that leaves.
// The result leaves through the store side of out's path <OPATH, OWIDE>: dss_tile_to_rows for level-fastest rows (n levels alone: the
// n + 1 levels of PINT take the generic path, as tse_dss_view_plan says), lap_view_store_row for lines and points.
// LDS: one image for PINT / PMID, three for PHI / OMEGA.
constexpr int COL_PINT = 0, COL_PMID = 1, COL_PHI = 2, COL_OMEGA = 3;
constexpr int COL_IMG = 16 * VIEW_PITCH, COL_NI = (16 * NLEV + VIEW_THREADS - 1) / VIEW_THREADS, COL_CHUNK = 8;
struct ColumnViewArgs { const double* ptr[4]; long long vs[4][5]; int form[4]; DssViewArgs out; double ptop, rgas; };   // 0 dp, 1 p, 2 a, 3 b
static_assert(3 * COL_IMG * sizeof(double) <= 64 * 1024, "the three images of PHI / OMEGA fit the static LDS of a block");
static_assert(VIEW_PITCH >= NLEV + 2, "a row holds the n + 1 levels of PINT, and phis beside the n levels of T_v");
static_assert(NLEV % COL_CHUNK == 0, "the scans read whole chunks");

// row[k] = dp[k] -> row[k] = pi[k], k = 0..NLEV
__device__ __forceinline__ void col_scan_pint(double* row, double ptop) {
#pragma clang fp contract(off)
  double s = ptop;
  for (int k0 = 0; k0 < NLEV; k0 += COL_CHUNK) {
    double d[COL_CHUNK];
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) d[u] = row[k0 + u];
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) { row[k0 + u] = s; s = s + d[u]; }
  }
  row[NLEV] = s;
}
// row[k] = dp[k] -> dst[k] = p[k]; dst may be row
__device__ __forceinline__ void col_scan_pmid(const double* row, double* dst, double ptop) {
#pragma clang fp contract(off)
  double s = ptop, h = 0.0;
  for (int k0 = 0; k0 < NLEV; k0 += COL_CHUNK) {
    double d[COL_CHUNK];
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) d[u] = row[k0 + u] * 0.5;
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) {
      s = (k0 + u == 0) ? s + d[u] : (s + h) + d[u];
      h = d[u];
      dst[k0 + u] = s;
    }
  }
}
// row[k] = t*hkl of level k -> row[k] = phii[k] for k = NLEV-1 .. 1 (row[0] keeps its product: no phii[0] is formed)
__device__ __forceinline__ void col_scan_phii(double* row) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int k0 = NLEV - COL_CHUNK; k0 >= 0; k0 -= COL_CHUNK) {
    double d[COL_CHUNK];
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) d[u] = row[k0 + u];
#pragma unroll
    for (int u = COL_CHUNK - 1; u >= 0; u--) {
      if (k0 + u == 0) break;
      s = (k0 + u == NLEV - 1) ? d[u] : s + d[u];
      row[k0 + u] = s;
    }
  }
}
// row[k] = divdp[k] -> row[k] = s of level k = divdp[0] + ... + divdp[k-1] for k = 1..NLEV-1 (row[0] is not used)
__device__ __forceinline__ void col_scan_s(double* row) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int k0 = 0; k0 < NLEV; k0 += COL_CHUNK) {
    double d[COL_CHUNK];
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) d[u] = row[k0 + u];
#pragma unroll
    for (int u = 0; u < COL_CHUNK; u++) {
      if (k0 + u > 0) row[k0 + u] = s;
      if (k0 + u < NLEV - 1) s = (k0 + u == 0) ? d[u] : s + d[u];
    }
  }
}

template <int OP, bool PGIVEN, int OPATH, bool OWIDE>
__global__ __launch_bounds__(VIEW_THREADS) void k_column_view(ColumnViewArgs a, double* __restrict__ out) {
#pragma clang fp contract(off)
  static_assert(OP >= COL_PHI || !PGIVEN, "PINT and PMID take no p");
  static_assert(OP != COL_PINT || OPATH != 1, "the n + 1 levels of PINT never take path 1");
  constexpr int NIMG = OP <= COL_PMID ? 1 : 3, NKO = OP == COL_PINT ? NLEVP : NLEV, PHIS = NLEV + 1;
  __shared__ __attribute__((aligned(16))) double img[NIMG * COL_IMG];
  double* const I0 = img;                                   // PINT / PMID: dp -> the result;  PHI: dp -> t*hkl -> phii;  OMEGA: vgrad_p -> om
  double* const I1 = img + (NIMG > 1 ? COL_IMG : 0);        // PHI: p -> phi;  OMEGA: p (or dp -> p)
  double* const I2 = img + (NIMG > 1 ? 2 * COL_IMG : 0);    // PHI: T_v, phis in column PHIS;  OMEGA: divdp -> s
  const int tid = threadIdx.x;
  const long long e = blockIdx.x;
  auto load = [&](int i, int nk, double* dst) { stats_load_image(a.ptr[i] + e * a.vs[i][0], a.vs[i], a.form[i], nk, dst, tid); };
  double* row = nullptr;   // the row of a scanning lane
  const bool scans = tid < 16;

  if (OP <= COL_PMID) {
    load(0, NLEV, I0);
    __syncthreads();
    if (scans) { row = I0 + tid * VIEW_PITCH; if (OP == COL_PINT) col_scan_pint(row, a.ptop); else col_scan_pmid(row, row, a.ptop); }
  } else {
    if (OP == COL_PHI) { load(0, NLEV, I0); if (PGIVEN) load(1, NLEV, I1); load(2, NLEV, I2); load(3, 1, I2 + PHIS); }
    else { load(2, NLEV, I0); load(PGIVEN ? 1 : 0, NLEV, I1); load(3, NLEV, I2); }
    __syncthreads();
    if (!PGIVEN) {
      if (scans) col_scan_pmid((OP == COL_PHI ? I0 : I1) + tid * VIEW_PITCH, I1 + tid * VIEW_PITCH, a.ptop);
      __syncthreads();
    }
    // the independent part in front of the scan; x, y, z: PHI t*hkk | OMEGA vgrad_p/p, ckl, ckk*divdp
    double x[COL_NI], y[COL_NI], z[COL_NI];
#pragma unroll
    for (int u = 0; u < COL_NI; u++) {
      const int it = min(u * VIEW_THREADS + tid, 16 * NLEV - 1), idx = (it / NLEV) * VIEW_PITCH + it % NLEV;
      const double p = I1[idx];
      if (OP == COL_PHI) {
        const double hkk = (I0[idx] * 0.5) / p, hkl = 2.0 * hkk, t = a.rgas * I2[idx];
        x[u] = t * hkk; y[u] = t * hkl;
      } else {
        const double ckk = 0.5 / p;
        x[u] = I0[idx] / p; y[u] = 2.0 * ckk; z[u] = ckk * I2[idx];
      }
    }
    if (OP == COL_PHI) {
#pragma unroll
      for (int u = 0; u < COL_NI; u++) {
        const int it = u * VIEW_THREADS + tid;
        if (it < 16 * NLEV) I0[(it / NLEV) * VIEW_PITCH + it % NLEV] = y[u];
      }
    }
    __syncthreads();
    if (scans) { if (OP == COL_PHI) col_scan_phii(I0 + tid * VIEW_PITCH); else col_scan_s(I2 + tid * VIEW_PITCH); }
    __syncthreads();
    // the final combination: PHI into I1 (p is done with), OMEGA into I0 (vgrad_p is in x)
#pragma unroll
    for (int u = 0; u < COL_NI; u++) {
      const int it = u * VIEW_THREADS + tid, pt = it / NLEV, k = it % NLEV, idx = pt * VIEW_PITCH + k;
      if (it >= 16 * NLEV) continue;
      if (OP == COL_PHI) {
        const double phis = I2[pt * VIEW_PITCH + PHIS];
        const double base = k == NLEV - 1 ? phis : phis + I0[idx + 1];
        I1[idx] = base + x[u];
      } else {
        const double s = I2[idx];
        I0[idx] = k == 0 ? x[u] - z[u] : (x[u] - y[u] * s) - z[u];
      }
    }
  }
  __syncthreads();

  const double* O = OP == COL_PHI ? I1 : I0;
  double* V = out + e * a.out.vs[0];
  if (OPATH == 1) dss_tile_to_rows<OWIDE, NLEV>(O, V, a.out.vs[4], tid);
  else {
    for (int it = tid; it < 4 * NKO; it += VIEW_THREADS) {
      const int j = it & 3, k = it >> 2;
      double r[4];
#pragma unroll
      for (int i = 0; i < 4; i++) r[i] = O[(4 * j + i) * VIEW_PITCH + k];
      lap_view_store_row<OPATH, OWIDE>(V + k * a.out.vs[2], a.out, j, r);
    }
  }
}

}  // namespace tse
