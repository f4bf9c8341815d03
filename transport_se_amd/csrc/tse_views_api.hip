// tse_views_api.hip -- the entries of the C ABI that work on a resident host's own arrays through strided device views: tse_view_put /
// tse_view_get, tse_apply_forcing, tse_remap_view, tse_dss_view, tse_biharmonic_view, tse_vector_setup / tse_vlaplace_view,
// tse_hypervis_view, tse_sphere_op_view, tse_stats_view, tse_column_view.
//
// A translation unit and a code object apart from the tracer path (tse_api.hip): the kernels of tse_view_kernels.h are instantiated
// here (k_column_view in tse_column.hip) and nowhere else, and no kernel that tse_api.hip or tse_stage3.hip instantiates is launched
// from here -- the one the view entries need, k_pack<>, is launched by pack_staged of tse_api.hip.  The context, the error channel
// and the functions of tse_api.hip these entries call are tse_ctx.h's.
#include <cmath>
#include <initializer_list>

#include "tse_ctx.h"
#include "tse_tables.h"
#include "tse_view_launch.h"
#include "tse_views.h"

using namespace tse;

// ---- strided device views: state exchange with a GPU-resident host ------------------------------------
// tse_view_put / tse_view_get (include/transport_se_hip.h).  The descriptor logic -- fields, extents, path, footprint, overlap -- is
// host code (tse_views.cpp); here: the checks that need the runtime, the stream ordering and the launch of one conversion kernel
// (tse_view_kernels.h: k_view_lines, k_view_levels, k_view_generic) on the compute stream.  Nothing is enqueued before every check has passed.
static dim3 view_blocks(size_t items) { return dim3((unsigned)((items + VIEW_THREADS - 1) / VIEW_THREADS)); }   // one item per thread
template <bool PUT>
static void launch_view(tse_ctx* c, const ViewPlan& p, const tse_view* v, double* lib) {
  double* view = (double*)v->ptr;
  const long long* s = v->stride;
  ViewDims d;
  for (int a = 0; a < 5; a++) { d.ext[a] = p.ext[a]; d.lib[a] = p.lib[a]; d.vs[a] = s[a]; }
  const size_t slabs = (size_t)p.ext[0] * p.ext[1] * p.ext[2];
  const bool wide = view_wide(p.path, v);
  if (p.path == 0) {
    if (wide) hipLaunchKernelGGL((k_view_lines<PUT, 2>), view_blocks(slabs * 8), dim3(VIEW_THREADS), 0, c->stream, d, lib, view);
    else hipLaunchKernelGGL((k_view_lines<PUT, 1>), view_blocks(slabs * 16), dim3(VIEW_THREADS), 0, c->stream, d, lib, view);
  } else if (p.path == 1) {
    const dim3 grid((unsigned)((size_t)p.ext[0] * p.ext[1]));
#define TSE_VIEW_LEVELS(W, K) hipLaunchKernelGGL((k_view_levels<PUT, W, K>), grid, dim3(VIEW_THREADS), 0, c->stream, p.ext[1], p.lib[0], p.lib[1], p.lib[2], s[0], s[1], s[4], lib, view)
    if (p.ext[2] == NLEV) { if (wide) TSE_VIEW_LEVELS(true, NLEV); else TSE_VIEW_LEVELS(false, NLEV); }
    else { if (wide) TSE_VIEW_LEVELS(true, NLEVP); else TSE_VIEW_LEVELS(false, NLEVP); }
#undef TSE_VIEW_LEVELS
  } else hipLaunchKernelGGL((k_view_generic<PUT>), view_blocks(slabs * 16), dim3(VIEW_THREADS), 0, c->stream, d, lib, view);
}

// Everything a view entry (tse_view_put, tse_view_get, tse_apply_forcing) checks before it enqueues: the plan of the view, nt, null and
// alignment, the caller's stream (not being captured, on the context's device), the view's memory (device memory of the context's device)
// and its footprint (inside the allocation that holds ptr).  Returns 0 with the plan in *out, or 1 with the message set, under the name `who`.
static int view_runtime_checks(tse_ctx* c, const char* who, const char* field, const ViewPlan& p, const tse_view* v, void* stream, void** alloc);
static int view_checks(tse_ctx* c, const char* who, const char* field, int nt, const tse_view* v, void* stream, bool get, ViewPlan* out) {
  if (!c) return fail("%s: null context", who);
  ViewPlan& p = *out;
  std::string err;
  if (view_plan(field, c->nelemd, c->qsize, v, get, &p, &err)) return fail("%s%s", strcmp(who, "tse_apply_forcing") ? "" : "tse_apply_forcing: ", err.c_str());
  if (p.field == VF_QDP && (nt < 1 || nt > 2)) return fail("%s: nt=%d", who, nt);
  return view_runtime_checks(c, who, field, p, v, stream, nullptr);
}
// the part of view_checks that follows the plan (tse_remap_view makes its own plans); *alloc, if given: the base of the allocation that holds ptr
static int view_runtime_checks(tse_ctx* c, const char* who, const char* field, const ViewPlan& p, const tse_view* v, void* stream, void** alloc) {
  if (!v->ptr) return fail("%s: null view pointer", who);
  if ((uintptr_t)v->ptr & 7) return fail("%s: the view pointer %p is not 8-byte aligned", who, v->ptr);
  if ((size_t)p.ext[0] * p.ext[1] >= ((size_t)1 << 31)) return fail("%s: %d elements x %d", who, p.ext[0], p.ext[1]);
  if ((p.field == VF_Q || p.field == VF_LNPS) && !c->qmix_valid)
    return fail("%s: %s is stale (the state changed since the last tse_state_q, or there was none)", who, field);
  // the caller's stream first: while it is being captured no other runtime call of this thread is safe
  hipStream_t us = (hipStream_t)stream;
  if (us) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(us, &cs) != hipSuccess) { (void)hipGetLastError(); return fail("%s: stream %p is not a stream of this process", who, stream); }
    if (cs != hipStreamCaptureStatusNone) return fail("%s: stream %p is being captured; views are not recorded into graphs", who, stream);
    hipDevice_t sd = 0;
    if (hipStreamGetDevice(us, &sd) != hipSuccess) (void)hipGetLastError();   // (the runtime cannot tell)
    else if ((int)sd != c->device) return fail("%s: stream %p belongs to device %d, the context to device %d", who, stream, (int)sd, c->device);
  }
  // the view's memory: device memory of this device, and every address of the view inside the allocation that holds ptr
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, v->ptr) != hipSuccess) { (void)hipGetLastError(); return fail("%s: %p is not a device address (host memory cannot be viewed)", who, v->ptr); }
  if (at.type != hipMemoryTypeDevice) return fail("%s: %p is not device memory (host memory cannot be viewed)", who, v->ptr);
  if (at.device != c->device) return fail("%s: %p lies on device %d, the context on device %d", who, v->ptr, at.device, c->device);
  hipDeviceptr_t abase = nullptr; size_t asize = 0;
  if (hipMemGetAddressRange(&abase, &asize, (hipDeviceptr_t)v->ptr) != hipSuccess) { (void)hipGetLastError(); return fail("%s: no allocation holds %p", who, v->ptr); }
  if (!Footprint(v, p).inside(Footprint((const void*)abase, asize)))
    return fail("%s: the view reaches doubles [%lld, %lld) around %p, outside its allocation [%p, +%zu bytes)", who, p.lo, p.hi, v->ptr, (void*)abase, asize);
  if (alloc) *alloc = (void*)abase;
  return 0;
}
// One view of an entry that works on the host's own arrays (tse_remap_view, tse_dss_view, tse_biharmonic_view, tse_vlaplace_view).
// who: the name its refusals carry; role: which view of the entry it is ("in", "out"), named by the refusal below alone, or null.
struct HostView { const char *who, *role; const ViewPlan* p; const tse_view* v; };
// view_runtime_checks on every view in turn, and none of them inside an allocation of the library.  own_qdp (tse_remap_view): the first
// view may lie in qdp1 or qdp2, *own_qdp says whether it does.
static int host_array_checks(tse_ctx* c, std::initializer_list<HostView> views, void* stream, bool* own_qdp = nullptr) {
  const std::vector<void*> mine = device_allocations(c);
  for (const HostView& h : views) {
    void* alloc = nullptr;
    if (view_runtime_checks(c, h.who, "field", *h.p, h.v, stream, &alloc)) return 1;
    if (std::find(mine.begin(), mine.end(), alloc) == mine.end()) continue;
    if (own_qdp && &h == views.begin() && (alloc == c->q(1) || alloc == c->q(2))) { *own_qdp = true; continue; }
    return fail("%s%s%s: %p lies inside an allocation of the library%s; the call works on the host's own arrays", h.who, h.role ? ": " : "", h.role ? h.role : "", h.v->ptr,
                own_qdp ? " that is not qdp1 or qdp2 (or is not the field)" : "");
  }
  return 0;
}
// The read-only inputs of an entry (tse_stats_view, tse_column_view): view_runtime_checks on each of the n views that is given, under the
// name who[i] of its role.  Nothing is written through them, so one may lie inside an allocation of the library -- *in_library says
// whether one does -- but not inside `own`, the partials buffer of tse_stats_view (null: the entry has no buffer of its own).
static int input_view_checks(tse_ctx* c, int n, const char* const who[], const ViewPlan p[], const tse_view* const v[], void* stream, const void* own, bool* in_library) {
  const std::vector<void*> mine = device_allocations(c);
  *in_library = false;
  for (int i = 0; i < n; i++) {
    if (!v[i]) continue;
    void* alloc = nullptr;
    if (view_runtime_checks(c, who[i], "field", p[i], v[i], stream, &alloc)) return 1;
    if (own && alloc == own) return fail("%s: %p lies inside the call's own partials buffer", who[i], v[i]->ptr);
    *in_library = *in_library || std::find(mine.begin(), mine.end(), alloc) != mine.end();
  }
  return 0;
}
// ... and their share of the kernel's arguments (StatsViewArgs, ColumnViewArgs): pointer, loader (stats_form) and strides; an absent view
// is a null pointer
template <class Args>
static void input_view_args(Args& a, int n, const ViewPlan p[], const tse_view* const v[]) {
  for (int i = 0; i < n; i++) {
    a.ptr[i] = v[i] ? (const double*)v[i]->ptr : nullptr;
    a.form[i] = v[i] ? stats_form(p[i].path, view_wide(p[i].path, v[i])) : STATS_POINTS;
    for (int k = 0; k < 5; k++) a.vs[i][k] = v[i] ? v[i]->stride[k] : 0;
  }
}

// The stream order of every view entry: the caller's stream -> the compute stream (order_in, behind every check and before the first
// launch) -> the caller's stream (order_out, behind the last launch), with no host synchronisation; without a stream the call is complete
// on return.  The two events are created by the first call that brings a stream.
static int order_in(tse_ctx* c, hipStream_t us) {
  if (!us) return 0;
  if (!c->view_ev[0])
    for (hipEvent_t& e : c->view_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(c->view_ev[0], us)); HIPCHK(hipStreamWaitEvent(c->stream, c->view_ev[0], 0));
  return 0;
}
static int order_out(tse_ctx* c, hipStream_t us) {
  if (us) { HIPCHK(hipEventRecord(c->view_ev[1], c->stream)); HIPCHK(hipStreamWaitEvent(us, c->view_ev[1], 0)); }
  else HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

static int view_io(tse_ctx* c, const char* field, int nt, const tse_view* v, void* stream, bool get) {
  const char* who = get ? "tse_view_get" : "tse_view_put";
  ViewPlan p;
  if (view_checks(c, who, field, nt, v, stream, get, &p)) return 1;
  hipStream_t us = (hipStream_t)stream;

  double* lib = nullptr;
  switch (p.field) {
    case VF_QDP: lib = c->q(nt); break;
    case VF_VN0: lib = c->vn0; break;
    case VF_DP: lib = c->dp; break;
    case VF_ETA: lib = c->eta; break;
    case VF_OMEGA_P: lib = c->omega_p; break;
    case VF_DIVDP: lib = c->divdp; break;
    case VF_DIVDP_PROJ: lib = c->divdp_proj; break;
    case VF_DP3D: lib = c->dp3d; break;
    case VF_PS_V: lib = c->ps_v; break;
    case VF_Q: lib = c->qmix; break;
    case VF_LNPS: lib = c->lnps; break;
  }
  if (!lib) return fail("%s: the library holds no field \"%s\"", who, field);
  if (order_in(c, us)) return 1;
  // the side effects of the host entry that writes the same field (tse_copy_qdp_h2d; tse_set_derived)
  if (!get) {
    if (p.field == VF_QDP || p.field == VF_DP) set_bounds_cache(c, 0);
    if (p.field == VF_DP || p.field == VF_OMEGA_P) c->dcmip_static = false;
  }
  {
    Scope s(c, "view");
    if (get) launch_view<false>(c, p, v, lib); else launch_view<true>(c, p, v, lib);
    LAUNCH_CHECK();
  }
  return order_out(c, us);
}
int tse_view_put(tse_ctx* c, const char* field, int nt, const tse_view* v, void* stream) { return view_io(c, field, nt, v, stream, false); }
int tse_view_get(tse_ctx* c, const char* field, int nt, const tse_view* v, void* stream) { return view_io(c, field, nt, v, stream, true); }

// ---- tracer forcing: Qdp(nt) += FQ of the host, on the device (k_forcing, tse_view_kernels.h) --------------------------
// tse_apply_forcing reads FQ through a view held to the rules of a "qdp" put view (view_checks); tse_apply_forcing_host brings FQ of a
// host-memory elem(:) over by the path of tse_copy_qdp_h2d into the Q field of tse_state_q -- stale after this call anyway, allocated here if
// no tse_state_q has run, so a context that forms Q holds no field more than before -- and runs the same kernel on that dense field.
static int forcing_args(tse_ctx* c, const char* who, int nt, double dt, int mode) {
  if (!c) return fail("%s: null context", who);
  if (mode != TSE_FORCING_TENDENCY && mode != TSE_FORCING_ADJUST) return fail("%s: mode=%d (0: tendency, 1: adjust)", who, mode);
  if (!std::isfinite(dt)) return fail("%s: dt=%g is not finite", who, dt);
  if (nt < 1 || nt > 2) return fail("%s: nt=%d", who, nt);
  return 0;
}
template <int MODE, bool BUDGET>
static void launch_forcing(tse_ctx* c, const ViewPlan& p, const tse_view* v, int nt, double dt, double* budget_d) {
  const long long* s = v->stride;
  const dim3 grid((unsigned)((size_t)c->nelemd * c->qsize));
  with_view_path(p.path, view_wide(p.path, v), [&](auto path, auto wide) {
    hipLaunchKernelGGL((k_forcing<MODE, decltype(path)::value, decltype(wide)::value, BUDGET>), grid, dim3(VIEW_THREADS), 0, c->stream, c->qsize, s[0], s[1], s[2],
                       s[3], s[4], dt, (const double*)c->ps_v, (const double*)c->hyai, (const double*)c->hybi, c->ps0, (const double*)c->spheremp, c->q(nt),
                       (const double*)v->ptr, budget_d);
  });
}
// every check has passed: order behind the caller's stream, launch, hand the order back; with a budget (host [nelemd][qsize][2]) the call
// is complete on return
struct DeviceBuffer { double* p = nullptr; ~DeviceBuffer() { if (p) (void)hipFree(p); } };   // the budget on the device: given back on every return
static int forcing_run(tse_ctx* c, int nt, double dt, int mode, const ViewPlan& p, const tse_view* v, hipStream_t us, double* budget) {
  const size_t nb = (size_t)c->nelemd * c->qsize * 2;
  DeviceBuffer b;
  if (budget && dalloc(&b.p, nb)) return 1;
  double* const bd = b.p;
  if (order_in(c, us)) return 1;
  set_bounds_cache(c, 0);   // the side effects of tse_copy_qdp_h2d: the cached element bounds are dropped, Q / lnps are stale
  {
    Scope s(c, "forcing");
    if (mode == TSE_FORCING_TENDENCY) { if (bd) launch_forcing<0, true>(c, p, v, nt, dt, bd); else launch_forcing<0, false>(c, p, v, nt, dt, bd); }
    else { if (bd) launch_forcing<1, true>(c, p, v, nt, dt, bd); else launch_forcing<1, false>(c, p, v, nt, dt, bd); }
    LAUNCH_CHECK();
  }
  if (!bd) return order_out(c, us);
  if (us && order_out(c, us)) return 1;
  HIPCHK(hipMemcpyAsync(budget, bd, nb * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int tse_apply_forcing(tse_ctx* c, int nt, double dt, int mode, const tse_view* fq, void* stream, double* budget) {
  const char* who = "tse_apply_forcing";
  if (forcing_args(c, who, nt, dt, mode)) return 1;
  ViewPlan p;
  if (view_checks(c, who, "qdp", nt, fq, stream, false, &p)) return 1;
  // FQ is read while Qdp(nt) is written in place: no address of the view may lie inside that field
  if (Footprint(fq, p).meets(Footprint(c->q(nt), c->trc() * 8))) return fail("%s: the view [%p%+lld, %p%+lld doubles) overlaps Qdp(%d), the field it is applied to", who, fq->ptr, p.lo, fq->ptr, p.hi, nt);
  return forcing_run(c, nt, dt, mode, p, fq, (hipStream_t)stream, budget);
}
int tse_apply_forcing_host(tse_ctx* c, int nt, double dt, int mode, const double* fq1, size_t stride, int qsize_d, double* budget) {
  const char* who = "tse_apply_forcing_host";
  if (forcing_args(c, who, nt, dt, mode)) return 1;
  if (!fq1) return fail("%s: null FQ", who);
  if (qsize_d < c->qsize) return fail("%s: qsize_d=%d < qsize=%d", who, qsize_d, c->qsize);
  const size_t per = (size_t)c->qsize * NLEV * 16;   // FQ(np,np,nlev,qsize_d,timelevels): the caller names the time level by the address
  if (stride < per * 8 && c->nelemd > 1) return fail("%s: element stride %zu smaller than the field (%zu bytes)", who, stride, per * 8);
  if (!c->qmix) {
    const hipError_t e = hipMalloc((void**)&c->qmix, c->trc() * 8);
    if (e != hipSuccess) {
      (void)hipGetLastError(); c->qmix = nullptr;
      return fail("%s: cannot allocate the staging field (%.3f GB of device memory): %s", who, c->trc() * 8 / 1e9, hipGetErrorString(e));
    }
  }
  c->qmix_valid = false;   // the Q field is the staging field from here on
  if (copy_field(c, c->qmix, per, (void*)fq1, stride, per, true)) return 1;
  tse_view v;
  v.ptr = c->qmix;
  const long long dense[5] = {(long long)per, (long long)NLEV * 16, 16, 4, 1};
  for (int a = 0; a < 5; a++) v.stride[a] = dense[a];
  ViewPlan p;
  std::string err;
  if (view_plan("qdp", c->nelemd, c->qsize, &v, false, &p, &err)) return fail("%s: %s", who, err.c_str());
  return forcing_run(c, nt, dt, mode, p, &v, nullptr, budget);   // (null stream: complete on return, the caller may reuse FQ)
}

// ---- vertical remap of a resident host's own level fields (k_remap_view_check, k_remap_view: tse_view_kernels.h) ------------------------
// The plans and the overlap test are host code (tse_views.cpp: remap_view_plan); here the checks that need the runtime, the stream order
// of tse_view_put and two launches on the compute stream: the check kernel decides per element whether the bracket search can end on the
// two grids (the test of check_remap_grids, on the device: the grids never visit the host), the remap kernel leaves a refused element alone
// (its instantiation: with_remap_view, tse_view_launch.h).
static int remap_view_buffers(tse_ctx* c) {
  if (c->rv_acc) return 0;
  for (int i = 0; i < 8; i++) {   // (the attribute is per kernel and device; set once per context, before the first launch)
    if (with_remap_view(i & 1, i & 2, i & 4, [](auto kern, size_t lds) -> int {
          HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          return 0;
        })) return 1;
  }
  c->rv_status_ints = REMAP_STATUS;
  if (dalloc(&c->rv_status, (size_t)c->nelemd * REMAP_STATUS) || dalloc(&c->rv_detail, (size_t)c->nelemd * 2)) return 1;
  HIPCHK(hipMemset(c->rv_status, 0, (size_t)c->nelemd * REMAP_STATUS * sizeof(int)));
  unsigned long long* acc = nullptr;
  if (dalloc(&acc, 2)) return 1;
  const unsigned long long clear[2] = {0ull, ~0ull};
  if (hipMemcpy(acc, clear, sizeof clear, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(acc); return fail("tse_remap_view: cannot clear the status"); }
  c->rv_acc = acc;
  return 0;
}

int tse_remap_view(tse_ctx* c, int nf, int mode, int alg, const tse_view* field, const tse_view* dp_src, const tse_view* dp_tgt, void* stream) {
  const char* who = "tse_remap_view";
  if (!c) return fail("%s: null context", who);
  if (mode != TSE_REMAP_MASS && mode != TSE_REMAP_MEAN) return fail("%s: mode=%d (0: mass per layer, 1: layer mean)", who, mode);
  if (alg < 0 || alg > 2) return fail("%s: alg=%d (0|1: mirrored ghost cells, 2: piecewise-constant end cells)", who, alg);
  if (c->nelemd >= (1 << 24)) return fail("%s: %d elements (the status word holds 24 bits of element index)", who, c->nelemd);
  ViewPlan p[3];
  { std::string err; if (remap_view_plan(c->nelemd, nf, field, dp_src, dp_tgt, p, &err)) return fail("%s", err.c_str()); }
  // the library's own memory: only its Qdp, and only as the field (a host with real dynamics remaps the engine's tracers on its own grids)
  bool own_qdp = false;
  if (host_array_checks(c, {{"tse_remap_view: field", nullptr, &p[0], field}, {"tse_remap_view: dp_src", nullptr, &p[1], dp_src},
                            {"tse_remap_view: dp_tgt", nullptr, &p[2], dp_tgt}}, stream, &own_qdp)) return 1;
  { std::string err; if (remap_view_overlap(field, dp_src, dp_tgt, p, &err)) return fail("%s", err.c_str()); }
  if (remap_view_buffers(c)) return 1;
  hipStream_t us = (hipStream_t)stream;

  RemapViewArgs a;
  a.field = (double*)field->ptr; a.src = (const double*)dp_src->ptr; a.tgt = (const double*)dp_tgt->ptr;
  for (int k = 0; k < 5; k++) { a.fs[k] = field->stride[k]; a.ss[k] = dp_src->stride[k]; a.ts[k] = dp_tgt->stride[k]; }
  a.spath = p[1].path; a.tpath = p[2].path;
  // level-fastest rows whose chunks of CL levels are 16-byte aligned in every column; the kernel has no wide form of path 0
  const bool wide = p[0].path == 1 && view_wide(1, field);
  const bool mean = mode == TSE_REMAP_MEAN;

  if (order_in(c, us)) return 1;
  if (own_qdp) set_bounds_cache(c, 0);   // the side effects of tse_copy_qdp_h2d
  {
    Scope sc(c, "fieldremap");
    hipLaunchKernelGGL(k_remap_view_check<>, dim3(c->nelemd), dim3(REMAP_CHECK_THREADS), 0, c->stream, a, (int)mean, c->rv_status, c->rv_detail,
                       us ? c->rv_acc : (unsigned long long*)nullptr, c->rv_seq & 0xffffffu);
    with_remap_view(alg == 2, mean, wide, [&](auto kern, size_t lds) -> int {
      hipLaunchKernelGGL(kern, dim3(c->nelemd), dim3(REMAP_THREADS), lds, c->stream, nf, a, (const int*)c->rv_status);
      return 0;
    });
    LAUNCH_CHECK();
  }
  if (us) {
    c->rv_seq++;
    return order_out(c, us);
  }
  // complete on return: the verdicts come back, the lowest refused element is named
  std::vector<int> st((size_t)c->nelemd * REMAP_STATUS);
  HIPCHK(hipMemcpyAsync(st.data(), c->rv_status, st.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  int nref = 0, first = -1;
  for (int e = 0; e < c->nelemd; e++)
    if (st[(size_t)e * REMAP_STATUS]) { nref++; if (first < 0) first = e; }
  if (!nref) return 0;
  double det[2];
  HIPCHK(hipMemcpy(det, c->rv_detail + (size_t)first * 2, sizeof det, hipMemcpyDeviceToHost));
  RemapGridFault f;
  f.code = st[(size_t)first * REMAP_STATUS]; f.level = st[(size_t)first * REMAP_STATUS + 2]; f.has_limit = st[(size_t)first * REMAP_STATUS + 3];
  f.value = det[0]; f.limit = det[1];
  fail("%s: %d of %d elements refused and left as they were; the first: %s", who, nref, c->nelemd,
       remap_grid_message(first, st[(size_t)first * REMAP_STATUS + 1], f, mean).c_str());
  return 2;
}

int tse_remap_view_status(tse_ctx* c, int* nrefused, int where[4]) {
  if (!c) return fail("tse_remap_view_status: null context");
  if (nrefused) *nrefused = 0;
  if (where) where[0] = where[1] = where[2] = where[3] = 0;
  if (!c->rv_acc) return 0;   // no tse_remap_view yet
  HIPCHK(hipStreamSynchronize(c->stream));
  unsigned long long acc[2] = {0ull, ~0ull};
  HIPCHK(hipMemcpy(acc, c->rv_acc, sizeof acc, hipMemcpyDeviceToHost));
  if (acc[0]) {
    const unsigned long long clear[2] = {0ull, ~0ull};
    HIPCHK(hipMemcpy(c->rv_acc, clear, sizeof clear, hipMemcpyHostToDevice));
    if (nrefused) *nrefused = (int)std::min<unsigned long long>(acc[0], 0x7fffffffull);
    if (where) { where[0] = (int)((acc[1] >> 16) & 0xffffffull); where[1] = (int)((acc[1] >> 12) & 15ull); where[2] = (int)((acc[1] >> 4) & 255ull); where[3] = (int)(acc[1] & 15ull); }
  }
  c->rv_seq = 0;
  return 0;
}

// ---- DSS of a resident host's own fields (k_dss_view_stage, k_dss_view_sum: tse_view_kernels.h) -----------------------------------------
// The plan is host code (tse_views.cpp: dss_view_plan); here the checks that need the runtime and one call of stage_exchange_out, which
// tse_biharmonic_view and tse_vlaplace_view share: the stream order of tse_view_put, and on the compute stream
// stage -> (pack -> halo_exchange kind 0 with nl = nf * nk layers, on a rank with neighbours) -> out.  The staging field and the halo
// buffers are these calls' own; a steady-state call allocates nothing.
// second (tse_hypervis_view): the second staging field too, grown by the same rule
static int dss_view_buffers(tse_ctx* c, size_t nl, bool second = false) {
  if (second && nl > c->hv_layers) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->hv_stage) (void)hipFree(c->hv_stage);
    c->hv_stage = nullptr; c->hv_layers = 0;
    if (dalloc(&c->hv_stage, (size_t)c->nelemd * nl * 16)) return 1;
    c->hv_layers = nl;
  }
  if (nl <= c->dv_layers) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));   // (an earlier call may still read the buffers that are given back)
  double** bufs[3] = {&c->dv_stage, &c->dv_send, &c->dv_recv};
  for (double** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
  c->dv_layers = 0;
  if (dalloc(&c->dv_stage, (size_t)c->nelemd * nl * 16)) return 1;
  if (c->halo() && (dalloc(&c->dv_send, (size_t)std::max(1, c->ncol_send) * nl) || dalloc(&c->dv_recv, (size_t)std::max(1, c->ncol_recv) * nl))) return 1;
  c->dv_layers = nl;
  return 0;
}
static DssViewArgs dss_view_args(int nf, int nk, const tse_view* v) {
  DssViewArgs a;
  for (int k = 0; k < 5; k++) a.vs[k] = v->stride[k];
  a.nf = nf; a.nk = nk; a.base = 0; a.nl = nf * nk;
  return a;
}
// the staged field's rank-boundary columns to the neighbour ranks and theirs into dv_recv; staged: dv_stage, or tse_hypervis_view's second field
static int stage_exchange(tse_ctx* c, size_t nl, unsigned pack_blocks, const double* staged = nullptr) {
  CommScope w(c, "comm_wait", c->stream);   // (on the compute stream: the whole exchange is exposed)
  if (c->ncol_send && pack_staged(c, c->stream, staged ? staged : c->dv_stage, (int)nl, pack_blocks, c->dv_send)) return 1;   // (k_pack<> is tse_api.hip's)
  return halo_exchange(c, (int)nl, 0, c->stream, c->dv_send, c->dv_recv);
}
// What follows the checks of the three entries.  group: the timer group of the two kernels; exchange: whether the staged field goes to
// the neighbour ranks in between; stage / out: launch the entry's two kernels on the compute stream.
template <class Stage, class Out>
static int stage_exchange_out(tse_ctx* c, const char* group, size_t nl, bool exchange, hipStream_t us, Stage&& stage, Out&& out) {
  unsigned pack_blocks = 0;
  if (exchange && c->ncol_send && halo_items((size_t)c->ncol_send * nl, &pack_blocks)) return 1;
  if (dss_view_buffers(c, nl)) return 1;
  if (order_in(c, us)) return 1;
  {
    Scope sc(c, group);
    stage();
    LAUNCH_CHECK();
  }
  if (exchange && stage_exchange(c, nl, pack_blocks)) return 1;
  {
    Scope sc(c, group);
    out();
    LAUNCH_CHECK();
  }
  return order_out(c, us);
}
// the grid of a kernel's level-fastest path: one (element, field) tile per block, for the second kernel the elements padded to groups of 8
static dim3 view_tiles(int nelemd, int nf, bool padded) { return dim3((unsigned)((padded ? 8ll * ((nelemd + 7) >> 3) : (long long)nelemd) * nf)); }

template <int MODE>
static void launch_dss_view_stage(tse_ctx* c, int path, bool wide, const DssViewArgs& a, const double* view) {
  const size_t slabs = (size_t)c->nelemd * a.nf * a.nk;
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    constexpr bool W = decltype(wc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, a.nf, false) : view_blocks(slabs * (W ? 8 : 16));
    hipLaunchKernelGGL((k_dss_view_stage<PATH, W, MODE>), grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, (const double*)c->spheremp, view, c->dv_stage);
  });
}
static void launch_dss_view_sum(tse_ctx* c, int path, bool wide, const DssViewArgs& a, double* view) {
  const long long nl = (long long)a.nf * a.nk;
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    constexpr bool W = decltype(wc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, a.nf, true) : dim3((unsigned)dss_view_sum_blocks(c->nelemd, nl * (W ? 8 : 16)));
    hipLaunchKernelGGL((k_dss_view_sum<PATH, W>), grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, (const int2*)c->dss_tab, (const double*)c->rspheremp,
                       (const double*)c->dv_stage, (const double*)c->dv_recv, (const int*)c->order, view);
  });
}

int tse_dss_view(tse_ctx* c, int nf, int nk, int mode, const tse_view* field, void* stream) {
  const char* who = "tse_dss_view";
  if (!c) return fail("%s: null context", who);
  if (mode != TSE_DSS_AVERAGE && mode != TSE_DSS_WEAK) return fail("%s: mode=%d (0: average, f <- rspheremp * DSS(spheremp * f); 1: weak, f <- rspheremp * DSS(f))", who, mode);
  ViewPlan p;
  { std::string err; if (dss_view_plan(c->nelemd, nf, nk, field, &p, &err)) return fail("%s", err.c_str()); }
  const size_t nl = (size_t)nf * nk;
  if ((size_t)c->nelemd * nl >= ((size_t)1 << 27)) return fail("%s: %d elements x %zu layers (the launches count 32-bit blocks)", who, c->nelemd, nl);
  if (host_array_checks(c, {{who, nullptr, &p, field}}, stream)) return 1;
  const DssViewArgs a = dss_view_args(nf, nk, field);
  const bool wide = view_wide(p.path, field);
  return stage_exchange_out(c, "fielddss", nl, c->halo(), (hipStream_t)stream,
    [&] { if (mode == TSE_DSS_AVERAGE) launch_dss_view_stage<0>(c, p.path, wide, a, (const double*)field->ptr); else launch_dss_view_stage<1>(c, p.path, wide, a, (const double*)field->ptr); },
    [&] { launch_dss_view_sum(c, p.path, wide, a, (double*)field->ptr); });
}

// ---- weak Laplacian / biharmonic of a resident host's own scalar fields (k_lap_view_stage, k_lap_view_out: tse_view_kernels.h) ------------
// The plan is host code (tse_views.cpp: biharmonic_view_plan / biharmonic_view_overlap); here the checks that need the runtime and
// stage_exchange_out with tse_dss_view's buffers; the exchange for order 2 alone.
static void launch_lap_view_stage(tse_ctx* c, int path, bool wide, const DssViewArgs& a, const double* view) {
  const long long quads = (long long)c->nelemd * lap_view_groups((long long)a.nf * a.nk);
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, a.nf, false) : view_blocks((size_t)quads * 4);
    hipLaunchKernelGGL((k_lap_view_stage<PATH, decltype(wc)::value>), grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, c->D, c->geo(), view, c->dv_stage);
  });
}
template <int ORDER>
static void launch_lap_view_out(tse_ctx* c, int path, bool wide, const DssViewArgs& a, double* view) {
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, a.nf, true) : dim3((unsigned)lap_view_out_blocks(c->nelemd, (long long)a.nf * a.nk));
    hipLaunchKernelGGL((k_lap_view_out<PATH, decltype(wc)::value, ORDER>), grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, c->D, c->geo(),
                       (const int2*)c->dss_tab, (const double*)c->dv_stage, (const double*)c->dv_recv, (const int*)c->order, view);
  });
}

int tse_biharmonic_view(tse_ctx* c, int nf, int nk, int order, const tse_view* in, const tse_view* out, void* stream) {
  const char* who = "tse_biharmonic_view";
  if (!c) return fail("%s: null context", who);
  if (order != TSE_LAPLACE && order != TSE_BIHARMONIC)
    return fail("%s: order=%d (1: out = laplace_sphere_wk(in); 2: out = laplace_sphere_wk(rspheremp * DSS(laplace_sphere_wk(in))))", who, order);
  ViewPlan p[2];
  { std::string err; if (biharmonic_view_plan(c->nelemd, nf, nk, in, out, p, &err)) return fail("%s", err.c_str()); }
  const size_t nl = (size_t)nf * nk;
  if ((size_t)c->nelemd * nl >= ((size_t)1 << 27)) return fail("%s: %d elements x %zu layers (the launches count 32-bit blocks)", who, c->nelemd, nl);
  if (host_array_checks(c, {{who, "in", &p[0], in}, {who, "out", &p[1], out}}, stream)) return 1;
  { std::string err; if (biharmonic_view_overlap(in, out, p, &err)) return fail("%s", err.c_str()); }
  const DssViewArgs ai = dss_view_args(nf, nk, in), ao = dss_view_args(nf, nk, out);
  const bool wi = view_wide(p[0].path, in), wo = view_wide(p[1].path, out);
  return stage_exchange_out(c, "fieldlap", nl, order == TSE_BIHARMONIC && c->halo(), (hipStream_t)stream,
    [&] { launch_lap_view_stage(c, p[0].path, wi, ai, (const double*)in->ptr); },
    [&] { if (order == TSE_LAPLACE) launch_lap_view_out<1>(c, p[1].path, wo, ao, (double*)out->ptr); else launch_lap_view_out<2>(c, p[1].path, wo, ao, (double*)out->ptr); });
}

// ---- weak vector Laplacian / biharmonic of a resident host's own wind (k_vec_fold, k_vlap_view_stage, k_vlap_view_out: tse_view_kernels.h) ----
// tse_vector_setup: elem%D, elem%metinv, elem%mp -> [e][p][9] on the device -> the folded tables (allocated once; a later call overwrites them)
int tse_vector_setup(tse_ctx* c, const double* D, size_t D_stride, const double* metinv, size_t metinv_stride, const double* mp, size_t mp_stride) {
  if (!c) return fail("tse_vector_setup: null context");
  if (!D || !metinv || !mp) return fail("tse_vector_setup: null argument");
  const int n = c->nelemd;
  std::vector<double> d, m, w, h((size_t)n * 16 * 9);
  gather_strided(d, D, D_stride, n, 64);
  gather_strided(m, metinv, metinv_stride, n, 64);
  gather_strided(w, mp, mp_stride, n, 16);
  for (size_t t = 0; t < (size_t)n * 16; t++) {
    for (int k = 0; k < 4; k++) { h[t * 9 + k] = d[t * 4 + k]; h[t * 9 + 4 + k] = m[t * 4 + k]; }
    h[t * 9 + 8] = w[t];
  }
  if (!c->vec_tab && dalloc(&c->vec_tab, (size_t)n * VEC_TABS * 16)) return 1;
  c->vec_ready = false;
  HIPCHK(hipStreamSynchronize(c->stream));   // (a kernel still running reads the old tables)
  double* src = nullptr;
  if (upload(&src, h)) return 1;
  hipLaunchKernelGGL(k_vec_fold<>, dim3((unsigned)(((size_t)n * 16 + 255) / 256)), dim3(256), 0, c->stream, n, c->geo(), (const double*)src, c->vec_tab);
  const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(c->stream);
  (void)hipFree(src);
  HIPCHK(launched); HIPCHK(done);
  c->vec_ready = true;
  return 0;
}
// (the kernels take both components of a level at once: a tile is an element)
static void launch_vlap_view_stage(tse_ctx* c, int path, bool wide, const DssViewArgs& a, double nu_ratio, const double* view) {
  const long long quads = (long long)c->nelemd * vlap_view_groups(a.nk);
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, 1, false) : view_blocks((size_t)quads * 4);
    hipLaunchKernelGGL((k_vlap_view_stage<PATH, decltype(wc)::value>), grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, c->D, c->geo(),
                       (const double*)c->vec_tab, nu_ratio, view, c->dv_stage);
  });
}
template <int ORDER>
static void launch_vlap_view_out(tse_ctx* c, int path, bool wide, const DssViewArgs& a, double nu_ratio, double* view) {
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, 1, true) : dim3((unsigned)vlap_view_out_blocks(c->nelemd, a.nk));
    hipLaunchKernelGGL((k_vlap_view_out<PATH, decltype(wc)::value, ORDER>), grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, c->D, c->geo(),
                       (const double*)c->vec_tab, nu_ratio, (const int2*)c->dss_tab, (const double*)c->dv_stage, (const double*)c->dv_recv, (const int*)c->order, view);
  });
}

// As tse_biharmonic_view with nf = 2 (the plan is vlaplace_view_plan, tse_views.cpp).
int tse_vlaplace_view(tse_ctx* c, int nk, int order, double nu_ratio, const tse_view* in, const tse_view* out, void* stream) {
  const char* who = "tse_vlaplace_view";
  if (!c) return fail("%s: null context", who);
  if (order != TSE_VLAPLACE && order != TSE_VBIHARMONIC)
    return fail("%s: order=%d (1: out = vlaplace_sphere_wk(in); 2: out = vlaplace_sphere_wk(rspheremp * DSS(vlaplace_sphere_wk(in))))", who, order);
  if (!std::isfinite(nu_ratio)) return fail("%s: nu_ratio = %g is not finite", who, nu_ratio);
  if (!c->vec_ready) return fail("%s: call tse_vector_setup first (elem%%D, elem%%metinv and elem%%mp are not part of tse_init_args)", who);
  ViewPlan p[2];
  { std::string err; if (vlaplace_view_plan(c->nelemd, nk, in, out, p, &err)) return fail("%s", err.c_str()); }
  const size_t nl = (size_t)2 * nk;
  if ((size_t)c->nelemd * nl >= ((size_t)1 << 27)) return fail("%s: %d elements x %zu layers (the launches count 32-bit blocks)", who, c->nelemd, nl);
  if (host_array_checks(c, {{who, "in", &p[0], in}, {who, "out", &p[1], out}}, stream)) return 1;
  { std::string err; if (biharmonic_view_overlap(in, out, p, &err, who)) return fail("%s", err.c_str()); }
  const DssViewArgs ai = dss_view_args(2, nk, in), ao = dss_view_args(2, nk, out);
  const bool wi = view_wide(p[0].path, in), wo = view_wide(p[1].path, out);
  return stage_exchange_out(c, "fieldvlap", nl, order == TSE_VBIHARMONIC && c->halo(), (hipStream_t)stream,
    [&] { launch_vlap_view_stage(c, p[0].path, wi, ai, nu_ratio, (const double*)in->ptr); },
    [&] { if (order == TSE_VLAPLACE) launch_vlap_view_out<1>(c, p[1].path, wo, ao, nu_ratio, (double*)out->ptr); else launch_vlap_view_out<2>(c, p[1].path, wo, ao, nu_ratio, (double*)out->ptr); });
}

// ---- one hyperviscosity sub-step of a resident host's scalars and wind (k_lap_view_mid, k_vlap_view_mid, k_dss_view_final: tse_view_kernels.h) ----
// The plans and the overlap rule are host code (tse_views.cpp: hypervis_view_plan / hypervis_view_overlap); here the checks that need the
// runtime, the stream order of tse_view_put and on the compute stream
//   stage (scalars, wind) -> exchange -> mid (scalars, wind) -> exchange -> final
// with the scalars' and the wind's layers in ONE staging field, so that each exchange is one halo_exchange of nl = (nf + 2) * nk layers.
// Both exchanges use dv_send / dv_recv: every step is ordered on the compute stream (halo_exchange enqueues its receives and sends there,
// or drains it before the callback), so the second pack follows the first exchange's sends and the second receive follows the mid
// kernels, the only readers of what the first one brought.
static HvSide hv_side(const DssViewArgs& a, int path, const tse_view* v) {
  HvSide s;
  s.a = a; s.x = (double*)v->ptr;
  const bool wide = view_wide(path, v);
  s.form = path == 1 ? (wide ? HV_ROWS_WIDE : HV_ROWS) : path == 0 && wide ? HV_LINES_WIDE : HV_POINTS;
  return s;
}
static unsigned hv_side_blocks(int nelemd, const HvSide& s) {
  if (s.form >= HV_ROWS_WIDE) return view_tiles(nelemd, s.a.nf, true).x;
  return (unsigned)dss_view_sum_blocks(nelemd, (long long)s.a.nf * s.a.nk * (s.form == HV_LINES_WIDE ? 8 : 16));
}

int tse_hypervis_view(tse_ctx* c, int nf, int nk, const double* coef, double nu_ratio, const tse_view* s, const tse_view* v, const tse_view* s_out,
                      const tse_view* v_out, void* stream) {
  const char* who = "tse_hypervis_view";
  if (!c) return fail("%s: null context", who);
  if (!coef) return fail("%s: null coef", who);
  if (!std::isfinite(nu_ratio)) return fail("%s: nu_ratio = %g is not finite", who, nu_ratio);
  ViewPlan p[4];
  { std::string err; if (hypervis_view_plan(c->nelemd, nf, nk, s, v, s_out, v_out, p, &err)) return fail("%s", err.c_str()); }
  for (int f = 0; f < nf + (v ? 1 : 0); f++)
    if (!std::isfinite(coef[f])) return fail("%s: coef[%d] = %g is not finite (%s)", who, f, coef[f], f < nf ? "a scalar field's factor" : "the wind's factor");
  if (v && !c->vec_ready) return fail("%s: call tse_vector_setup first (elem%%D, elem%%metinv and elem%%mp are not part of tse_init_args)", who);
  const tse_view* x[4] = {s, v, s_out, v_out};
  static const char* const role[4] = {"s", "v", "s_out", "v_out"};
  for (int i = 0; i < 4; i++)
    if (x[i] && host_array_checks(c, {{who, role[i], &p[i], x[i]}}, stream)) return 1;
  { std::string err; if (hypervis_view_overlap(x, p, &err)) return fail("%s", err.c_str()); }

  const int ns = nf * nk, nlt = ns + (v ? 2 * nk : 0);
  const size_t nl = (size_t)nlt;
  const bool add = !s_out && !v_out, exchange = c->halo();
  DssViewArgs as = {}, av = {};
  if (s) { as = dss_view_args(nf, nk, s); as.nl = nlt; }
  if (v) { av = dss_view_args(2, nk, v); av.base = ns; av.nl = nlt; }
  HvCoef cf = {};
  for (int f = 0; f < nf; f++) cf.c[f] = coef[f];
  const double cv = v ? coef[nf] : 0.0;
  // the final kernel's two sides: the views that are written
  HvFinalArgs fa = {};
  fa.blocks0 = 0;
  if (s) {
    const tse_view* w = add ? s : s_out;
    DssViewArgs a = dss_view_args(nf, nk, w); a.nl = nlt;
    fa.side[0] = hv_side(a, p[add ? 0 : 2].path, w);
    fa.blocks0 = hv_side_blocks(c->nelemd, fa.side[0]);
  }
  unsigned blocks1 = 0;
  if (v) {
    const tse_view* w = add ? v : v_out;
    DssViewArgs a = dss_view_args(2, nk, w); a.base = ns; a.nl = nlt;
    fa.side[1] = hv_side(a, p[add ? 1 : 3].path, w);
    blocks1 = hv_side_blocks(c->nelemd, fa.side[1]);
  }

  hipStream_t us = (hipStream_t)stream;
  unsigned pack_blocks = 0;
  if (exchange && c->ncol_send && halo_items((size_t)c->ncol_send * nl, &pack_blocks)) return 1;
  if (dss_view_buffers(c, nl, true)) return 1;
  if (order_in(c, us)) return 1;
  if (s) {
    Scope sc(c, "fieldhv");
    launch_lap_view_stage(c, p[0].path, view_wide(p[0].path, s), as, (const double*)s->ptr);
    LAUNCH_CHECK();
  }
  if (v) {
    Scope sc(c, "fieldhv");
    launch_vlap_view_stage(c, p[1].path, view_wide(p[1].path, v), av, nu_ratio, (const double*)v->ptr);
    LAUNCH_CHECK();
  }
  if (exchange && stage_exchange(c, nl, pack_blocks)) return 1;
  if (s) {
    Scope sc(c, "fieldhv");
    hipLaunchKernelGGL(k_lap_view_mid<>, dim3((unsigned)lap_view_out_blocks(c->nelemd, ns)), dim3(VIEW_THREADS), 0, c->stream, c->nelemd, nf, nk, nlt, cf, c->D, c->geo(),
                       (const int2*)c->dss_tab, (const double*)c->dv_stage, (const double*)c->dv_recv, (const int*)c->order, c->hv_stage);
    LAUNCH_CHECK();
  }
  if (v) {
    Scope sc(c, "fieldhv");
    hipLaunchKernelGGL(k_vlap_view_mid<>, dim3((unsigned)vlap_view_out_blocks(c->nelemd, nk)), dim3(VIEW_THREADS), 0, c->stream, c->nelemd, nk, ns, nlt, cv, c->D, c->geo(),
                       (const double*)c->vec_tab, nu_ratio, (const int2*)c->dss_tab, (const double*)c->dv_stage, (const double*)c->dv_recv, (const int*)c->order,
                       c->hv_stage);
    LAUNCH_CHECK();
  }
  if (exchange && stage_exchange(c, nl, pack_blocks, c->hv_stage)) return 1;
  {
    Scope sc(c, "fieldhv");
    const dim3 grid(fa.blocks0 + blocks1);
    if (add) hipLaunchKernelGGL(k_dss_view_final<true>, grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, fa, (const int2*)c->dss_tab, (const double*)c->rspheremp,
                                (const double*)c->hv_stage, (const double*)c->dv_recv, (const int*)c->order);
    else hipLaunchKernelGGL(k_dss_view_final<false>, grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, fa, (const int2*)c->dss_tab, (const double*)c->rspheremp,
                            (const double*)c->hv_stage, (const double*)c->dv_recv, (const int*)c->order);
    LAUNCH_CHECK();
  }
  return order_out(c, us);
}

// ---- gradient, divergence and vorticity of a resident host's own fields, local or C0 (k_sphere_op_stage: tse_view_kernels.h) ------------
// The plan is host code (tse_views.cpp: sphere_op_view_plan / sphere_op_view_overlap).  The stage kernel is the entry's own; the out
// kernel is tse_dss_view's sum (C0) or tse_biharmonic_view's own-line copy (LOCAL), each with the nf_out fields of `out`.
static void launch_sphere_op_stage(tse_ctx* c, int path, bool wide, int op, bool c0, const DssViewArgs& a, const double* view) {
  const long long quads = (long long)c->nelemd * sphere_op_groups(a.nk);
  with_view_path(path, wide, [&](auto pc, auto wc) {
    constexpr int PATH = decltype(pc)::value;
    constexpr bool W = decltype(wc)::value;
    const dim3 grid = PATH == 1 ? view_tiles(c->nelemd, 1, false) : view_blocks((size_t)quads * 4);
    auto go = [&](auto k) {
      hipLaunchKernelGGL(k, grid, dim3(VIEW_THREADS), 0, c->stream, c->nelemd, a, c->D, c->geo(), (const double*)c->vec_tab, view, c->dv_stage);
    };
    if (op == TSE_OP_GRADIENT) { if (c0) go(k_sphere_op_stage<PATH, W, 0, true>); else go(k_sphere_op_stage<PATH, W, 0, false>); }
    else if (op == TSE_OP_DIVERGENCE) { if (c0) go(k_sphere_op_stage<PATH, W, 1, true>); else go(k_sphere_op_stage<PATH, W, 1, false>); }
    else { if (c0) go(k_sphere_op_stage<PATH, W, 2, true>); else go(k_sphere_op_stage<PATH, W, 2, false>); }
  });
}

int tse_sphere_op_view(tse_ctx* c, int nk, int op, int c0, const tse_view* in, const tse_view* out, void* stream) {
  const char* who = "tse_sphere_op_view";
  if (!c) return fail("%s: null context", who);
  if (c0 != TSE_OP_LOCAL && c0 != TSE_OP_C0) return fail("%s: c0=%d (0: out = op(in); 1: out = rspheremp * DSS(spheremp * op(in)))", who, c0);
  ViewPlan p[2];
  { std::string err; if (sphere_op_view_plan(c->nelemd, nk, op, in, out, p, &err)) return fail("%s", err.c_str()); }
  if (op == TSE_OP_VORTICITY && !c->vec_ready) return fail("%s: TSE_OP_VORTICITY: call tse_vector_setup first (elem%%D is not part of tse_init_args)", who);
  int nfi = 0, nfo = 0;
  sphere_op_fields(op, &nfi, &nfo);
  const size_t nl = (size_t)nfo * nk;
  if ((size_t)c->nelemd * 2 * nk >= ((size_t)1 << 27)) return fail("%s: %d elements x %d layers (the launches count 32-bit blocks)", who, c->nelemd, 2 * nk);
  if (host_array_checks(c, {{who, "in", &p[0], in}, {who, "out", &p[1], out}}, stream)) return 1;
  { std::string err; if (sphere_op_view_overlap(in, out, p, &err)) return fail("%s", err.c_str()); }
  const DssViewArgs ai = dss_view_args(nfi, nk, in), ao = dss_view_args(nfo, nk, out);
  const bool wi = view_wide(p[0].path, in), wo = view_wide(p[1].path, out);
  return stage_exchange_out(c, "fieldop", nl, c0 == TSE_OP_C0 && c->halo(), (hipStream_t)stream,
    [&] { launch_sphere_op_stage(c, p[0].path, wi, op, c0 == TSE_OP_C0, ai, (const double*)in->ptr); },
    [&] { if (c0 == TSE_OP_C0) launch_dss_view_sum(c, p[1].path, wo, ao, (double*)out->ptr); else launch_lap_view_out<1>(c, p[1].path, wo, ao, (double*)out->ptr); });
}

// ---- min, max, sums and integrals of a resident host's fields (k_stats_view: tse_view_kernels.h) ------------------------------------------
// The plans are host code (tse_views.cpp: stats_view_plan); here the checks that need the runtime -- those of tse_dss_view, except that a
// view may lie inside an allocation of the library (nothing is written through it) -- the stream order of tse_view_put, one launch on the
// compute stream and the copy of the shares to the host: the call is complete on return.  The partials buffer is the call's own.
int tse_stats_view(tse_ctx* c, int nf, int nk, int per_level, const tse_view* field, const tse_view* ref, const tse_view* weight, void* stream, double* out) {
  const char* who = "tse_stats_view";
  if (!c) return fail("%s: null context", who);
  if (!out) return fail("%s: null out", who);
  if (per_level != 0 && per_level != 1) return fail("%s: per_level=%d (0: one share per element and field, 1: one per level)", who, per_level);
  ViewPlan p[3];
  { std::string err; if (stats_view_plan(c->nelemd, nf, nk, field, ref, weight, p, &err)) return fail("%s", err.c_str()); }
  const size_t n = (size_t)c->nelemd * nf * (per_level ? nk : 1) * STATS_N;
  if ((size_t)c->nelemd * nf >= ((size_t)1 << 31)) return fail("%s: %d elements x %d fields (the launch counts 32-bit blocks)", who, c->nelemd, nf);
  const tse_view* v[3] = {field, ref, weight};
  bool in_library = false;
  const char* const role[3] = {"tse_stats_view (field)", "tse_stats_view (ref)", "tse_stats_view (weight)"};   // the name a runtime refusal carries
  if (input_view_checks(c, 3, role, p, v, stream, c->st_part, &in_library)) return 1;
  if (n > c->st_cap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->st_part) (void)hipFree(c->st_part);
    c->st_part = nullptr; c->st_cap = 0;
    if (dalloc(&c->st_part, n)) return 1;
    c->st_cap = n;
  }
  StatsViewArgs a;
  input_view_args(a, 3, p, v);
  a.nf = nf; a.nk = nk; a.per_level = per_level;
  hipStream_t us = (hipStream_t)stream;
  if (order_in(c, us)) return 1;
  if (in_library && join_inputs(c)) return 1;   // (a library field the auxiliary stream may still be writing)
  {
    Scope s(c, "fieldstats");
    with_stats_view(ref != nullptr, weight != nullptr, [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)((size_t)c->nelemd * nf)), dim3(VIEW_THREADS), 0, c->stream, a, (const double*)c->spheremp, c->st_part);
    });
    LAUNCH_CHECK();
  }
  if (us && order_out(c, us)) return 1;
  HIPCHK(hipMemcpyAsync(out, c->st_part, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- pressure, geopotential and omega / p of a resident host's columns (k_column_view: tse_view_kernels.h) --------------------------------
// The plans and the overlap rule are host code (tse_views.cpp: column_view_plan / column_view_overlap); here the checks that need the
// runtime -- an input may lie inside an allocation of the library as in tse_stats_view, `out` may not (host_array_checks) -- the stream
// order of tse_view_put and one launch on the compute stream (launch_column_view: the kernel's instantiations are tse_column.hip's).
static_assert(COL_PINT == TSE_COL_PINT && COL_PMID == TSE_COL_PMID && COL_PHI == TSE_COL_PHI && COL_OMEGA == TSE_COL_OMEGA, "the ops of the header");
int tse_column_view(tse_ctx* c, int op, double ptop, double rgas, const tse_view* dp, const tse_view* p, const tse_view* a, const tse_view* b, const tse_view* out,
                    void* stream) {
  const char* who = "tse_column_view";
  if (!c) return fail("%s: null context", who);
  ViewPlan pl[5];
  { std::string err; if (column_view_plan(c->nelemd, op, dp, p, a, b, out, pl, &err)) return fail("%s", err.c_str()); }
  if (!std::isfinite(ptop) || ptop < 0.0) return fail("%s: ptop = %g (the pressure at the model top: finite and not negative)", who, ptop);
  if (!std::isfinite(rgas)) return fail("%s: rgas = %g is not finite", who, rgas);
  const tse_view* v[5] = {dp, p, a, b, out};
  bool in_library = false;
  const char* const role[4] = {"tse_column_view (dp)", "tse_column_view (p)", "tse_column_view (a)", "tse_column_view (b)"};   // the name a runtime refusal carries
  if (input_view_checks(c, 4, role, pl, v, stream, nullptr, &in_library)) return 1;
  if (host_array_checks(c, {{who, "out", &pl[4], out}}, stream)) return 1;
  { std::string err; if (column_view_overlap(v, pl, &err)) return fail("%s", err.c_str()); }
  ColumnViewArgs ka;
  input_view_args(ka, 4, pl, v);
  ka.out = dss_view_args(1, pl[4].ext[2], out);
  ka.ptop = ptop; ka.rgas = rgas;
  hipStream_t us = (hipStream_t)stream;
  if (order_in(c, us)) return 1;
  if (in_library && join_inputs(c)) return 1;   // (a library field the auxiliary stream may still be writing)
  {
    Scope s(c, "fieldcol");
    launch_column_view(c->stream, c->nelemd, op, p != nullptr, pl[4].path, view_wide(pl[4].path, out), ka, (double*)out->ptr);   // (tse_column.hip)
    LAUNCH_CHECK();
  }
  return order_out(c, us);
}
