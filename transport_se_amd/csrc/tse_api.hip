// tse_api.hip -- host side of libtransport_se_hip.so: the C ABI declared in include/transport_se_hip.h.
//
// Owns all device memory for the run (as cuda_mod owns qdp_d etc., reference cuda_mod.F90:74-106), converts the
// reference's edge descriptors (putmapP/getmapP/reverse + Send/RecvCycle slots) into on-device gather tables once
// at init, and sequences the kernels of tse_kernels.h on two HIP streams: the compute stream and -- when the rank has
// neighbour ranks -- a communication stream that carries pack -> RCCL send/recv -> unpack of the rank-boundary columns
// while the compute stream works on the interior elements (the reference's own accelerator seam orders its work the
// same way: cuda_mod.F90:358-401,961-1005; the exchange it replaces is bndry_mod.F90:74-124).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "tse_ctx.h"
#include "tse_launch.h"
#include "tse_tables.h"
#include "tse_views.h"

using namespace tse;

// Experiment and fault-injection switches (TSE_AB_*: A/B variants; TSE_TEST_*: failures on request for the tests) exist only in a build
// with -DTSE_AB_HOOKS
// (libtransport_se_hip_hooks.so: tools/ab_build.sh, _lib.build_hooks()); the product library does not read them at all.
#ifdef TSE_AB_HOOKS
static const char* hook_env(const char* name) { return getenv(name); }
#else
static const char* hook_env(const char*) { return nullptr; }
#endif

// the message of tse_last_error: written by tse::fail alone (tse_ctx.h), whichever unit the refusing entry is defined in
static thread_local char g_err[512] = "";
namespace tse {
int fail(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return 1;
}
int set_last_error(const char* msg) { return fail("%s", msg); }   // (tse_views.cpp: tse_view_plan)
}  // namespace tse

const char* tse_last_error(void) { return g_err; }
int tse_nlev(void) { return NLEV; }

// the element bounds of Qdp(tl)/dp now sit in qmin2/qmax2 (tl = 0: nothing cached); any halo of older bounds is stale.  Every entry that
// changes Qdp or ps_v passes here, so the Q / lnps of tse_state_q go stale here too.
void tse::set_bounds_cache(tse_ctx* c, int tl) { c->mm_valid = c->lim ? tl : 0; c->mm_halo = 0; c->qmix_valid = false; }

// The route switches of a call.  Read from the environment by every call that asks, never kept in the context: tests flip them between
// calls on a live context.
struct Route {
  // the whole-step call assembles the DSS on read.  false: one DSS pass per stage, as the per-stage API always does -- TSE_DSS_ON_READ=0,
  // or a scratch plane of plane_limit bytes or more (plane_over): gather offsets are 32-bit bytes within a plane, and
  // TSE_TEST_PLANE_LIMIT lowers the 4 GiB limit so that tests reach the fallback
  bool dss_on_read, plane_over;
  size_t plane_limit;
  int remap_nt;        // TSE_REMAP_NT: tracers per thread in the remap's lockstep column loop
  int remap_generic;   // TSE_REMAP_GENERIC=1: the remap always takes the generic loop (tests)
  // the remap that closes a cycle of tse_prim_run_subcycle assembles the last step's final DSS + time average on read; false
  // (TSE_REMAP_FUSED=0, no DSS on read, or TSE_REMAP_NT != 1): that step runs its own final DSS pass and the remap works in place
  bool remap_fused;
};
static Route route(const tse_ctx* c) {
  auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
  auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  Route r;
  r.plane_limit = hook_env("TSE_TEST_PLANE_LIMIT") ? (size_t)strtoull(hook_env("TSE_TEST_PLANE_LIMIT"), nullptr, 10) : ((size_t)1 << 32);
  r.plane_over = on("TSE_DSS_ON_READ") && c->tps * 8 >= r.plane_limit;
  r.dss_on_read = on("TSE_DSS_ON_READ") && !r.plane_over;
  r.remap_nt = num("TSE_REMAP_NT", 1);
  r.remap_generic = num("TSE_REMAP_GENERIC", 0);
  r.remap_fused = on("TSE_REMAP_FUSED") && r.dss_on_read && r.remap_nt == 1;
  return r;
}

static void resolve_timers(tse_ctx* c) {
  if (c->pending.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  if (c->comm_pending && c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);   // (a prefetched bounds exchange may be in flight)
  c->comm_pending = false;
  for (auto& p : c->pending) take_pending(c, p);
  c->pending.clear();
}

// streaming pass over n double2: in -> out (in null: write only; out null: read only); every block works through contiguous 16 KB pieces
__global__ __launch_bounds__(256) void k_probe_copy(size_t n, const double2* __restrict__ in, double2* __restrict__ out) {
  const size_t per = 1024;
  for (size_t p = blockIdx.x; p * per < n; p += gridDim.x)
#pragma unroll
    for (int u = 0; u < 4; u++) { const size_t i = p * per + u * 256 + threadIdx.x; if (i < n) { double2 v = in ? in[i] : make_double2(1., 2.); if (out) out[i] = v; else if (v.x == 1.2345e300) ((double2*)in)[i] = v; } }
}

// Where the five tracer-sized fields live.  The 288 GB are not one uniform memory: streaming WRITES into separately allocated 28 GB
// chunks run at 5.5 to 6.9 TB/s depending on the chunk (reads: 6.35 everywhere; tools/region_probe.hip); the rate is a property of the
// allocation (of how its physical memory happens to be put together: the same virtual range freed and allocated again behind a small
// pad writes at another rate; in short bursts all chunks are alike), it is fixed for the life of the allocation -- and the kernels
// follow it:
//  * with a 5.5 TB/s chunk as T (written by stages 1 and 3a) a tracer step takes 2-3 ms longer than with any faster one (k_lap1 14.8
//    instead of 13.4-13.7 ms, k_advance<0,0> 12.6 instead of 12.0; a probe timed all 60-120 assignments of three out of five or six
//    chunks with the real kernels);
//  * k_dss_patch, which writes Qdp(np1), takes 16.3-17.1 ms into a chunk that streams at 5.9 TB/s or more and 18.5-19.3 ms into one
//    at 5.5-5.7; with both time levels in one allocation it alternated between the two step by step, the first allocation of a
//    process being a slow one nearly always.
// This was the unexplained "run-to-run modes" of rounds 1 and 2.  So tse_init places the five fields by trial: it allocates field-sized
// chunks (up to 8 held at a time, memory allowing) and times a streaming write into each (3 x 5 ms); as long as fewer than three of the
// held chunks reach TSE_PLACEMENT_GOOD (6000 GB/s) it frees the slowest, allocates a 256 MB pad and tries again -- at most
// TSE_PLACEMENT tries in all (default 20; 0 = off).  The five fastest become T, Qdp(1), Qdp(2), B, C in that order (the first three are
// the roles that matter), the rest and the pads are freed before anything else is allocated.  Pure placement: no bit of any result moves.
// (profiles/r03_ab_placement.txt)
static int place_fields(tse_ctx* c, size_t scr_n, size_t trc) {
  c->place_n = 0;
  const int budget = std::min(32, getenv("TSE_PLACEMENT") ? atoi(getenv("TSE_PLACEMENT")) : 20);   // (place_bw / tse_placement report 32 tries)
  const double good = getenv("TSE_PLACEMENT_GOOD") ? atof(getenv("TSE_PLACEMENT_GOOD")) : 6000.0;
  const size_t chunk = std::max(scr_n, trc);
  double** role[5] = {&c->T, &c->qlev[0], &c->qlev[1], &c->B, &c->C};
  if (budget <= 5 || chunk * 8 < ((size_t)1 << 30)) {   // small fields live in the caches: nothing to choose
    if (dalloc(&c->qlev[0], trc) || dalloc(&c->qlev[1], trc) || dalloc(&c->T, scr_n) || dalloc(&c->B, scr_n) || dalloc(&c->C, scr_n)) return 1;
    return 0;
  }
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
  struct Held { double gbs; double* p; int tryno; };
  std::vector<Held> held;
  std::vector<void*> pads;
  const size_t reserve = (size_t)24 << 30;   // what the rest of tse_init allocates (level fields, bounds, halo) and a margin
  auto ngood = [&]() { int n = 0; for (const Held& h : held) n += h.gbs >= good; return n; };
  int rc = 0;
  while (c->place_n < budget) {
    if (held.size() >= 5 && ngood() >= 3) break;
    size_t fr = 0, tot = 0;
    const bool room = held.size() < 5 || (held.size() < 8 && hipMemGetInfo(&fr, &tot) == hipSuccess && fr >= chunk * 8 + reserve);
    if (!room) {   // give the slowest one back and shift what the next allocation gets
      size_t w = 0;
      for (size_t i = 1; i < held.size(); i++) if (held[i].gbs < held[w].gbs) w = i;
      (void)hipFree(held[w].p); held.erase(held.begin() + w);
      void* pad = nullptr;
      if (hipMalloc(&pad, (size_t)256 << 20) == hipSuccess) pads.push_back(pad); else (void)hipGetLastError();
    }
    double* p = nullptr;
    if (hipMalloc((void**)&p, chunk * 8) != hipSuccess) { (void)hipGetLastError(); if (held.size() < 5) rc = 1; break; }
    hipLaunchKernelGGL(k_probe_copy, dim3(2048), dim3(256), 0, c->stream, chunk / 2, (const double2*)nullptr, (double2*)p);
    (void)hipEventRecord(a, c->stream);
    for (int r = 0; r < 2; r++) hipLaunchKernelGGL(k_probe_copy, dim3(2048), dim3(256), 0, c->stream, chunk / 2, (const double2*)nullptr, (double2*)p);
    float ms = 0;
    if (hipEventRecord(b, c->stream) != hipSuccess || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipFree(p); rc = 1; break; }
    const double gbs = (double)chunk * 8 / (ms / 2) / 1e6;
    if (c->place_n < 32) c->place_bw[c->place_n] = gbs;
    held.push_back({gbs, p, c->place_n++});
  }
  if (held.size() < 5) rc = 1;
  std::stable_sort(held.begin(), held.end(), [](const Held& x, const Held& y) { return x.gbs > y.gbs; });
  for (size_t i = 0; i < held.size(); i++) {
    if (!rc && i < 5) { *role[i] = held[i].p; c->place_sel[i] = held[i].tryno; }
    else (void)hipFree(held[i].p);
  }
  for (void* p : pads) (void)hipFree(p);
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  if (rc) {
    // the trial ran out of memory or of luck part-way (a chunk given back and its replacement refused: fragmentation, another
    // process on the device): everything it held is free again -- take the fields as they come, as with TSE_PLACEMENT=0
    c->place_n = 0;
    for (double** r : role) *r = nullptr;
    if (dalloc(&c->qlev[0], trc) || dalloc(&c->qlev[1], trc) || dalloc(&c->T, scr_n) || dalloc(&c->B, scr_n) || dalloc(&c->C, scr_n)) return 1;
    return 0;
  }
  return 0;
}

static int init_impl(tse_ctx* c, const tse_init_args* a) {
  if (a->device >= 0) HIPCHK(hipSetDevice(a->device));
  HIPCHK(hipGetDevice(&c->device));
  c->nelemd = a->nelemd; c->qsize = a->qsize; c->nu_q = a->nu_q; c->ps0 = a->ps0; c->rsplit = a->rsplit;
  c->exchange = a->exchange; c->exchange_user = a->exchange_user;
  c->remap_alg2 = a->vert_remap_q_alg == 2;
  c->lim = a->limiter_option == 8 || a->limiter_option == 9;
  c->limiter_option = a->limiter_option;
  memcpy(c->D.d, a->Dvv, sizeof c->D.d);
  { std::vector<double> dv(a->Dvv, a->Dvv + 16); if (upload(&c->dvv_d, dv)) return 1; }
  HIPCHK(hipStreamCreate(&c->stream));   // blocking w.r.t. the legacy default stream: see the note above split_stage
  HIPCHK(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_inputs, hipEventDisableTiming));
  const int n = a->nelemd;
  std::vector<double> h;
  gather_strided(h, a->Dinv, a->Dinv_stride, n, 64);
  // Dinv(a,b,i,j) in Fortran memory = [p][b][a] -> keep as is: [e][p][4] = {D11, D21, D12, D22}
  if (upload(&c->Dinv, h)) return 1;
  gather_strided(h, a->metdet, a->metdet_stride, n, 16);       if (upload(&c->metdet, h)) return 1;
  gather_strided(h, a->rmetdet, a->rmetdet_stride, n, 16);     if (upload(&c->rmetdet, h)) return 1;
  gather_strided(h, a->spheremp, a->spheremp_stride, n, 16);   if (upload(&c->spheremp, h)) return 1;
  gather_strided(h, a->rspheremp, a->rspheremp_stride, n, 16); if (upload(&c->rspheremp, h)) return 1;
  {
    std::vector<double> v(a->hyai, a->hyai + NLEVP); if (upload(&c->hyai, v)) return 1;
    std::vector<double> w(a->hybi, a->hybi + NLEVP); if (upload(&c->hybi, w)) return 1;
    std::vector<double> d0(NLEV);  // dp0(k), prim_advection_mod.F90:818-819
    for (int k = 0; k < NLEV; k++) d0[k] = (a->hyai[k + 1] - a->hyai[k]) * a->ps0 + (a->hybi[k + 1] - a->hybi[k]) * a->ps0;
    if (upload(&c->dp0, d0)) return 1;
  }

  // ---- edge descriptors -> the tables of the kernels (tse_tables.cpp) ------------------------------
  {
    // TSE_BOUNDARY_STRIPS=1: rank-boundary elements in patches of their own (tse_tables.cpp: Tiling::bands; off by default)
    const bool strips = getenv("TSE_BOUNDARY_STRIPS") && atoi(getenv("TSE_BOUNDARY_STRIPS")) != 0;
    HostTables t;
    std::string err;
    if (build_tables(*a, strips, &t, &err)) return fail("%s", err.c_str());
    c->ncol_send = t.ncol_send; c->ncol_recv = t.ncol_recv; c->nmm_send = t.nmm_send; c->nmm_recv = t.nmm_recv;
    c->send_peer = t.send_peer; c->recv_peer = t.recv_peer; c->send_len = t.send_len; c->recv_len = t.recv_len;
    c->mm_send_len = t.mm_send_len; c->mm_recv_len = t.mm_recv_len;
    c->n_bnd = t.n_bnd; c->n_int = t.n_int; c->nslots = t.nslots; c->cse = t.cse;
    PatchSet& P = c->pset;
    P.npatch = t.npatch; P.np_bnd = t.np_bnd; P.np_int = t.np_int;
    if (upload(&c->dss_tab, t.dss_tab) || upload(&c->nbr, t.nbr) || upload(&c->send_src, t.send_src) || upload(&c->mm_send_src, t.mm_send_src) ||
        upload(&c->order, t.order) || upload(&c->ord_bnd, t.ord_bnd) || upload(&c->ord_int, t.ord_int) ||
        upload(&P.pslots, t.pslots) || upload(&P.pring, t.pring) || upload(&P.plds, t.plds) || upload(&P.pering, t.pering) || upload(&P.pnb, t.pnb) ||
        upload(&P.plist_bnd, t.plist_bnd) || upload(&P.plist_int, t.plist_int) ||
        upload(&c->slot_of, t.slot_of) || upload(&c->send_src_s, t.send_src_s) || upload(&c->pperm, t.pperm) || upload(&c->pexp, t.pexp) ||
        upload(&c->etab, t.etab) || upload(&c->rl_all, t.rl_all) || upload(&c->rl_bnd, t.rl_bnd) || upload(&c->rl_int, t.rl_int)) return 1;
  }

  // ---- state -------------------------------------------------------------------------------------
  const size_t lev = c->lev(), trc = c->trc();
  // scratch fields T, B: one plane per tracer = NCHUNK chunks of (element slots + one all-zero slot, the target of empty DSS
  // contributions, + the received halo columns, which DSS-on-read reads from there); see tse_kernels.h
  c->tps = ((size_t)NCHUNK * c->cse * CL + 15) / 16 * 16;
  if (c->tps < (size_t)n * 16 * NLEV) return fail("tse_init: scratch plane smaller than a tracer plane");
  const size_t scr_n = (size_t)(c->qsize + 1) * c->tps;   // qsize tracer planes + the plane of the stage's extra DSS variable
  if (place_fields(c, scr_n, trc)) return fail("tse_init: out of device memory (%zu B per tracer field, 5 fields)", trc * 8);
  HIPCHK(hipMemset(c->T, 0, scr_n * 8)); HIPCHK(hipMemset(c->B, 0, scr_n * 8)); HIPCHK(hipMemset(c->C, 0, scr_n * 8));
  if (dalloc(&c->vn0, 2 * lev) || dalloc(&c->dp, lev) || dalloc(&c->divdp, lev) || dalloc(&c->divdp_proj, lev) ||
      dalloc(&c->eta, (size_t)n * NLEVP * 16) || dalloc(&c->omega_p, lev) || dalloc(&c->dp3d, lev) || dalloc(&c->ps_v, (size_t)n * 16) ||
      dalloc(&c->lvl_tmp, lev) || dalloc(&c->sink, (size_t)NLEV * 16 + 2 * (size_t)c->mm_m()) || dalloc(&c->eta2, (size_t)n * NLEVP * 16)) return 1;
  // (behind the local elements: room for the received bounds of the compact exchange, see k_unpack_minmax)
  const size_t mm = (size_t)(n + c->nmm_recv) * c->mm_m();
  if (dalloc(&c->qmin, mm) || dalloc(&c->qmax, mm) || dalloc(&c->qmin2, mm) || dalloc(&c->qmax2, mm) || dalloc(&c->bad, 1)) return 1;
  HIPCHK(hipMemset(c->qlev[0], 0, trc * 8)); HIPCHK(hipMemset(c->qlev[1], 0, trc * 8));
  HIPCHK(hipMemset(c->vn0, 0, 2 * lev * 8)); HIPCHK(hipMemset(c->dp, 0, lev * 8)); HIPCHK(hipMemset(c->divdp, 0, lev * 8));
  HIPCHK(hipMemset(c->divdp_proj, 0, lev * 8)); HIPCHK(hipMemset(c->eta, 0, (size_t)n * NLEVP * 16 * 8));
  HIPCHK(hipMemset(c->omega_p, 0, lev * 8)); HIPCHK(hipMemset(c->dp3d, 0, lev * 8)); HIPCHK(hipMemset(c->ps_v, 0, (size_t)n * 16 * 8));
  HIPCHK(hipMemset(c->qmin, 0, mm * 8)); HIPCHK(hipMemset(c->qmax, 0, mm * 8));
  HIPCHK(hipMemset(c->qmin2, 0, mm * 8)); HIPCHK(hipMemset(c->qmax2, 0, mm * 8));   // (the pad tracers of the layout are exchanged and reduced like the others)
  HIPCHK(hipMemset(c->bad, 0, sizeof(int)));
  HIPCHK(hipHostMalloc((void**)&c->bad_host, 2 * sizeof(int), hipHostMallocDefault));
  c->bad_host[0] = c->bad_host[1] = 0;
  for (hipEvent_t& e : c->bad_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // Halo buffers.  The reference sizes one aliased buffer for 3*qsize*nlev layers (prim_advection_mod.F90:488); here the
  // tracer DSS (qsize*nlev + nlev layers per column) and the element-constant min/max exchange (2*qsize*nlev per
  // (element, direction) pair) have their own buffers, so that the two exchanges of stage 3 can be in flight together.
  c->nlyr_halo = c->qsize * NLEV + NLEV;
  if (c->halo()) {
    const size_t m2 = (size_t)2 * c->mm_m();
    if (dalloc(&c->sendbuf, (size_t)std::max(1, c->ncol_send) * c->nlyr_halo) || dalloc(&c->recvbuf, (size_t)std::max(1, c->ncol_recv) * c->nlyr_halo) ||
        dalloc(&c->sendbuf_mm, (size_t)std::max(1, c->nmm_send) * m2) || dalloc(&c->recvbuf_mm, (size_t)std::max(1, c->nmm_recv) * m2)) return 1;
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi = numerically lowest = greatest priority
    HIPCHK(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, hi));
    if (!(hook_env("TSE_AB_SPLIT_STREAMS") && !atoi(hook_env("TSE_AB_SPLIT_STREAMS"))))   // A/B: 0 = both launches on the compute stream
      HIPCHK(hipStreamCreateWithPriority(&c->int_stream, hipStreamNonBlocking, lo));
    c->sync_events.assign(16, nullptr);
    for (hipEvent_t& e : c->sync_events) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_mm, hipEventDisableTiming));
  }
  if (with_every_remap([](auto kern, int) -> int {
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(RemapLds)));
        return 0;
      })) return 1;
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

int tse_init(tse_ctx** out, const tse_init_args* a) {
  if (!out || !a) return fail("tse_init: null argument");
  *out = nullptr;
  if (a->limiter_option != 8 && a->limiter_option != 9 && a->limiter_option != 0)
    return fail("tse_init: limiter_option=%d (supported: limiter_option=8, the optimization-based limiter, 9, the clip-and-sum limiter, and 0, no limiter)",
                a->limiter_option);
  if (a->nelemd <= 0 || a->qsize <= 0) return fail("tse_init: nelemd=%d qsize=%d", a->nelemd, a->qsize);
  if (a->vert_remap_q_alg < 0 || a->vert_remap_q_alg > 2)
    return fail("tse_init: vert_remap_q_alg=%d (0|1: mirrored ghost cells, 2: piecewise-constant boundary cells; control_mod.F90:61-66)", a->vert_remap_q_alg);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("tse_init: no HIP device (this library has no CPU fallback)");
#ifdef TSE_AB_HOOKS
  { static bool said = false; if (!said) { fprintf(stderr, "transport_se_hip: this is the TSE_AB_HOOKS build (A/B switches and fault injection enabled) -- not the product library\n"); said = true; } }
#endif
  tse_ctx* c = new tse_ctx();
  if (init_impl(c, a)) {   // release whatever was allocated before the failure (the message in g_err survives)
    tse_finalize(c);
    return 1;
  }
  *out = c;
  return 0;
}

// every device allocation the context owns (each one a hipMalloc of its own): what tse_finalize frees, and what a view of tse_remap_view
// may not touch
std::vector<void*> tse::device_allocations(const tse_ctx* c) {
  const PatchSet& P = c->pset;
  void* ptrs[] = {c->dcmip_tab, c->dvv_d, c->Dinv, c->metdet, c->rmetdet, c->spheremp, c->rspheremp, c->hyai, c->hybi, c->dp0, c->dss_tab, c->send_src,
                  c->nbr, c->mm_send_src, c->qlev[0], c->qlev[1], c->vn0, c->dp, c->divdp, c->divdp_proj, c->eta, c->omega_p, c->dp3d, c->ps_v,
                  c->lvl_tmp, c->eta2, c->sink, c->order, c->qmin, c->qmax, c->qmin2, c->qmax2, c->qmix, c->lnps, c->norm_owner, c->norm_colw, c->norm_dh, c->qref, c->bad, c->lat, c->lon, c->zm, c->zi, c->pint, c->dph,
                  c->sendbuf, c->recvbuf, c->sendbuf_mm, c->recvbuf_mm, c->ord_bnd, c->ord_int, c->slot_of, c->send_src_s, c->pperm, c->pexp, c->etab, c->rl_all, c->rl_bnd, c->rl_int,
                  c->T, c->B, c->C, P.pslots, P.plist_bnd, P.plist_int, P.pering, P.pring, P.plds, P.pnb, c->rv_status, c->rv_detail, c->rv_acc, c->dv_stage, c->dv_send, c->dv_recv, c->hv_stage, c->vec_tab, c->st_part};
  std::vector<void*> out;
  for (void* p : ptrs) if (p) out.push_back(p);
  return out;
}

void tse_finalize(tse_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
  if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
  if (c->pin_hi) (void)hipHostUnregister((void*)c->pin_lo);
  if (c->bad_host) (void)hipHostFree(c->bad_host);
  for (hipEvent_t e : c->bad_ev) if (e) (void)hipEventDestroy(e);
  for (int i = 0; i < 2; i++) { if (c->stage[i]) (void)hipHostFree(c->stage[i]); if (c->stage_ev[i]) (void)hipEventDestroy(c->stage_ev[i]); }
  for (void* p : device_allocations(c)) (void)hipFree(p);
  resolve_timers(c);
  for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->sync_events) if (e) (void)hipEventDestroy(e);
  if (c->ev_mm) (void)hipEventDestroy(c->ev_mm);
  for (hipEvent_t e : c->view_ev) if (e) (void)hipEventDestroy(e);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  if (c->int_stream) { (void)hipStreamSynchronize(c->int_stream); (void)hipStreamDestroy(c->int_stream); }
  if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_inputs) (void)hipEventDestroy(c->ev_inputs);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int tse_synchronize(tse_ctx* c) {
  if (c->comm_stream) HIPCHK(hipStreamSynchronize(c->comm_stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int tse_halo_layout(tse_ctx* c, int* ns, int* nr) { if (ns) *ns = c->ncol_send; if (nr) *nr = c->ncol_recv; return 0; }
int tse_halo_minmax_layout(tse_ctx* c, int* send_len, int* recv_len) {
  for (size_t i = 0; i < c->mm_send_len.size(); i++) send_len[i] = c->mm_send_len[i];
  for (size_t i = 0; i < c->mm_recv_len.size(); i++) recv_len[i] = c->mm_recv_len[i];
  return 0;
}
int tse_boundary_layout(tse_ctx* c, int* nb, int* ni) { if (nb) *nb = c->n_bnd; if (ni) *ni = c->n_int; return 0; }
// field placement: chunks tried at init (0: no choice was made), their streaming-write GB/s in the order tried (the first 32), and
// which try became T, Qdp(1), Qdp(2), B, C
int tse_placement(tse_ctx* c, int* ntried, double* write_gbs /* [32] */, int* chosen /* [5] */) {
  if (ntried) *ntried = std::min(c->place_n, 32);
  if (write_gbs) for (int i = 0; i < 32; i++) write_gbs[i] = i < c->place_n ? c->place_bw[i] : 0.0;
  if (chosen) for (int r = 0; r < 5; r++) chosen[r] = c->place_sel[r];
  return 0;
}
// patches that touch another rank (launched first in every stage) and that do not
int tse_patch_layout(tse_ctx* c, int* np_boundary, int* np_interior) {
  if (np_boundary) *np_boundary = c->pset.np_bnd;
  if (np_interior) *np_interior = c->pset.np_int;
  return 0;
}
int tse_invalidate_cache(tse_ctx* c) { set_bounds_cache(c, 0); c->dcmip_static = false; return 0; }

// ---- RCCL communicator ----------------------------------------------------------------------------
static const char* rccl_path() {
  static char buf[512] = "";
  if (!buf[0]) {
    Dl_info info;
    if (dladdr((void*)&ncclGetVersion, &info) && info.dli_fname) strncpy(buf, info.dli_fname, sizeof buf - 1);
    else strcpy(buf, "?");
  }
  return buf;
}
int tse_comm_unique_id(void* id_out) {
  static_assert(sizeof(ncclUniqueId) == TSE_COMM_ID_BYTES, "ncclUniqueId size");
  if (!id_out) return fail("tse_comm_unique_id: null argument");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  memcpy(id_out, &id, sizeof id);
  return 0;
}
// Everything tse_comm_init can find wrong WITHOUT talking to the other ranks.  ncclCommInitRank is a blocking collective: a rank
// that returned early from tse_comm_init would leave its peers inside the bootstrap for ever, so a host first calls this on
// every rank, agrees on the outcome over its own control plane (MPI_Allreduce, a gloo all_gather), and enters tse_comm_init
// only if every rank is ready (driver.PrimRun, cuda_mod_hip.F90).
int tse_comm_precheck(tse_ctx* c, int rank, int nranks) {
  if (!c) return fail("tse_comm_precheck: null context");
  if (c->comm) return fail("tse_comm_precheck: communicator already initialised");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail("tse_comm_precheck: rank %d of %d", rank, nranks);
  for (int p : c->send_peer) if (p < 0 || p >= nranks) return fail("tse_comm_precheck: send peer %d (this is rank %d of %d)", p, rank, nranks);
  for (int p : c->recv_peer) if (p < 0 || p >= nranks) return fail("tse_comm_precheck: recv peer %d (this is rank %d of %d)", p, rank, nranks);
  if (hook_env("TSE_TEST_FAIL_PRECHECK_RANK") && atoi(hook_env("TSE_TEST_FAIL_PRECHECK_RANK")) == rank)   // tests: one rank alone is not ready
    return fail("tse_comm_precheck: rank %d fails on request (TSE_TEST_FAIL_PRECHECK_RANK)", rank);
  if (c->halo() && !c->comm_stream) return fail("tse_comm_precheck: no communication stream");
  HIPCHK(hipSetDevice(c->device));
  int rt = 0;
  NCCLCHK(ncclGetVersion(&rt));
  // The library was compiled against rccl.h NCCL_MAJOR.NCCL_MINOR.NCCL_PATCH; the process runs whichever librccl.so.1 was loaded
  // first (under Python: the copy bundled with torch, which ships no rccl.h to build against -- see _lib.py: one RCCL per process).
  // What is used of RCCL is eleven entry points (ncclGetVersion, ncclGetErrorString, ncclGetUniqueId, ncclCommInitRank,
  // ncclCommUserRank, ncclCommCount, ncclGroupStart/End, ncclSend, ncclRecv, ncclCommAbort/Destroy), ncclDouble and the 128-byte
  // ncclUniqueId: unchanged through all of 2.x, and every one of them is EXECUTED against the runtime of the process by the loopback
  // tests (tests/test_gpu_rccl_exchange.py: RCCL 2.26.6 from torch under headers of 2.27.7).  Policy:
  //   * another major, or a runtime older than point-to-point send/recv (2.7): refused;
  //   * a runtime OLDER than the headers (the Python case): accepted, and said once on stderr with both versions and the path --
  //     refusing it would silently turn every multi-GPU run under Python into a host-staged one; TSE_RCCL_STRICT=1 refuses it
  //     (a host that wants header == runtime, e.g. the Fortran seam linking /opt/rocm/lib/librccl.so, gets exactly that);
  //   * a runtime newer than the headers: accepted silently (RCCL keeps old entry points).
  if (rt / 10000 != NCCL_MAJOR || rt < 20700)
    return fail("tse_comm_precheck: RCCL runtime %d.%d.%d (%s) cannot serve a library built with the headers of %d.%d.%d", rt / 10000, rt / 100 % 100,
                rt % 100, rccl_path(), NCCL_MAJOR, NCCL_MINOR, NCCL_PATCH);
  if (rt < NCCL_VERSION_CODE) {
    const char* strict = getenv("TSE_RCCL_STRICT");
    if (strict && atoi(strict))
      return fail("tse_comm_precheck: RCCL runtime %d.%d.%d (%s) is older than the headers the library was built with (%d.%d.%d) and TSE_RCCL_STRICT is set",
                  rt / 10000, rt / 100 % 100, rt % 100, rccl_path(), NCCL_MAJOR, NCCL_MINOR, NCCL_PATCH);
    static bool said = false;
    if (!said && rank == 0) {
      fprintf(stderr, "transport_se_hip: note: RCCL runtime %d.%d.%d (%s) is older than the build headers %d.%d.%d; the entry points used are common to "
                      "both (TSE_RCCL_STRICT=1 refuses this)\n", rt / 10000, rt / 100 % 100, rt % 100, rccl_path(), NCCL_MAJOR, NCCL_MINOR, NCCL_PATCH);
      said = true;
    }
  }
  return 0;
}
int tse_comm_init(tse_ctx* c, const void* id_in, int rank, int nranks) {
  if (!c || !id_in) return fail("tse_comm_init: null argument");
  if (tse_comm_precheck(c, rank, nranks)) return 1;
  ncclUniqueId id;
  memcpy(&id, id_in, sizeof id);
  ncclComm_t cm = nullptr;
  NCCLCHK(ncclCommInitRank(&cm, nranks, id, rank));   // on failure the context keeps its callback route (c->comm stays null)
  c->comm = cm;
  return 0;
}
// which RCCL this process resolved: version code of the runtime (ncclGetVersion), of the headers the library was built with, and
// the path of the shared object that provides ncclGetVersion (dladdr)
int tse_comm_version(int* runtime, int* built, char* path, size_t path_len) {
  int rt = 0;
  NCCLCHK(ncclGetVersion(&rt));
  if (runtime) *runtime = rt;
  if (built) *built = NCCL_VERSION_CODE;
  if (path && path_len) { strncpy(path, rccl_path(), path_len - 1); path[path_len - 1] = 0; }
  return 0;
}
int tse_comm_abort(tse_ctx* c) {
  if (!c) return fail("tse_comm_abort: null context");
  if (c->comm) { (void)ncclCommAbort(c->comm); c->comm = nullptr; }
  return 0;
}
int tse_comm_info(tse_ctx* c, int* rank, int* nranks) {
  int r = 0, n = 1;
  if (c->comm) { NCCLCHK(ncclCommUserRank(c->comm, &r)); NCCLCHK(ncclCommCount(c->comm, &n)); }
  if (rank) *rank = r;
  if (nranks) *nranks = n;
  return 0;
}

// ---- host <-> device copies ---------------------------------------------------------------------
// The host keeps elem(:) as a strided array of structures.  A host that has declared that array with tse_host_register
// (page-locked once, for the life of the context) gets every field copy as ONE 2-D DMA straight between elem(:) and the dense
// device array (row = one element's field, pitch = sizeof(element_t)): no staging copy at all.  Any other host pointer --
// temporaries, numpy arrays -- goes through the library's own page-locked staging buffers, two of them, so that packing the
// next block of elements overlaps the DMA of the previous one.  (Page-locking memory the caller may free behind the
// library's back is not safe, so it is never done implicitly.)
int tse_host_register(tse_ctx* c, void* base, size_t bytes) {
  static const double limit_gb = getenv("TSE_PIN_LIMIT_GB") ? atof(getenv("TSE_PIN_LIMIT_GB")) : 64.0;
  if (!base || !bytes) return fail("tse_host_register: null range");
  if (c->pin_hi) return fail("tse_host_register: a host range is already registered");
  if ((double)bytes > limit_gb * 1073741824.0) return 0;   // staged copies (TSE_PIN_LIMIT_GB raises the limit)
  if (hipHostRegister(base, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return 0; }   // not fatal: staged copies
  c->pin_lo = (uintptr_t)base; c->pin_hi = c->pin_lo + bytes;
  return 0;
}
static const size_t STAGE_BYTES = (size_t)32 << 20;
// `cnt` doubles per element between host (element stride `stride` bytes) and a dense device array [nelemd][cnt_dev]; asynchronous
// on the compute stream for registered host memory, complete on return otherwise
int tse::copy_field(tse_ctx* c, double* dev, size_t cnt_dev, void* host, size_t stride, size_t cnt, bool to_device) {
  if (!host) return 0;
  const int n = c->nelemd;
  if (stride < cnt * 8 && n > 1) return fail("field copy: element stride %zu smaller than the field (%zu bytes)", stride, cnt * 8);
  const uintptr_t a = (uintptr_t)host, b = a + (size_t)(n - 1) * stride + cnt * 8;
  if (c->pin_hi && a >= c->pin_lo && b <= c->pin_hi) {
    const size_t pitch = n > 1 ? stride : cnt * 8;
    if (to_device) HIPCHK(hipMemcpy2DAsync(dev, cnt_dev * 8, host, pitch, cnt * 8, n, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpy2DAsync(host, pitch, dev, cnt_dev * 8, cnt * 8, n, hipMemcpyDeviceToHost, c->stream));
    return 0;
  }
  if (!c->stage[0]) {
    HIPCHK(hipHostMalloc((void**)&c->stage[0], STAGE_BYTES, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void**)&c->stage[1], STAGE_BYTES, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&c->stage_ev[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->stage_ev[1], hipEventDisableTiming));
  }
  const int per = (int)std::max<size_t>(1, STAGE_BYTES / (cnt * 8));   // elements per block
  if (to_device) {
    int bi = 0;
    for (int e0 = 0; e0 < n; e0 += per, bi ^= 1) {
      const int m = std::min(per, n - e0);
      HIPCHK(hipEventSynchronize(c->stage_ev[bi]));   // the DMA that last read this buffer
      for (int e = 0; e < m; e++) memcpy(c->stage[bi] + (size_t)e * cnt, (const char*)host + (size_t)(e0 + e) * stride, cnt * 8);
      HIPCHK(hipMemcpy2DAsync(dev + (size_t)e0 * cnt_dev, cnt_dev * 8, c->stage[bi], cnt * 8, cnt * 8, m, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipEventRecord(c->stage_ev[bi], c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    int bi = 0, pend_e0 = -1, pend_m = 0;
    auto drain = [&](int buf, int e0, int m) {
      (void)hipEventSynchronize(c->stage_ev[buf]);
      for (int e = 0; e < m; e++) memcpy((char*)host + (size_t)(e0 + e) * stride, c->stage[buf] + (size_t)e * cnt, cnt * 8);
    };
    for (int e0 = 0; e0 < n; e0 += per, bi ^= 1) {
      const int m = std::min(per, n - e0);
      HIPCHK(hipMemcpy2DAsync(c->stage[bi], cnt * 8, dev + (size_t)e0 * cnt_dev, cnt_dev * 8, cnt * 8, m, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipEventRecord(c->stage_ev[bi], c->stream));
      if (pend_e0 >= 0) drain(bi ^ 1, pend_e0, pend_m);   // unpack the previous block while this one travels
      pend_e0 = e0; pend_m = m;
    }
    if (pend_e0 >= 0) drain(bi ^ 1, pend_e0, pend_m);
  }
  return 0;
}
int tse_copy_qdp_h2d(tse_ctx* c, const double* q1, size_t stride, int qsize_d, int nt) {
  set_bounds_cache(c, 0);
  if (nt < 1 || nt > 2 || qsize_d < c->qsize) return fail("tse_copy_qdp_h2d: nt=%d qsize_d=%d", nt, qsize_d);
  const size_t per = (size_t)c->qsize * NLEV * 16;   // Qdp(np,np,nlev,qsize_d,2): time level nt starts qsize_d*nlev*16 doubles in
  if (copy_field(c, c->q(nt), per, (char*)q1 + (size_t)(nt - 1) * qsize_d * NLEV * 16 * 8, stride, per, true)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int tse_copy_qdp_d2h(tse_ctx* c, double* q1, size_t stride, int qsize_d, int nt) {
  if (nt < 1 || nt > 2 || qsize_d < c->qsize) return fail("tse_copy_qdp_d2h: nt=%d qsize_d=%d", nt, qsize_d);
  const size_t per = (size_t)c->qsize * NLEV * 16;
  if (copy_field(c, c->q(nt), per, (char*)q1 + (size_t)(nt - 1) * qsize_d * NLEV * 16 * 8, stride, per, false)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
// state%Q(np,np,nlev,qsize_d) of elem(:), tracers 1..qsize, and state%lnps(:,:,np1): the device fields tse_state_q formed
int tse_copy_q_d2h(tse_ctx* c, double* q1, size_t stride, int qsize_d) {
  if (qsize_d < c->qsize) return fail("tse_copy_q_d2h: qsize_d=%d < qsize=%d", qsize_d, c->qsize);
  if (!c->qmix_valid) return fail("tse_copy_q_d2h: Q is stale (the state changed since the last tse_state_q, or there was none)");
  const size_t per = (size_t)c->qsize * NLEV * 16;
  if (copy_field(c, c->qmix, per, q1, stride, per, false)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int tse_copy_lnps_d2h(tse_ctx* c, double* lnps1, size_t stride) {
  if (!c->qmix_valid) return fail("tse_copy_lnps_d2h: lnps is stale (the state changed since the last tse_state_q, or there was none)");
  if (copy_field(c, c->lnps, 16, lnps1, stride, 16, false)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
static int put_level(tse_ctx* c, double* dev, const double* host, size_t stride, size_t cnt_dev, size_t cnt_host) {
  return copy_field(c, dev, cnt_dev, (void*)host, stride, std::min(cnt_dev, cnt_host), true);
}
static int get_level(tse_ctx* c, const double* dev, double* host, size_t stride, size_t cnt_dev, size_t cnt_host) {
  return copy_field(c, (double*)dev, cnt_dev, host, stride, std::min(cnt_dev, cnt_host), false);
}
int tse_set_derived(tse_ctx* c, const double* vn0, size_t s0, const double* dp, size_t s1, const double* eta, size_t s2,
                    const double* omega_p, size_t s3) {
  // vn0(np,np,2,nlev) in Fortran memory is [k][c][p]: the device layout
  if (put_level(c, c->vn0, vn0, s0, 2 * NLEV * 16, 2 * NLEV * 16)) return 1;
  if (dp) set_bounds_cache(c, 0);   // bounds were formed with the previous dp
  if (dp || omega_p) c->dcmip_static = false;
  if (put_level(c, c->dp, dp, s1, NLEV * 16, NLEV * 16)) return 1;
  if (put_level(c, c->eta, eta, s2, NLEVP * 16, NLEVP * 16)) return 1;
  if (put_level(c, c->omega_p, omega_p, s3, NLEV * 16, NLEV * 16)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));   // the caller may reuse its arrays
  return 0;
}
int tse_set_divdp(tse_ctx* c, const double* divdp, size_t s0, const double* divdp_proj, size_t s1) {
  if (put_level(c, c->divdp, divdp, s0, NLEV * 16, NLEV * 16)) return 1;
  if (put_level(c, c->divdp_proj, divdp_proj, s1, NLEV * 16, NLEV * 16)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int tse_get_derived(tse_ctx* c, double* divdp_proj, size_t s1, double* eta, size_t s2, double* omega_p, size_t s3, double* divdp,
                    size_t s4, double* dp3d, size_t s5, double* ps_v, size_t s6) {
  if (get_level(c, c->divdp_proj, divdp_proj, s1, NLEV * 16, NLEV * 16)) return 1;
  if (get_level(c, c->eta, eta, s2, NLEVP * 16, NLEV * 16)) return 1;  // levels 1:nlev only are DSS'd (:835-837)
  if (get_level(c, c->omega_p, omega_p, s3, NLEV * 16, NLEV * 16)) return 1;
  if (get_level(c, c->divdp, divdp, s4, NLEV * 16, NLEV * 16)) return 1;
  if (get_level(c, c->dp3d, dp3d, s5, NLEV * 16, NLEV * 16)) return 1;
  if (get_level(c, c->ps_v, ps_v, s6, 16, 16)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int tse_get_qminmax(tse_ctx* c, double* qmin, double* qmax) {
  if (!c->lim) return fail("tse_get_qminmax: this context runs without a limiter (limiter_option=0) and keeps no tracer bounds");
  const size_t mm = (size_t)c->nelemd * c->mm_m();
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<double> h(mm);
  double* outs[2] = {qmin, qmax};
  const double* devs[2] = {c->qmin, c->qmax};
  for (int a = 0; a < 2; a++) {
    if (!outs[a]) continue;
    HIPCHK(hipMemcpy(h.data(), devs[a], mm * 8, hipMemcpyDeviceToHost));
    for (int e = 0; e < c->nelemd; e++)          // device layout [e][k / CL][q][k % CL] (tse_kernels.h: mm_idx) -> [e][q][k]
      for (int q = 0; q < c->qsize; q++)
        for (int k = 0; k < NLEV; k++)
          outs[a][((size_t)e * c->qsize + q) * NLEV + k] = h[(((size_t)e * NCHUNK + k / CL) * mm_qpad(c->qsize) + q) * CL + (k % CL)];
  }
  return 0;
}

// ---- the path -----------------------------------------------------------------------------------

int tse_compute_divdp(tse_ctx* c) {
  Scope s(c, "level");
  hipLaunchKernelGGL(k_divdp<>, dim3(flat_blocks(c->nelemd)), dim3(FLAT_THREADS), 0, c->stream, c->nelemd, c->D, c->geo(), c->vn0, c->divdp, c->divdp_proj);
  LAUNCH_CHECK();
  return 0;
}

// bndry_exchangeV on the packed rank-boundary columns, ordered on stream `st` (no-op on one rank).
// kind 0: sendbuf/recvbuf, one entry per edge-buffer column; kind 1: the compact min/max buffers.
// With a communicator: one grouped RCCL receive + send per neighbour slot enqueued on `st`, no host synchronisation
// (bndry_mod.F90:74-112 posts all sends and receives, then waits).  Otherwise the host's callback, after `st` has drained.
// sb / rb: other buffers of the same column layout instead of the context's (tse_dss_view brings its own: nlyr is not bounded by qsize).
int tse::halo_exchange(tse_ctx* c, int nlyr, int kind, hipStream_t st, double* sb, double* rb) {
  if (!c->halo()) return 0;
  CommScope s(c, kind ? "comm_exchange_mm" : "comm_exchange_q", st);
  if (!sb) sb = kind ? c->sendbuf_mm : c->sendbuf;
  if (!rb) rb = kind ? c->recvbuf_mm : c->recvbuf;
  if (c->comm) {
    const std::vector<int>& ls = kind ? c->mm_send_len : c->send_len;
    const std::vector<int>& lr = kind ? c->mm_recv_len : c->recv_len;
    NCCLCHK(ncclGroupStart());
    size_t off = 0;
    for (size_t i = 0; i < lr.size(); i++) {
      if (lr[i]) NCCLCHK(ncclRecv(rb + off * nlyr, (size_t)lr[i] * nlyr, ncclDouble, c->recv_peer[i], c->comm, st));
      off += lr[i];
    }
    off = 0;
    for (size_t i = 0; i < ls.size(); i++) {
      if (ls[i]) NCCLCHK(ncclSend(sb + off * nlyr, (size_t)ls[i] * nlyr, ncclDouble, c->send_peer[i], c->comm, st));
      off += ls[i];
    }
    NCCLCHK(ncclGroupEnd());
    return 0;
  }
  if (!c->exchange) return fail("halo exchange: this rank has neighbour ranks but neither tse_comm_init was called nor an exchange callback given");
  HIPCHK(hipStreamSynchronize(st));
  if (c->exchange(c->exchange_user, sb, rb, nlyr, kind)) return fail("exchange callback failed");
  return 0;
}

// ---- pack / unpack launches (on stream st) ----
// scratch field (T, B or C) -> sendbuf layers [0, nlyr) of nlyr_halo; nlyr = qsize*nlev (tracers) or qsize*nlev + nlev (tracers and
// the plane of the stage's extra variable behind them: the reference's edgeAdv_p1 message, prim_advection_mod.F90:497,911-919)
// 32-bit work-item indices in the pack / unpack kernels
int tse::halo_items(size_t tot, unsigned* blocks) {
  if (tot >= ((size_t)1 << 32)) return fail("halo pack: %zu work items", tot);
  *blocks = (unsigned)((tot + 255) / 256);
  return 0;
}
static int pack_tracers(tse_ctx* c, hipStream_t st, const double* scratch, int nlyr_halo, int nlyr = 0) {
  const int nq = nlyr ? nlyr : c->qsize * NLEV;
  if (!c->ncol_send) return 0;
  CommScope s(c, "comm_pack_q", st);
  unsigned nb;
  if (halo_items((size_t)c->ncol_send * (nq / CL), &nb)) return 1;
  hipLaunchKernelGGL(k_pack_scratch<>, dim3(nb), dim3(256), 0, st, c->ncol_send, nq / CL, c->send_src_s, scratch, c->sendbuf, nlyr_halo, c->scr());
  LAUNCH_CHECK();
  return 0;
}
// spheremp*var -> sendbuf layers [qsize*nlev, +nlev).  eta_dot_dpdn carries nlev+1 levels per element; levels 1:nlev are exchanged (:835-837)
static int pack_var(tse_ctx* c, hipStream_t st, const double* var, int var_levels) {
  const int nq = c->qsize * NLEV;
  if (!c->ncol_send || !var) return 0;
  CommScope s(c, "comm_pack_q", st);
  unsigned nb;
  if (halo_items((size_t)c->ncol_send * NLEV, &nb)) return 1;
  hipLaunchKernelGGL(k_pack<>, dim3(nb), dim3(256), 0, st, c->ncol_send, NLEV, c->send_src, var, c->spheremp, c->sendbuf, nq + NLEV, nq, var_levels);
  LAUNCH_CHECK();
  return 0;
}
// The view entries' pack (tse_views_api.hip: stage_exchange): the rank-boundary columns of a dense staged field [e][nl][16], unweighted,
// into `send` with nl layers per column; `blocks` is halo_items of ncol_send * nl.  Here because k_pack<> is this code object's kernel.
int tse::pack_staged(tse_ctx* c, hipStream_t st, const double* staged, int nl, unsigned blocks, double* send) {
  CommScope s(c, "comm_pack_q", st);
  hipLaunchKernelGGL(k_pack<>, dim3(blocks), dim3(256), 0, st, c->ncol_send, nl, c->send_src, staged, (const double*)nullptr, send, nl, 0, nl);
  LAUNCH_CHECK();
  return 0;
}
static int pack_minmax(tse_ctx* c, hipStream_t st, const double* qmin = nullptr, const double* qmax = nullptr) {
  const int m = c->mm_m();
  if (!c->nmm_send) return 0;
  CommScope s(c, "comm_pack_mm", st);
  unsigned nb;
  if (halo_items((size_t)c->nmm_send * (m / 2), &nb)) return 1;
  hipLaunchKernelGGL(k_pack_minmax<>, dim3(nb), dim3(256), 0, st, c->nmm_send, m, c->mm_send_src,
                     qmin ? qmin : (const double*)c->qmin, qmax ? qmax : (const double*)c->qmax, c->sendbuf_mm, 2 * m, 0);
  LAUNCH_CHECK();
  return 0;
}
// DSS on read: copy the received tracer halo behind the planes of the scratch field the next slab kernel gathers from
static int unpack_halo(tse_ctx* c, hipStream_t st, double* field, int nlyr_halo, int nlyr = 0) {
  if (!c->ncol_recv) return 0;
  CommScope s(c, "comm_unpack_q", st);
  const int nq = nlyr ? nlyr : c->qsize * NLEV;   // layers to copy: the tracer planes, or also the extra variable's plane
  unsigned nb;
  if (halo_items((size_t)c->ncol_recv * (nq / CL), &nb)) return 1;
  hipLaunchKernelGGL(k_unpack_halo<>, dim3(nb), dim3(256), 0, st, c->ncol_recv, nq / CL, c->recvbuf, nlyr_halo, field, c->scr(), c->halo0());
  LAUNCH_CHECK();
  return 0;
}

// received element bounds -> behind the local elements of qmin/qmax (read by the stage-3 kernel through its element ring)
static int unpack_minmax(tse_ctx* c, hipStream_t st) {
  const int m = c->mm_m();
  if (!c->nmm_recv) return 0;
  CommScope s(c, "comm_unpack_mm", st);
  unsigned nb;
  if (halo_items((size_t)c->nmm_recv * (m / 2), &nb)) return 1;
  hipLaunchKernelGGL(k_unpack_minmax<>, dim3(nb), dim3(256), 0, st, c->nmm_recv, m, (const double*)c->recvbuf_mm, c->qmin + (size_t)c->nelemd * m,
                     c->qmax + (size_t)c->nelemd * m);
  LAUNCH_CHECK();
  return 0;
}

// ---- the two exchanges, pack to unpack, on stream st ----
// a scratch field's rank-boundary columns: nlyr_halo layers per column in the buffers, of which nlyr are the field's (0: the tracer
// planes alone) and, where the stage's extra variable travels from its own array, the last NLEV are spheremp*var
static int exchange_halo(tse_ctx* c, hipStream_t st, double* field, int nlyr_halo, int nlyr = 0, const double* var = nullptr, int var_levels = 0) {
  return pack_tracers(c, st, field, nlyr_halo, nlyr) || pack_var(c, st, var, var_levels) || halo_exchange(c, nlyr_halo, 0, st) ||
         unpack_halo(c, st, field, nlyr_halo, nlyr);
}
// the element bounds into recvbuf_mm: qmin/qmax, or those in `from` (tse_ctx::emitted)
static int exchange_bounds(tse_ctx* c, hipStream_t st, tse_ctx::Bounds from = {nullptr, nullptr}) {
  return pack_minmax(c, st, from.mn, from.mx) || halo_exchange(c, 2 * c->mm_m(), 1, st);
}

// min/max over the <= 8 neighbours of qmin/qmax (double-buffered on the device); the halo part must have arrived
static int nbr_minmax_kernel(tse_ctx* c) {
  const int m = c->mm_m();
  {
    Scope s(c, "minmax");
    hipLaunchKernelGGL(k_nbr_minmax_patch<8>, dim3(nbr_patch_blocks(c->pset.npatch, c->qsize)), dim3(512), 0, c->stream, c->pset.npatch, c->qsize, c->nbr,
                       c->pset.pslots, c->slot_of, c->qmin, c->qmax, c->qmin2, c->qmax2, c->recvbuf_mm, 2 * m);
    LAUNCH_CHECK();
  }
  std::swap(c->qmin, c->qmin2); std::swap(c->qmax, c->qmax2);
  return 0;
}
// neighbor_minmax (viscosity_mod.F90:748-816), everything on the compute stream (per-stage API)
static int neighbor_minmax(tse_ctx* c) {
  {
    CommScope w(c, "comm_wait", c->stream);   // (on the compute stream: the whole exchange is exposed)
    if (exchange_bounds(c, c->stream)) return 1;
  }
  return nbr_minmax_kernel(c);
}
// the element bounds of Qdp(n0)/dp into qmin/qmax: those the previous step's last kernel (final DSS or remap) left in qmin2/qmax2
// (cached), else formed here
static int own_bounds(tse_ctx* c, const double* Qn0, bool cached) {
  if (cached) { std::swap(c->qmin, c->qmin2); std::swap(c->qmax, c->qmax2); return 0; }
  Scope s(c, "minmax");
  hipLaunchKernelGGL(k_qminmax<>, dim3(flat_blocks(c->nelemd)), dim3(FLAT_THREADS), 0, c->stream, c->nelemd, c->qsize, 0.0, Qn0, c->dp, c->divdp_proj,
                     c->qmin, c->qmax);
  LAUNCH_CHECK();
  return 0;
}

// DSS of the extra level variable of a stage (divdp_proj / eta_dot_dpdn / omega_p): rspheremp*DSS(spheremp*var), remote
// contributions from recvbuf layers [qsize*nlev, +nlev) (prim_advection_mod.F90:911-919,943-957)
static int dss_level_var(tse_ctx* c, double** varp, int var_levels) {
  if (!varp) return 0;
  const int nq = c->qsize * NLEV;
  Scope s(c, "level");
  // out of place into the field's twin buffer (the source must stay intact while neighbours read it), then swap the two
  double** twin = var_levels == NLEV ? &c->lvl_tmp : &c->eta2;
  hipLaunchKernelGGL(k_dss_lvl<>, dim3(8 * dss_blocks_per_xcd<LVL_UNITS>(c->nelemd)), dim3(DSS_FLAT_THREADS), 0, c->stream, c->nelemd, c->dss_tab,
                     c->rspheremp, c->spheremp, *varp, var_levels, *twin, var_levels, c->recvbuf, nq + NLEV, nq, c->order);
  LAUNCH_CHECK();
  std::swap(*varp, *twin);
  return 0;
}
// tracer DSS pass src (scratch layout, halo columns filled) -> dst (standard layout), optionally fused with qdp_time_avg and the
// next step's bounds; over all patches (npwork < 0) or over the patch list of a split launch
static int dss_tracer_launch(tse_ctx* c, const double* src, double* dst, const double* Qn0_avg, const int* plist, int npwork,
                             double* var_out = nullptr, int var_out_lev = 0) {
  if (!npwork) return 0;
  const GatherArgs ga = c->gargs(nullptr, c->nelemd, plist, npwork, nullptr, 0, var_out, var_out_lev);
  const dim3 grid(patch_blocks(npwork));
  if (Qn0_avg)
    hipLaunchKernelGGL(k_dss_patch<1>, grid, dim3(Patch::THREADS), 0, c->stream, c->qsize, src, dst, Qn0_avg, (const double*)c->dp, c->emitted().mn,
                       c->emitted().mx, ga);
  else
    hipLaunchKernelGGL(k_dss_patch<0>, grid, dim3(Patch::THREADS), 0, c->stream, c->qsize, src, dst, (const double*)nullptr, (const double*)nullptr,
                       (double*)nullptr, (double*)nullptr, ga);
  LAUNCH_CHECK();
  return 0;
}
static int dss_tracer_pass(tse_ctx* c, const double* src, double* dst, const double* Qn0_avg, double* var_out = nullptr, int var_out_lev = 0) {
  Scope s(c, "dss");
  return dss_tracer_launch(c, src, dst, Qn0_avg, nullptr, c->pset.npatch, var_out, var_out_lev);
}

// one launch of a stage's slab kernel on the compute stream (tse_launch.h): the context's share of the arguments, and what the stages
// and the launches of a split stage differ in
static StageArgs stage_args(const tse_ctx* c, dim3 grid, dim3 block, double dt, const double* Qn0, const double* lap, double* out, const GatherArgs& ga) {
  return StageArgs{c->stream, grid, block, c->nelemd, c->D, c->geo(), c->qsize, dt, c->nu_q, Qn0, lap, out, c->vn0, c->dp, c->divdp, c->divdp_proj,
                   c->qmin, c->qmax, c->dp0, ga, c->lim, c->limiter_option};
}

// One euler_step of the per-stage API (prim_advection_mod.F90:667-970): every stage ends with a tracer DSS pass, because
// Qdp(np1) must exist after each call; all work and the halo exchanges are ordered on the compute stream.
static int euler_step_impl(tse_ctx* c, int np1_qdp, int n0_qdp, double dt, int DSSopt, int rhs, bool fuse_avg, int avg_n0, bool fused_mm) {
  if (np1_qdp < 1 || np1_qdp > 2 || n0_qdp < 1 || n0_qdp > 2) return fail("euler_step: bad time levels %d %d", np1_qdp, n0_qdp);
  if (rhs < 0 || rhs > 2) return fail("euler_step: rhs_multiplier=%d", rhs);
  double* Qn0 = c->q(n0_qdp);
  double* Qnp1 = c->q(np1_qdp);
  double** var = DSSopt == 1 ? &c->eta : DSSopt == 2 ? &c->omega_p : DSSopt == 3 ? &c->divdp_proj : nullptr;
  const int var_levels = DSSopt == 1 ? NLEVP : NLEV;
  const int nq = c->qsize * NLEV;
  const dim3 grid(flat_blocks(c->nelemd)), blk(FLAT_THREADS);
  const GatherArgs plain = c->gargs(nullptr, c->nelemd, nullptr, 0);
  if (rhs == 0) {
    if (c->lim) {
      if (own_bounds(c, Qn0, fused_mm && c->mm_valid == n0_qdp)) return 1;
      set_bounds_cache(c, 0);
      if (neighbor_minmax(c)) return 1;
    }
    Scope s(c, "advance0");
    launch_advance<0, 0, false>(stage_args(c, grid, blk, dt, Qn0, nullptr, c->T, plain));
    LAUNCH_CHECK();
  } else if (rhs == 1) {
    Scope s(c, "advance1");
    launch_advance<1, 0, false>(stage_args(c, grid, blk, dt, Qn0, nullptr, c->T, plain));
    LAUNCH_CHECK();
  } else {
    c->t_zero_dirty = true;   // below, T receives rspheremp*DSS(lap) in the plain tracer layout
    {
      Scope s(c, "lap");
      launch_lap1<0>(stage_args(c, grid, blk, 2 * dt, Qn0, nullptr, c->B, plain));
      LAUNCH_CHECK();
    }
    // biharmonic_wk_scalar_minmax: DSS(lap1) (+ min/max exchange) -> T = rspheremp*DSS(lap1).  The reference's message is
    // (lap, Qmin, Qmax) = 3*qsize*nlev layers (viscosity_mod.F90:389-391); here the Laplacian and the bounds travel separately.
    {
      CommScope w(c, "comm_wait", c->stream);
      if (exchange_halo(c, c->stream, c->B, nq)) return 1;
    }
    if (dss_tracer_pass(c, c->B, c->T, nullptr)) return 1;
    if (c->lim && neighbor_minmax(c)) return 1;
    Scope s(c, "advance2");
    launch_advance<2, 0, false>(stage_args(c, grid, blk, dt, Qn0, c->T, c->B, plain));
    LAUNCH_CHECK();
  }
  double* pre = rhs == 2 ? c->B : c->T;
  const double* avg = fuse_avg ? c->q(avg_n0) : nullptr;
  // edgeVpack(Qdp) + edgeVpack(spheremp*DSSvar) -> bndry_exchangeV -> edgeVunpack + rspheremp  (:911-960)
  {
    CommScope w(c, "comm_wait", c->stream);
    if (exchange_halo(c, c->stream, pre, nq + NLEV, 0, var ? *var : nullptr, var_levels)) return 1;
  }
  if (dss_tracer_pass(c, pre, Qnp1, avg)) return 1;
  return dss_level_var(c, var, var_levels);
}

int tse_euler_step(tse_ctx* c, int np1_qdp, int n0_qdp, double dt, int DSSopt, int rhs_multiplier) {
  set_bounds_cache(c, 0);
  return euler_step_impl(c, np1_qdp, n0_qdp, dt, DSSopt, rhs_multiplier, false, 0, false);
}

int tse_qdp_time_avg(tse_ctx* c, int rkstage, int n0_qdp, int np1_qdp) {
  set_bounds_cache(c, 0);
  Scope s(c, "avg");
  size_t n = c->trc();
  hipLaunchKernelGGL(k_time_avg<>, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, c->stream, n, rkstage,
                     c->q(n0_qdp), c->q(np1_qdp));
  LAUNCH_CHECK();
  return 0;
}

// ---- whole-step path: DSS on read + boundary-first overlap ------------------------------------------
// Stages 1 and 2 leave their pre-DSS scratch (T, then B) un-DSS'd and the next stage's slab kernel assembles
// rspheremp*DSS(.) while reading it; the stage-3 Laplacian is handed over the same way.
//
// On several ranks every slab kernel is launched twice: over the elements that touch another rank (`ord_bnd`), then over
// the rest (`ord_int`).  Between the two launches the communication stream is handed the pack -> exchange -> unpack of
// the stage, so the halo travels over xGMI while the interior elements are computed; the compute stream waits for it
// only before the next stage's first launch.  With an RCCL communicator nothing blocks the host.  With the callback
// form of the seam the host has to drain the packs and run the callback; that is done after the interior launch has
// been queued.  Whether the exchange then overlaps the interior launch depends on the callback: one that moves the slots on
// streams of its own (or over MPI from host memory) does; the Python callbacks of driver.HaloExchange copy on the legacy
// default stream, which waits for this (blocking) compute stream -- their exchange runs behind the interior launch.  (The
// compute stream stays a blocking stream on purpose: the synchronous hipMemcpy / hipMemset calls of the set-up and of the
// operator-level entry points are ordered against it by the default-stream rule.)
static hipEvent_t next_sync_event(tse_ctx* c) {
  hipEvent_t e = c->sync_events[c->sync_next];
  c->sync_next = (c->sync_next + 1) % c->sync_events.size();
  return e;
}

// the part of the local mesh one launch covers: everything (single rank), the elements / patches that touch another rank, the rest
struct Work { const int* order; int nwork; const int* plist; int npwork; };
static Work work_of(const tse_ctx* c, int part) {
  const PatchSet& P = c->pset;
  if (part == 0) return Work{nullptr, c->nelemd, nullptr, P.npatch};
  if (part == 1) return Work{c->ord_bnd, c->n_bnd, P.plist_bnd, P.np_bnd};
  return Work{c->ord_int, c->n_int, P.plist_int, P.np_int};
}

// done_out == nullptr: the compute stream waits for the communication work before it goes on; otherwise the event that marks
// its completion is handed back and whoever consumes the halo waits for it (the prefetched bounds exchange)
template <class Launch, class CommWork>
static int split_stage(tse_ctx* c, const char* timer, Launch launch /* (Work) */,
                       CommWork comm_work /* () on c->comm_stream */, hipEvent_t* done_out = nullptr) {
  Scope s(c, timer);
  if (!c->halo()) return launch(work_of(c, 0));
  // The two launches touch disjoint elements and depend on the same predecessors, not on each other: the interior launch goes to a
  // stream of its own (lower priority) that waits for what the compute stream has seen so far, so its first blocks fill the CUs the
  // boundary launch's last, partial round of blocks leaves idle (a rank's boundary launch is 1-3 rounds of blocks); the compute stream
  // goes on when both are done.
  hipEvent_t evA = nullptr;
  if (c->int_stream) { evA = next_sync_event(c); HIPCHK(hipEventRecord(evA, c->stream)); }
  if (launch(work_of(c, 1))) return 1;
  hipEvent_t evB = next_sync_event(c), evC = done_out ? c->ev_mm : next_sync_event(c);
  HIPCHK(hipEventRecord(evB, c->stream));
  HIPCHK(hipStreamWaitEvent(c->comm_stream, evB, 0));
  if (c->comm) { if (comm_work()) return 1; HIPCHK(hipEventRecord(evC, c->comm_stream)); }
  if (c->int_stream) {
    HIPCHK(hipStreamWaitEvent(c->int_stream, evA, 0));
    std::swap(c->stream, c->int_stream);   // (the launch closures launch on c->stream)
    const int rc = launch(work_of(c, 2));
    std::swap(c->stream, c->int_stream);
    if (rc) return 1;
    hipEvent_t evI = next_sync_event(c);
    HIPCHK(hipEventRecord(evI, c->int_stream));
    HIPCHK(hipStreamWaitEvent(c->stream, evI, 0));
  } else if (launch(work_of(c, 2))) return 1;
  if (!c->comm) { if (comm_work()) return 1; HIPCHK(hipEventRecord(evC, c->comm_stream)); }
  if (done_out) *done_out = evC;
  else { CommScope w(c, "comm_wait", c->stream); HIPCHK(hipStreamWaitEvent(c->stream, evC, 0)); }   // (the comm_wait pair brackets the wait)
  return 0;
}

// The launch that leaves Qdp(np1) and emits its element bounds for the next step (final DSS, remap), under the timer `timer`.
// prefetch: the caller knows that the next thing to happen to Qdp(np1) is the next tracer step (no remap in between), so the
// bounds exchange that step would start with is started here, under the interior part of this launch
template <class Launch>
static int launch_emitting_bounds(tse_ctx* c, const char* timer, int np1_qdp, bool prefetch, Launch launch /* (Work) */) {
  if (prefetch && c->halo() && c->lim) {
    hipEvent_t done = nullptr;
    if (split_stage(c, timer, launch, [&]() -> int { return exchange_bounds(c, c->comm_stream, c->emitted()); }, &done)) return 1;
    set_bounds_cache(c, np1_qdp);
    c->mm_halo = np1_qdp;
  } else {
    Scope s(c, timer);
    if (launch(work_of(c, 0))) return 1;
    set_bounds_cache(c, np1_qdp);
  }
  return 0;
}

// the step's inputs (vn0, eta_dot_dpdn; dp, omega_p on the first step) are being written on the auxiliary stream: wait for them
int tse::join_inputs(tse_ctx* c) {
  if (!c->inputs_pending) return 0;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_inputs, 0));
  c->inputs_pending = false;
  return 0;
}
// defer_dss: the caller launches the remap next and lets IT assemble the final DSS + time average on read (remap_launch): no
// k_dss_patch<1> here, Qdp(np1) is not written by this call
static int advec_dss_on_read(tse_ctx* c, double dts /* stage dt = dt/2 */, int n0_qdp, int np1_qdp, bool prefetch, bool defer_dss = false) {
  double* Qn0 = c->q(n0_qdp);
  double* Qnp1 = c->q(np1_qdp);
  const int nq = c->qsize * NLEV;
  const dim3 blk(FLAT_THREADS), pblk(Patch::THREADS);
  hipStream_t cs = c->comm_stream;
  // the stage's extra DSS variable travels as plane qsize of the stage's scratch output and is assembled on read by the next
  // kernel (var_in / var_out of GatherArgs): divdp_proj with stage 1, eta_dot_dpdn with stage 2, omega_p with stage 3
  auto gargs = [&](const Work& w, const double* vin = nullptr, int vin_lev = 0, double* vout = nullptr, int vout_lev = 0) {
    return c->gargs(w.order, w.nwork, w.plist, w.npwork, vin, vin_lev, vout, vout_lev);
  };
  const int nqv = nq + NLEV;   // layers of a tracer halo message with the extra variable behind the tracers

  // ---- stage 1 (rhs_multiplier 0, DSS extra = divdp_proj): bounds, neighbour min/max, advance Qdp(n0) -> T
  // (unlimited: the advance alone)
  if (c->lim) {
    const bool halo_ready = c->halo() && c->mm_valid == n0_qdp && c->mm_halo == n0_qdp;   // prefetched by the previous step / remap
    if (c->mm_valid != n0_qdp && join_inputs(c)) return 1;   // k_qminmax reads dp
    if (own_bounds(c, Qn0, c->mm_valid == n0_qdp)) return 1;
    if (halo_ready) {
      CommScope w(c, "comm_wait", c->stream);
      HIPCHK(hipStreamWaitEvent(c->stream, c->ev_mm, 0));
    } else if (c->halo()) {
      hipEvent_t ev0 = next_sync_event(c), evM = next_sync_event(c);
      HIPCHK(hipEventRecord(ev0, c->stream));
      HIPCHK(hipStreamWaitEvent(cs, ev0, 0));
      if (exchange_bounds(c, cs)) return 1;
      HIPCHK(hipEventRecord(evM, cs));
      CommScope w(c, "comm_wait", c->stream);
      HIPCHK(hipStreamWaitEvent(c->stream, evM, 0));
    }
    if (nbr_minmax_kernel(c)) return 1;
  }
  set_bounds_cache(c, 0);
  // (divdp = div(vn0) has no pass of its own here: stage 1's kernel forms it for its own slab and stores it for the later stages)
  if (join_inputs(c)) return 1;   // (the wind generator ran beside the neighbour min/max pass)
  if (split_stage(c, "advance0",
        [&](Work w) -> int {
          if (!w.nwork) return 0;
          GatherArgs ga = gargs(w, c->divdp_proj, NLEV);
          ga.divdp_out = c->divdp;
          launch_advance<0, 0, false>(stage_args(c, dim3(flat_blocks(w.nwork)), blk, dts, Qn0, nullptr, c->T, ga));
          LAUNCH_CHECK(); return 0; },
        [&]() -> int { return exchange_halo(c, cs, c->T, nqv, nqv); })) return 1;

  // ---- stage 2 (rhs_multiplier 1, DSS extra = eta_dot_dpdn): T (+) edges -> B
  if (split_stage(c, "advance1",
        [&](Work w) -> int {
          if (!w.npwork) return 0;
          launch_advance<1, 1, true>(stage_args(c, dim3(patch_blocks(w.npwork)), pblk, dts, c->T, nullptr, c->B, gargs(w, c->eta, NLEVP, c->divdp_proj, NLEV)));
          LAUNCH_CHECK(); return 0; },
        [&]() -> int { return exchange_halo(c, cs, c->B, nqv, nqv); })) return 1;

  // ---- stage 3 (rhs_multiplier 2, DSS extra = omega_p)
  // 3a: B (+) edges -> first Laplacian (pre-DSS) of the stage-2 tracers in T, element min/max (the DSS'd tracers themselves are
  //     not stored: 3b assembles them again from B); the element bounds and the Laplacian halo travel together (biharmonic_wk_scalar_minmax packs lap, Qmin, Qmax into one message: viscosity_mod.F90:389-391)
  if (split_stage(c, "lap",
        [&](Work w) -> int {
          if (!w.npwork) return 0;
          GatherArgs ga = gargs(w, nullptr, 0, c->eta, NLEVP);
          ga.pexp = c->pexp;   // only what other patches and ranks read of the first Laplacian is stored: stage 3b forms its own slots' itself
          launch_lap1<1>(stage_args(c, dim3(patch_blocks(w.npwork)), pblk, 2 * dts, c->B, nullptr, c->T, ga));
          LAUNCH_CHECK(); return 0; },
        [&]() -> int { return (c->lim && (exchange_bounds(c, cs) || unpack_minmax(c, cs))) || exchange_halo(c, cs, c->T, nq); })) return 1;
  // (no neighbour min/max pass here: 3b forms it from the element bounds -- its patch's and the element ring's -- while it runs)
  // 3b: B (+) edges, T (+) edges -> C (2nd Laplacian + biharmonic scaling + advance + limiter)
  if (split_stage(c, "advance2",
        [&](Work w) -> int {
          if (!w.npwork) return 0;
          launch_advance23(stage_args(c, dim3(patch_blocks(w.npwork)), pblk, dts, c->B, c->T, c->C, gargs(w, c->omega_p, NLEV)));   // (tse_stage3.hip)
          LAUNCH_CHECK(); return 0; },
        [&]() -> int { return exchange_halo(c, cs, c->C, nqv, nqv); })) return 1;
  if (defer_dss) {   // C (halo columns filled: the stage's exchange is ordered before the next launch on the compute stream) waits for the remap
    c->dss_deferred_n0 = n0_qdp;
    set_bounds_cache(c, 0);
    return 0;
  }
  // final DSS fused with qdp_time_avg (:645-662) and with the next step's element min/max
  return launch_emitting_bounds(c, "dss", np1_qdp, prefetch,
                                [&](Work w) -> int { return dss_tracer_launch(c, c->C, Qnp1, Qn0, w.plist, w.npwork, c->omega_p, NLEV); });
}

static int advec_step(tse_ctx* c, double dt, int n0_qdp, int np1_qdp, bool prefetch, bool defer_dss = false) {
  if (n0_qdp == np1_qdp || n0_qdp < 1 || n0_qdp > 2 || np1_qdp < 1 || np1_qdp > 2)
    return fail("advec_tracers_remap_rk2: time levels n0_qdp=%d np1_qdp=%d", n0_qdp, np1_qdp);
  const Route rt = route(c);
  if (rt.plane_over) {
    static bool said = false;
    if (!said) {
      fprintf(stderr, "transport_se_hip: a scratch plane is %zu bytes (>= %zu): DSS on read disabled, one DSS pass per stage\n", c->tps * 8, rt.plane_limit);
      said = true;
    }
  }
  if (!rt.dss_on_read && join_inputs(c)) return 1;
  if (rt.dss_on_read) {
    if (c->t_zero_dirty) {   // restore the all-zero slots of T
      const int tot = c->qsize * NCHUNK * 16 * CL;
      hipLaunchKernelGGL(k_zero_slot<>, dim3((tot + 255) / 256), dim3(256), 0, c->stream, c->qsize, c->T, c->scr(), c->zero0());
      LAUNCH_CHECK();
      c->t_zero_dirty = false;
    }
    return advec_dss_on_read(c, dt / 2, n0_qdp, np1_qdp, prefetch, defer_dss);   // (sets the bounds cache itself)
  } else {
    if (tse_compute_divdp(c)) return 1;
    if (euler_step_impl(c, np1_qdp, n0_qdp, dt / 2, 3, 0, false, 0, true)) return 1;
    if (euler_step_impl(c, np1_qdp, np1_qdp, dt / 2, 1, 1, false, 0, false)) return 1;
    if (euler_step_impl(c, np1_qdp, np1_qdp, dt / 2, 2, 2, true, n0_qdp, false)) return 1;
  }
  set_bounds_cache(c, np1_qdp);   // the final DSS emitted min/max of Qdp(np1)/dp for the next step
  return 0;
}

int tse_advec_tracers_remap_rk2(tse_ctx* c, double dt, int n0_qdp, int np1_qdp) { return advec_step(c, dt, n0_qdp, np1_qdp, false); }

// prefetch: as in launch_emitting_bounds -- the next tracer step's bounds exchange starts under the interior elements of the remap
static int remap_launch(tse_ctx* c, double dt, int np1_qdp, bool prefetch) {
  if (np1_qdp < 1 || np1_qdp > 2) return fail("vertical_remap: np1_qdp=%d", np1_qdp);
  const Route rt = route(c);
  const int nt = rt.remap_nt;
  double* Qr = c->q(np1_qdp);
  // the tracer step before left its final DSS + time average to this launch (advec_dss_on_read, defer_dss): Qr is written only
  const int fused_n0 = c->dss_deferred_n0;
  c->dss_deferred_n0 = 0;
  if (fused_n0 && (fused_n0 == np1_qdp || nt != 1)) return fail("vertical_remap: deferred DSS of time level %d cannot be assembled here", fused_n0);
  RemapFuse F{};
  if (fused_n0) F = RemapFuse{c->C, c->scr(), c->etab, c->slot_of, c->pperm, c->q(fused_n0), c->rspheremp, c->omega_p, c->zero0()};
  auto launch = [&](Work w) -> int {   // block = element
    if (!w.nwork) return 0;
    const int* list = w.order == c->ord_bnd ? c->rl_bnd : w.order == c->ord_int ? c->rl_int : c->rl_all;   // the same elements, in slot order
    return with_remap(nt, c->remap_alg2, fused_n0 != 0, [&](auto kern, int threads) -> int {
      hipLaunchKernelGGL(kern, dim3(8 * ((w.nwork + 7) / 8)), dim3(threads), sizeof(RemapLds), c->stream, c->qsize, dt, c->ps0, c->hyai, c->hybi,
                         c->dp, c->divdp_proj, c->dp3d, c->ps_v, Qr, c->bad, c->emitted().mn, c->emitted().mx, rt.remap_generic, c->sink,
                         (const double*)nullptr, list, w.nwork, c->lvl_tmp, F);
      LAUNCH_CHECK();
      return 0;
    });
  };
  if (hook_env("TSE_TEST_FAIL_REMAP")) {   // tests: this process's remap reports a negative layer thickness (one rank of several failing alone)
    static const int one = 1;
    HIPCHK(hipMemcpyAsync(c->bad, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  return launch_emitting_bounds(c, "remap", np1_qdp, prefetch, launch);   // (k_remap emits the element min/max of the remapped field)
}
// the reference's abort condition (prim_advection_mod.F90:1323): the device flag every remap since the last check ORs into
static int remap_check(tse_ctx* c) {
  int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, c->bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (bad) {
    set_bounds_cache(c, 0);
    HIPCHK(hipMemset(c->bad, 0, sizeof(int)));
    fail("negative layer thickness.  timestep or remap time too large");
    return 2;
  }
  return 0;
}
int tse_vertical_remap(tse_ctx* c, double dt, int np1_qdp) {
  c->dss_deferred_n0 = 0;   // (only tse_prim_run_subcycle defers a final DSS to its remap; a call of its that failed in between must not leave the request behind)
  if (remap_launch(c, dt, np1_qdp, false)) return 1;
  return remap_check(c);
}

// ---- single calls of the public operators the path is built from (operator-level parity; host arrays in, host arrays out) ----
template <int OP>
static int elem_op(tse_ctx* c, const double* in, size_t in_per_elem, double* out) {
  if (!in || !out) return fail("element operator: null argument");
  double *din = nullptr, *dout = nullptr;
  if (dalloc(&din, (size_t)c->nelemd * in_per_elem) || dalloc(&dout, (size_t)c->nelemd * 16)) { if (din) (void)hipFree(din); return 1; }
  int rc = 0;
  do {
    if (hipMemcpyAsync(din, in, (size_t)c->nelemd * in_per_elem * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail("element operator: H2D copy failed"); break; }
    hipLaunchKernelGGL(k_elem_op<OP>, dim3((c->nelemd * 4 + 255) / 256), dim3(256), 0, c->stream, c->nelemd, c->D, c->geo(), (const double*)din, dout);
    if (hipGetLastError() != hipSuccess) { rc = fail("element operator: kernel launch failed"); break; }
    if (hipMemcpyAsync(out, dout, (size_t)c->nelemd * 16 * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { rc = fail("element operator: D2H copy failed"); break; }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail("element operator: stream synchronisation failed"); break; }
  } while (0);
  (void)hipFree(din); (void)hipFree(dout);
  return rc;
}
int tse_divergence_sphere(tse_ctx* c, const double* v, double* div) { return elem_op<0>(c, v, 32, div); }
int tse_laplace_sphere_wk(tse_ctx* c, const double* s, double* lap) { return elem_op<1>(c, s, 16, lap); }

// remap_Q_ppm(Qdp,np,qsize,dp1,dp2) (prim_advection_mod.F90:98-214) for every local element: the column kernel of
// vertical_remap with the caller's source and target thicknesses.  Uses time level 1 of the device tracer state and the
// level fields dp/divdp_proj/dp3d as work space (a test/utility call, not part of the time loop).
int tse_remap_q_ppm(tse_ctx* c, double* Qdp, const double* dp1, const double* dp2) {
  if (!Qdp || !dp1 || !dp2) return fail("tse_remap_q_ppm: null argument");
  // before any upload or launch: a target grid the kernel's bracket search cannot end on never reaches the device (tse_tables.h)
  { std::string err; if (check_remap_grids(dp1, dp2, c->nelemd, NLEV, nullptr, &err)) return fail("tse_remap_q_ppm: %s", err.c_str()); }
  set_bounds_cache(c, 0);
  c->dcmip_static = false;   // dp is overwritten below: the next tse_dcmip_step_inputs must write the prescribed values again
  const size_t lev = c->lev();
  double* d2 = nullptr;
  if (dalloc(&d2, lev)) return 1;
  int rc = 0;
  do {
    if (hipMemcpy(c->q(1), Qdp, c->trc() * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(c->dp, dp1, lev * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d2, dp2, lev * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemset(c->divdp_proj, 0, lev * 8) != hipSuccess) { rc = fail("tse_remap_q_ppm: upload failed"); break; }
    const int generic = route(c).remap_generic;
    {
      Scope s(c, "remap_q_ppm");   // (tse_kernel_time("remap") counts it)
      with_remap(1, c->remap_alg2, false, [&](auto kern, int threads) -> int {
        hipLaunchKernelGGL(kern, dim3(8 * ((c->nelemd + 7) / 8)), dim3(threads), sizeof(RemapLds), c->stream, c->qsize, 0.0, c->ps0, c->hyai, c->hybi,
                           c->dp, c->divdp_proj, c->dp3d, c->ps_v, c->q(1), c->bad, (double*)nullptr, (double*)nullptr, generic, c->sink, (const double*)d2,
                           (const int*)nullptr, c->nelemd, c->lvl_tmp, RemapFuse{});
        return 0;
      });
    }
    if (hipGetLastError() != hipSuccess) { rc = fail("tse_remap_q_ppm: kernel launch failed"); break; }
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(Qdp, c->q(1), c->trc() * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail("tse_remap_q_ppm: download failed"); break; }
    rc = remap_check(c);
  } while (0);
  (void)hipFree(d2);
  return rc;
}

// per-element tracer mass of time level nt -> host out[nelemd][qsize] (fixed summation order inside an element; the caller adds
// the elements up reproducibly: transport_se_amd/diagnostics.py)
int tse_element_mass(tse_ctx* c, int nt, double* out) {
  if (nt < 1 || nt > 2 || !out) return fail("tse_element_mass: nt=%d", nt);
  const size_t n = (size_t)c->nelemd * c->qsize;
  double* d = nullptr;
  if (dalloc(&d, n)) return 1;
  hipLaunchKernelGGL(k_elem_mass<>, dim3((unsigned)n), dim3(ELEM_MASS_THREADS), 0, c->stream, c->qsize, (const double*)(c->q(nt)),
                     (const double*)c->spheremp, d);
  int rc = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out, d, n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) rc = fail("tse_element_mass: launch or copy failed");
  (void)hipFree(d);
  return rc;
}

// per-element shares of Qmass = integral(sum_k Qdp) and Qvar = integral(sum_k Qdp*Q) of time level nt (prim_diag_scalars,
// prim_state_mod.F90:604-655, with the ps_v the last remap left) -> host mass_out, var_out [nelemd][qsize]
int tse_element_qdiag(tse_ctx* c, int nt, double* mass_out, double* var_out, double* min_out, double* max_out) {
  if (nt < 1 || nt > 2 || !mass_out || !var_out) return fail("tse_element_qdiag: nt=%d", nt);
  const size_t n = (size_t)c->nelemd * c->qsize;
  double* d = nullptr;
  if (dalloc(&d, 4 * n)) return 1;
  hipLaunchKernelGGL(k_elem_qdiag<>, dim3((unsigned)n), dim3(64), 0, c->stream, c->qsize, (const double*)(c->q(nt)), (const double*)c->spheremp,
                     (const double*)c->ps_v, (const double*)c->hyai, (const double*)c->hybi, c->ps0, d, d + n, d + 2 * n, d + 3 * n);
  int rc = hipGetLastError() != hipSuccess;
  double* outs[4] = {mass_out, var_out, min_out, max_out};
  for (int i = 0; i < 4 && !rc; i++)
    if (outs[i]) rc = hipMemcpyAsync(outs[i], d + i * n, n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess;
  if (!rc) rc = hipStreamSynchronize(c->stream) != hipSuccess;
  if (rc) rc = fail("tse_element_qdiag: launch or copy failed");
  (void)hipFree(d);
  return rc;
}

// state%Q = Qdp(nt)/dp(ps_v) and state%lnps = log(ps_v) of the current state, on the device (prim_driver_mod.F90:803-822); the two
// fields are allocated by the first call and read by tse_copy_q_d2h / tse_copy_lnps_d2h
int tse_state_q(tse_ctx* c, int nt) {
  if (nt < 1 || nt > 2) return fail("tse_state_q: nt=%d", nt);
  auto alloc = [&](double** p, size_t n, const char* what) -> int {
    if (*p) return 0;
    const hipError_t e = hipMalloc((void**)p, n * 8);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError(); *p = nullptr;
    return fail("tse_state_q: cannot allocate %s (%.3f GB of device memory): %s", what, n * 8 / 1e9, hipGetErrorString(e));
  };
  if (alloc(&c->qmix, c->trc(), "Q") || alloc(&c->lnps, (size_t)c->nelemd * 16, "lnps")) return 1;
  c->qmix_valid = false;
  {
    Scope s(c, "stateq");
    const size_t n = (size_t)c->nelemd * NLEV * 8;
    hipLaunchKernelGGL(k_state_q<>, dim3((unsigned)((n + STATEQ_THREADS - 1) / STATEQ_THREADS)), dim3(STATEQ_THREADS), 0, c->stream, c->nelemd, c->qsize,
                       (const double*)c->q(nt), (const double*)c->ps_v, (const double*)c->hyai, (const double*)c->hybi, c->ps0, c->qmix, c->lnps);
    LAUNCH_CHECK();
  }
  c->qmix_valid = true;
  return 0;
}

// ---- the DCMIP error norms from element partials (k_norm_reference / k_norm_partials, tse_kernels.h) ----
// owner[nelemd][16], colw[nelemd][16], dh[nlev] -> device (allocated once; a later call overwrites them)
int tse_norm_setup(tse_ctx* c, const int* owner, const double* colw, const double* dh) {
  if (!owner || !colw || !dh) return fail("tse_norm_setup: null argument");
  const size_t n = (size_t)c->nelemd * 16;
  if (!c->norm_owner && dalloc(&c->norm_owner, n)) return 1;
  if (!c->norm_colw && dalloc(&c->norm_colw, n)) return 1;
  if (!c->norm_dh && dalloc(&c->norm_dh, (size_t)NLEV)) return 1;
  c->norm_ready = false;
  HIPCHK(hipStreamSynchronize(c->stream));   // (a norm kernel still running reads the old tables)
  HIPCHK(hipMemcpy(c->norm_owner, owner, n * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->norm_colw, colw, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->norm_dh, dh, (size_t)NLEV * 8, hipMemcpyHostToDevice));
  c->norm_ready = true;
  return 0;
}
static int norm_args(tse_ctx* c, const char* who, int nt, int q, const void* out) {
  if (!c->norm_ready) return fail("%s: call tse_norm_setup first", who);
  if (nt < 1 || nt > 2) return fail("%s: nt=%d", who, nt);
  if (q < 0 || q >= c->qsize) return fail("%s: tracer q=%d outside 0..%d", who, q, c->qsize - 1);
  if (!out) return fail("%s: null argument", who);
  return 0;
}
// d[n] on the device -> host out, behind everything on the stream; frees d
static int norm_fetch(tse_ctx* c, const char* who, double* d, double* out, size_t n, bool launched) {
  int rc = !launched || hipMemcpyAsync(out, d, n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess;
  if (rc) rc = fail("%s: launch or copy failed", who);
  (void)hipFree(d);
  return rc;
}
int tse_norm_reference(tse_ctx* c, int nt, int q, double* sum0) {
  if (norm_args(c, "tse_norm_reference", nt, q, sum0)) return 1;
  if (!c->qref) {
    // (TSE_TEST_FAIL_NORM_ALLOC, hooks twin only: the allocation fails on request, for the test of this message)
    const hipError_t e = hook_env("TSE_TEST_FAIL_NORM_ALLOC") ? hipErrorOutOfMemory : hipMalloc((void**)&c->qref, c->lev() * 8);
    if (e != hipSuccess) {
      (void)hipGetLastError(); c->qref = nullptr;
      return fail("tse_norm_reference: cannot allocate the reference field (%.3f GB of device memory): %s", c->lev() * 8 / 1e9, hipGetErrorString(e));
    }
  }
  double* d = nullptr;
  if (dalloc(&d, (size_t)c->nelemd)) return 1;
  c->qref_set = false;
  bool ok;
  {
    Scope s(c, "norms");
    hipLaunchKernelGGL(k_norm_reference<>, dim3((unsigned)c->nelemd), dim3(NORM_THREADS), 0, c->stream, c->qsize, q, (const double*)c->q(nt), (const double*)c->ps_v,
                       (const double*)c->hyai, (const double*)c->hybi, c->ps0, (const int*)c->norm_owner, c->qref, d);
    ok = hipGetLastError() == hipSuccess;
  }
  if (norm_fetch(c, "tse_norm_reference", d, sum0, (size_t)c->nelemd, ok)) return 1;
  c->qref_set = true;
  return 0;
}
int tse_norm_partials(tse_ctx* c, int nt, int q, double avg, double* out) {
  if (norm_args(c, "tse_norm_partials", nt, q, out)) return 1;
  if (!c->qref_set) return fail("tse_norm_partials: call tse_norm_reference first");
  double* d = nullptr;
  if (dalloc(&d, (size_t)c->nelemd * 8)) return 1;
  bool ok;
  {
    Scope s(c, "norms");
    hipLaunchKernelGGL(k_norm_partials<>, dim3((unsigned)c->nelemd), dim3(NORM_THREADS), 0, c->stream, c->qsize, q, (const double*)c->q(nt), (const double*)c->ps_v,
                       (const double*)c->hyai, (const double*)c->hybi, c->ps0, (const int*)c->norm_owner, (const double*)c->norm_colw, (const double*)c->norm_dh,
                       (const double*)c->qref, avg, d);
    ok = hipGetLastError() == hipSuccess;
  }
  return norm_fetch(c, "tse_norm_partials", d, out, (size_t)c->nelemd * 8, ok);
}

// ---- the mixing and filament diagnostics from element partials (k_mix_partials, tse_kernels.h) ----
int tse_mix_partials(tse_ctx* c, int nt, int qa, int qb, double xmin, double xmax, double c0, double c2, const double* tau, int ntau, double* out) {
#pragma clang fp contract(off)
  const char* who = "tse_mix_partials";
  if (!c->norm_ready) return fail("%s: call tse_norm_setup first", who);
  if (nt < 1 || nt > 2) return fail("%s: nt=%d", who, nt);
  for (int q : {qa, qb})
    if (q < 0 || q >= c->qsize) return fail("%s: tracer q=%d outside 0..%d", who, q, c->qsize - 1);
  if (!(xmax > xmin)) return fail("%s: xmax=%.17g <= xmin=%.17g", who, xmax, xmin);
  if (!(c2 < 0.0)) return fail("%s: c2=%.17g (the relation c0 + c2*x*x must be concave: c2 < 0)", who, c2);
  if (ntau < 0 || ntau > MIX_NTAU) return fail("%s: ntau=%d outside 0..%d", who, ntau, MIX_NTAU);
  if (!out || (ntau > 0 && !tau)) return fail("%s: null argument", who);
  // the derived values, each operation rounded once (tests/mixing_model.py: constants() forms the same bits)
  MixPar m;
  m.xmin = xmin; m.xmax = xmax; m.c0 = c0; m.c2 = c2;
  m.yhi = c0 + c2 * (xmin * xmin); m.ylo = c0 + c2 * (xmax * xmax);
  m.Rx = xmax - xmin; m.Ry = m.yhi - m.ylo;
  m.sl = (m.ylo - m.yhi) / m.Rx;
  m.kk = (m.Ry * m.Ry) / (m.Rx * m.Rx);
  m.i2 = 1.0 / ((2.0 * c2) * c2);
  for (int j = 0; j < MIX_NTAU; j++) m.tau[j] = j < ntau ? tau[j] : __builtin_huge_val();
  double* d = nullptr;
  if (dalloc(&d, (size_t)c->nelemd * MIX_OUT)) return 1;
  bool ok;
  {
    Scope s(c, "mixing");
    hipLaunchKernelGGL(k_mix_partials<>, dim3((unsigned)c->nelemd), dim3(NORM_THREADS), 0, c->stream, c->qsize, qa, qb, (const double*)c->q(nt), (const double*)c->ps_v,
                       (const double*)c->hyai, (const double*)c->hybi, c->ps0, (const int*)c->norm_owner, (const double*)c->norm_colw, (const double*)c->norm_dh, m, d);
    ok = hipGetLastError() == hipSuccess;
  }
  return norm_fetch(c, who, d, out, (size_t)c->nelemd * MIX_OUT, ok);
}

// ---- prescribed fields + device-resident driver ---------------------------------------------------
int tse_dcmip_init(tse_ctx* c, int test, const double* lat, const double* lon, const double* hyam, const double* hybm) {
  if (test != 1 && test != 2) return fail("tse_dcmip_init: test_case=%d", test);
  c->dcmip_test = test; c->dcmip_static = false;
  const double H = 287.04 * 300.0 / 9.80616, P0 = 100000.0;
  std::vector<double> hyai(NLEVP), hybi(NLEVP);
  HIPCHK(hipMemcpy(hyai.data(), c->hyai, NLEVP * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hybi.data(), c->hybi, NLEVP * 8, hipMemcpyDeviceToHost));
  std::vector<double> zm(NLEV), zi(NLEVP), pint(NLEVP), dph(NLEV);
  for (int k = 0; k < NLEVP; k++) { zi[k] = H * log(1.0 / (hyai[k] + hybi[k])); pint[k] = P0 * exp(-zi[k] / H); }
  for (int k = 0; k < NLEV; k++) {
    zm[k] = H * log(1.0 / (hyam[k] + hybm[k]));
    dph[k] = (hyai[k + 1] - hyai[k]) * c->ps0 + (hybi[k + 1] - hybi[k]) * pint[NLEV];
  }
  std::vector<double> la(lat, lat + (size_t)c->nelemd * 16), lo(lon, lon + (size_t)c->nelemd * 16);
  void* old[] = {c->lat, c->lon, c->zm, c->zi, c->pint, c->dph};
  for (void* p : old) if (p) (void)hipFree(p);
  c->lat = c->lon = c->zm = c->zi = c->pint = c->dph = nullptr;
  if (upload(&c->lat, la) || upload(&c->lon, lo) || upload(&c->zm, zm) || upload(&c->zi, zi) || upload(&c->pint, pint) || upload(&c->dph, dph)) return 1;
  if (!c->dcmip_tab && dalloc(&c->dcmip_tab, 1)) return 1;
  hipLaunchKernelGGL(k_dcmip_tables<>, dim3(1), dim3(DCMIP_TAB_THREADS), 0, c->stream, test, c->zm, c->zi, c->dcmip_tab);   // level-only factors
  LAUNCH_CHECK();
  return 0;
}
int tse_dcmip_set_initial(tse_ctx* c) {
  set_bounds_cache(c, 0);
  if (!c->dcmip_test) return fail("tse_dcmip_set_initial: call tse_dcmip_init first");
  Scope s(c, "dcmip");
  size_t tot = c->lev();
  hipLaunchKernelGGL(k_dcmip_init<>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, c->nelemd, c->qsize, c->dcmip_test, c->lat,
                     c->lon, c->zm, c->pint, c->dph, c->q(1), c->q(2), c->dp3d, c->ps_v);
  LAUNCH_CHECK();
  return 0;
}
static int dcmip_step_launch(tse_ctx* c, int nstep, double tstep, hipStream_t st) {
  if (!c->dcmip_test) return fail("tse_dcmip_step_inputs: call tse_dcmip_init first");
  Scope s(c, "dcmip", st);
  size_t tot = (size_t)c->nelemd * 16;   // one thread per column
  double t_wind = (nstep > 0 ? nstep - 1 : 0) * tstep, t_now = nstep * tstep;
  // derived%dp is rewritten with the same time-independent p_i(k+1) - p_i(k) on every step (dcmip_wrapper_mod.F90:183,199), so
  // the cached next-step bounds (formed with that dp) stay valid; every other writer of dp drops them (tse_set_derived).  That holds
  // only while dp IS the prescribed one (dcmip_static).  Otherwise this launch replaces the dp another writer left (tse_set_derived,
  // tse_view_put, tse_remap_q_ppm), and bounds a step or a remap emitted in between were formed with that other dp: they go, with their
  // prefetched halo.  (Q / lnps depend on Qdp and ps_v alone and stay fresh.)
  if (!c->dcmip_static) { c->mm_valid = 0; c->mm_halo = 0; }
  hipLaunchKernelGGL(k_dcmip_step<>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, c->nelemd, c->dcmip_test, t_wind, t_now,
                     c->lat, c->lon, c->dcmip_tab, c->pint, c->vn0, c->dcmip_static ? nullptr : c->dp, c->eta, c->dcmip_static ? nullptr : c->omega_p);
  LAUNCH_CHECK();
  c->dcmip_static = true;   // until someone else writes dp or omega_p (tse_set_derived, tse_invalidate_cache)
  return 0;
}
int tse_dcmip_step_inputs(tse_ctx* c, int nstep, double tstep) { return join_inputs(c) || dcmip_step_launch(c, nstep, tstep, c->stream); }
int tse_prim_run_subcycle(tse_ctx* c, double tstep, int nsub, int* nstep_io) {
  if (!c || !nstep_io) return fail("tse_prim_run_subcycle: null argument");
  // rsplit is the cycle length below (a modulus and a trip count): the reference's default rsplit = 0 (no vertically Lagrangian cycle,
  // control_mod.F90) has no meaning for this loop and is refused before anything is launched or any state is touched
  if (c->rsplit < 1)
    return fail("tse_prim_run_subcycle: rsplit = %d (tse_init_args), the loop needs rsplit >= 1 tracer steps per remap cycle", c->rsplit);
  c->dss_deferred_n0 = 0;
  const int nstep0 = *nstep_io;
  int nstep = nstep0;
  // The reference aborts in the first remap that meets a negative layer thickness (prim_advection_mod.F90:1323).  Here the
  // device flag is copied to page-locked memory behind every cycle's remap and looked at TWO cycles later -- by then the copy
  // has long landed, so the host never waits for the device while it keeps a full cycle queued ahead -- and the call returns 2
  // with *nstep = the step count at the end of the failing cycle (at most two more cycles were started on the bad state).
  // (With the callback form of the halo exchange every stage synchronises with the host anyway.)
  // (*nstep may lie inside an rsplit cycle -- a caller that stepped part of it through the step-by-step entries: the first of the nsub
  // cycles is then the REST of that cycle, rsplit - nstep % rsplit steps and its remap)
  const int r0 = ((nstep0 % c->rsplit) + c->rsplit) % c->rsplit;
  auto failed = [&](int cyc) -> int {
    *nstep_io = nstep0 - r0 + (cyc + 1) * c->rsplit;
    set_bounds_cache(c, 0);
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemset(c->bad, 0, sizeof(int));
    fail("negative layer thickness.  timestep or remap time too large");
    return 2;
  };
  // the remap that closes the cycle assembles the last step's final DSS + time average on read (TSE_REMAP_FUSED=0: two kernels)
  const bool fuse_remap = route(c).remap_fused;
  for (int s = 0; s < nsub; s++) {
    if (s >= 2) {
      HIPCHK(hipEventSynchronize(c->bad_ev[s & 1]));
      if (c->bad_host[s & 1]) return failed(s - 2);
    }
    int n0 = 1, np1 = 2;
    for (int r = (s == 0 ? r0 : 0); r < c->rsplit; r++) {
      // the step's inputs on the auxiliary stream, forked behind everything launched so far (the previous step / remap read what this writes)
      HIPCHK(hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
      if (dcmip_step_launch(c, nstep, tstep, c->aux_stream)) return 1;
      HIPCHK(hipEventRecord(c->ev_inputs, c->aux_stream));
      c->inputs_pending = true;   // joined by the step before its first kernel that reads them (join_inputs)
      if (nstep % 2 == 0) { n0 = 1; np1 = 2; } else { n0 = 2; np1 = 1; }  // TimeLevel_Qdp, time_mod.F90:85-109
      if (advec_step(c, tstep, n0, np1, r + 1 < c->rsplit, fuse_remap && r + 1 == c->rsplit)) return 1;   // (the remap follows the last one: its bounds would be stale)
      nstep++;
    }
    if (remap_launch(c, tstep * c->rsplit, np1, true)) { *nstep_io = nstep; return 1; }
    HIPCHK(hipMemcpyAsync(&c->bad_host[s & 1], c->bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->bad_ev[s & 1], c->stream));
  }
  *nstep_io = nstep;
  for (int s = std::max(0, nsub - 2); s < nsub; s++) {
    HIPCHK(hipEventSynchronize(c->bad_ev[s & 1]));
    if (c->bad_host[s & 1]) return failed(s);
  }
  return 0;
}

// ---- introspection ------------------------------------------------------------------------------
void* tse_device_ptr(tse_ctx* c, const char* name, size_t* nbytes) {
  struct Ent { const char* n; void* p; size_t b; };
  const size_t lev = c->lev() * 8, trc = c->trc() * 8, mm = (size_t)c->nelemd * c->mm_m() * 8, scr = (size_t)c->qsize * c->tps * 8;
  const size_t m2 = (size_t)2 * c->mm_m() * 8;
  Ent ents[] = {{"qdp1", c->q(1), trc}, {"qdp2", c->q(2), trc}, {"T", c->T, scr + c->tps * 8}, {"B", c->B, scr + c->tps * 8}, {"C", c->C, scr + c->tps * 8}, {"vn0", c->vn0, 2 * lev}, {"dp", c->dp, lev},
                {"divdp", c->divdp, lev}, {"divdp_proj", c->divdp_proj, lev}, {"eta_dot_dpdn", c->eta, (size_t)c->nelemd * NLEVP * 16 * 8},
                {"omega_p", c->omega_p, lev}, {"dp3d", c->dp3d, lev}, {"ps_v", c->ps_v, (size_t)c->nelemd * 16 * 8}, {"q", c->qmix, trc}, {"lnps", c->lnps, (size_t)c->nelemd * 16 * 8}, {"qref", c->qref, lev}, {"qmin", c->qmin, mm},
                {"qmax", c->qmax, mm}, {"sendbuf", c->sendbuf, (size_t)c->ncol_send * c->nlyr_halo * 8},
                {"recvbuf", c->recvbuf, (size_t)c->ncol_recv * c->nlyr_halo * 8}, {"sendbuf_mm", c->sendbuf_mm, (size_t)c->nmm_send * m2},
                {"recvbuf_mm", c->recvbuf_mm, (size_t)c->nmm_recv * m2}, {"remap_status", c->rv_status, (size_t)c->nelemd * c->rv_status_ints * sizeof(int)},
                {"view_stage", c->dv_stage, (size_t)c->nelemd * c->dv_layers * 16 * 8},   // (the staging field of tse_dss_view / tse_biharmonic_view: null before their first call)
                {"hypervis_stage", c->hv_stage, (size_t)c->nelemd * c->hv_layers * 16 * 8},   // (the second staging field of tse_hypervis_view: null before its first call)
                {"stats_partials", c->st_part, c->st_cap * 8}};                           // (the partials buffer of tse_stats_view: null before its first call)
  for (auto& e : ents) if (!strcmp(e.n, name)) { if (nbytes) *nbytes = e.p ? e.b : 0; return e.p; }
  if (nbytes) *nbytes = 0;
  return nullptr;
}
#ifdef TSE_AB_HOOKS
// The host tables of tse_init without a device, for the CPU tests (tests/test_tables_cpu.py): tse_test_tables builds them into *h
// (strips: as TSE_BOUNDARY_STRIPS), tse_test_table hands one out by name -- the vectors of HostTables, and "counts": ncol_send,
// ncol_recv, nmm_send, nmm_recv, nslots, cse, n_bnd, n_int, npatch, np_bnd, np_int, zero0, halo0 as ints.
struct TseTestTables { HostTables t; std::vector<int> counts; };
extern "C" int tse_test_tables(const tse_init_args* a, int strips, void** h) {
  if (!a || !h) return fail("tse_test_tables: null argument");
  *h = nullptr;
  TseTestTables* r = new TseTestTables();
  std::string err;
  if (build_tables(*a, strips != 0, &r->t, &err)) { delete r; return fail("%s", err.c_str()); }
  const HostTables& t = r->t;
  r->counts = {t.ncol_send, t.ncol_recv, t.nmm_send, t.nmm_recv, t.nslots, (int)t.cse, t.n_bnd, t.n_int, t.npatch, t.np_bnd, t.np_int,
               (int)t.zero0(), (int)t.halo0()};
  *h = r;
  return 0;
}
extern "C" int tse_test_table(void* h, const char* name, const void** data, size_t* nbytes) {
  struct Ent { const char* n; const void* p; size_t b; };
  if (!h || !name) return fail("tse_test_table: null argument");
  const TseTestTables& r = *(const TseTestTables*)h;
  const HostTables& t = r.t;
  auto ent = [](const char* n, const auto& v) { return Ent{n, v.data(), v.size() * sizeof(v[0])}; };
  const Ent ents[] = {ent("counts", r.counts), ent("send_peer", t.send_peer), ent("recv_peer", t.recv_peer), ent("send_len", t.send_len),
                      ent("recv_len", t.recv_len), ent("mm_send_len", t.mm_send_len), ent("mm_recv_len", t.mm_recv_len), ent("send_src", t.send_src),
                      ent("mm_send_src", t.mm_send_src), ent("dss_tab", t.dss_tab), ent("nbr", t.nbr), ent("order", t.order), ent("ord_bnd", t.ord_bnd),
                      ent("ord_int", t.ord_int), ent("slot_of", t.slot_of), ent("pperm", t.pperm), ent("pexp", t.pexp), ent("send_src_s", t.send_src_s),
                      ent("etab", t.etab), ent("rl_all", t.rl_all), ent("rl_bnd", t.rl_bnd), ent("rl_int", t.rl_int), ent("pslots", t.pslots),
                      ent("pring", t.pring), ent("plds", t.plds), ent("pering", t.pering), ent("pnb", t.pnb), ent("plist_bnd", t.plist_bnd),
                      ent("plist_int", t.plist_int)};
  for (const Ent& e : ents)
    if (!strcmp(e.n, name)) { if (data) *data = e.p; if (nbytes) *nbytes = e.b; return 0; }
  return fail("tse_test_table: no table named %s", name);
}
extern "C" void tse_test_tables_free(void* h) { delete (TseTestTables*)h; }
// check_remap_grids (tse_tables.h) without a device: 0, or 1 with the offender in where[3] and the message in tse_last_error()
extern "C" int tse_test_remap_grids(const double* dp1, const double* dp2, int nelem, int nlev, int* where) {
  std::string err;
  if (check_remap_grids(dp1, dp2, nelem, nlev, where, &err)) return fail("%s", err.c_str());
  return 0;
}
// The slab limiters alone (tests/test_gpu_limiter_slab.py): limiter8_quad / limiter9_quad called as k_advance calls them.  One wave per
// block; lane l owns row l & 3 of slab l >> 2 of its wave, so slab s of the batch sits in wave s / 16 and the caller chooses its
// wave-mates.  sumc is formed as k_advance forms it.  x comes back as the limiter leaves it (not x * dp), the bounds in place, the
// return value in changed.  The arrays hold whole waves (tse_test_limiter pads them).
template <int LOPT>
__global__ __launch_bounds__(64) void k_test_limiter(double* __restrict__ x, const double* __restrict__ c, double* __restrict__ minp,
                                                     double* __restrict__ maxp, int* __restrict__ changed) {
  const int s = blockIdx.x * 16 + (threadIdx.x >> 2), j = threadIdx.x & 3;
  double xr[4], cr[4];
  load4(x + (size_t)s * 16 + j * 4, xr);
  load4(c + (size_t)s * 16 + j * 4, cr);
  double mn = minp[s], mx = maxp[s];
  const double sumc = quad_sum(((cr[0] + cr[1]) + cr[2]) + cr[3]);
  const bool ch = LOPT == 9 ? limiter9_quad(xr, cr, sumc, mn, mx) : limiter8_quad(xr, cr, sumc, mn, mx);
  store4(x + (size_t)s * 16 + j * 4, xr);
  if (j == 0) { minp[s] = mn; maxp[s] = mx; changed[s] = ch; }
}
// option: 8 | 9.  x, c: [nslab][4][4] (x in/out); minp, maxp: [nslab] (in/out); changed: [nslab].  Needs no tse_ctx: it allocates, copies,
// launches and frees on the current device.  nslab is padded to whole waves with copies of the last slab.
extern "C" int tse_test_limiter(int option, int nslab, double* x, const double* c, double* minp, double* maxp, int* changed) {
  if (option != 8 && option != 9) return fail("tse_test_limiter: option %d (8 or 9)", option);
  if (nslab <= 0 || !x || !c || !minp || !maxp || !changed) return fail("tse_test_limiter: no slabs or a null argument");
  const size_t n = (size_t)nslab, npad = (n + 15) / 16 * 16;
  std::vector<double> h(npad * 34);   // x, c, minp, maxp
  double *hx = h.data(), *hc = hx + npad * 16, *hmn = hc + npad * 16, *hmx = hmn + npad;
  for (size_t s = 0; s < npad; s++) {
    const size_t f = std::min(s, n - 1);
    memcpy(hx + s * 16, x + f * 16, 128); memcpy(hc + s * 16, c + f * 16, 128);
    hmn[s] = minp[f]; hmx[s] = maxp[f];
  }
  double* d = nullptr; int* dch = nullptr;
  std::vector<int> hch(npad);
  int rc = 0;
  do {
    if (hipMalloc((void**)&d, npad * 34 * 8) != hipSuccess || hipMalloc((void**)&dch, npad * 4) != hipSuccess) { rc = fail("tse_test_limiter: cannot allocate"); break; }
    if (hipMemcpy(d, hx, npad * 34 * 8, hipMemcpyHostToDevice) != hipSuccess) { rc = fail("tse_test_limiter: upload failed"); break; }
    double *dx = d, *dc = dx + npad * 16, *dmn = dc + npad * 16, *dmx = dmn + npad;
    with_limiter(true, option, [&](auto, auto lopt) {
      hipLaunchKernelGGL(k_test_limiter<decltype(lopt)::value>, dim3((unsigned)(npad / 16)), dim3(64), 0, 0, dx, dc, dmn, dmx, dch);
    });
    if (hipGetLastError() != hipSuccess) { rc = fail("tse_test_limiter: kernel launch failed"); break; }
    if (hipDeviceSynchronize() != hipSuccess) { rc = fail("tse_test_limiter: the kernel failed"); break; }
    if (hipMemcpy(hx, d, npad * 34 * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hch.data(), dch, npad * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = fail("tse_test_limiter: download failed"); break;
    }
    memcpy(x, hx, n * 128);
    for (size_t s = 0; s < n; s++) { minp[s] = hmn[s]; maxp[s] = hmx[s]; changed[s] = hch[s]; }
  } while (0);
  if (rc) (void)hipGetLastError();
  (void)hipFree(d); (void)hipFree(dch);
  return rc;
}
// The per-step inputs without the factorisation (tests/test_gpu_dcmip_pointwise.py): dcmip_point itself at every (column, level), the
// products u * dpr, v * dpr and (-9.80616 * rho) * w formed in k_dcmip_step's operand order.  One thread per column and interface.
__global__ __launch_bounds__(256) void k_test_dcmip_point(int nelemd, int test, double t_wind, double t_now, const double* __restrict__ lat,
                                                          const double* __restrict__ lon, const double* __restrict__ zm,
                                                          const double* __restrict__ zi, const double* __restrict__ pint,
                                                          double* __restrict__ vn0, double* __restrict__ eta) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nelemd * NLEVP * 16) return;
  const int p = (int)(t & 15), k = (int)((t >> 4) % NLEVP), e = (int)(t / (NLEVP * 16));
  const double lo = lon[(size_t)e * 16 + p], la = lat[(size_t)e * 16 + p];
  const DcmipPt i = dcmip_point(test, t_now, lo, la, zi[k]);
  eta[((size_t)e * NLEVP + k) * 16 + p] = (-9.80616 * i.rho) * i.w;
  if (k < NLEV) {
    const DcmipPt m = dcmip_point(test, t_wind, lo, la, zm[k]);
    const double dpr = pint[k + 1] - pint[k];
    vn0[(((size_t)e * NLEV + k) * 2 + 0) * 16 + p] = m.u * dpr;
    vn0[(((size_t)e * NLEV + k) * 2 + 1) * 16 + p] = m.v * dpr;
  }
}
// vn0_out: [nelemd][NLEV][2][4][4], eta_out: [nelemd][NLEVP][4][4], host arrays: what tse_dcmip_step_inputs(nstep, tstep) leaves in vn0 and
// eta_dot_dpdn, evaluated point by point.  Touches no field of the context (it reads the tables of tse_dcmip_init).
extern "C" int tse_test_dcmip_point(tse_ctx* c, int nstep, double tstep, double* vn0_out, double* eta_out) {
  if (!c || !vn0_out || !eta_out) return fail("tse_test_dcmip_point: null argument");
  if (!c->dcmip_test) return fail("tse_test_dcmip_point: call tse_dcmip_init first");
  const size_t nv = (size_t)c->nelemd * NLEV * 32, ne = (size_t)c->nelemd * NLEVP * 16;
  const double t_wind = (nstep > 0 ? nstep - 1 : 0) * tstep, t_now = nstep * tstep;
  double* d = nullptr;
  int rc = 0;
  do {
    if (hipMalloc((void**)&d, (nv + ne) * 8) != hipSuccess) { rc = fail("tse_test_dcmip_point: cannot allocate"); break; }
    hipLaunchKernelGGL(k_test_dcmip_point, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, c->stream, c->nelemd, c->dcmip_test, t_wind, t_now,
                       (const double*)c->lat, (const double*)c->lon, (const double*)c->zm, (const double*)c->zi, (const double*)c->pint, d, d + nv);
    if (hipGetLastError() != hipSuccess) { rc = fail("tse_test_dcmip_point: kernel launch failed"); break; }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail("tse_test_dcmip_point: the kernel failed"); break; }
    if (hipMemcpy(vn0_out, d, nv * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(eta_out, d + nv, ne * 8, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = fail("tse_test_dcmip_point: download failed"); break;
    }
  } while (0);
  if (rc) (void)hipGetLastError();
  (void)hipFree(d);
  return rc;
}
#endif
// the two switches reset their own groups only: the comm_* groups (tse_comm_timing) and all the others (tse_timing)
static void reset_timers(tse_ctx* c, bool comm) {
  for (auto it = c->timers.begin(); it != c->timers.end();)
    if ((it->first.compare(0, 5, "comm_") == 0) == comm) it = c->timers.erase(it); else ++it;
}
int tse_timing(tse_ctx* c, int enable) { resolve_timers(c); c->timing = enable != 0; reset_timers(c, false); return 0; }
int tse_comm_timing(tse_ctx* c, int enable) { resolve_timers(c); c->comm_timing = enable != 0; reset_timers(c, true); return 0; }
int tse_kernel_time(tse_ctx* c, const char* name, double* ms, long* launches) {
  resolve_timers(c);
  double t = 0; long n = 0;
  const size_t len = strlen(name);
  for (auto& kv : c->timers)   // prefix match: "advance" = advance0 + advance1 + advance2
    if (kv.first.compare(0, len, name) == 0) { t += kv.second.ms; n += kv.second.n; }
  if (ms) *ms = t;
  if (launches) *launches = n;
  return 0;
}

#ifdef TSE_LIMITER_STATS
extern "C" int tse_debug_limiter_hist(unsigned long long* out, int reset) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(tse::g_lim_hist), sizeof(unsigned long long) * 20));
  if (reset) { unsigned long long z[20] = {0}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(tse::g_lim_hist), z, sizeof z)); }
  return 0;
}
#endif
