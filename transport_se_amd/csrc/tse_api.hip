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

#include "../../include/transport_se_hip.h"
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

static thread_local char g_err[512] = "";
static int fail(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return 1;
}
namespace tse { int set_last_error(const char* msg) { return fail("%s", msg); } }   // (tse_views.cpp: tse_view_plan)
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail("%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); } while (0)
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return fail("%s:%d %s: %s", __FILE__, __LINE__, #x, ncclGetErrorString(r_)); } while (0)

struct KTimer { double ms = 0; long n = 0; };

// the tables of the patch tiling (tse_kernels.h: Patch)
struct PatchSet {
  int npatch = 0, np_bnd = 0, np_int = 0;
  int *pslots = nullptr, *plist_bnd = nullptr, *plist_int = nullptr, *pering = nullptr;
  unsigned* pring = nullptr;
  unsigned short* plds = nullptr;
  unsigned char* pnb = nullptr;
};

struct tse_ctx {
  int nelemd = 0, qsize = 0, device = 0, rsplit = 3;
  bool remap_alg2 = false;   // control_mod vert_remap_q_alg == 2: piecewise-constant boundary cells in the PPM remap
  // control_mod limiter_option: 8 or 9 (true) or 0 (false).  Unlimited, no kernel reads or writes qmin/qmax(2): the kernels without the
  // limiter (LIM = false) run, and no element bounds are formed, exchanged or reduced over neighbours (prim_advection_mod.F90:858,880).
  // limiter_option itself picks what a limited k_advance does inside a slab (8: limiter8_quad, 9: limiter9_quad, clip-and-sum); the
  // bounds work is the same for both.
  bool lim = true;
  int limiter_option = 8;
  double nu_q = 0, ps0 = 0;
  Dvv_t D;
  hipStream_t stream = nullptr;
  // metric + tables
  double *Dinv = nullptr, *metdet = nullptr, *rmetdet = nullptr, *spheremp = nullptr, *rspheremp = nullptr;
  double *hyai = nullptr, *hybi = nullptr, *dp0 = nullptr;
  int2 *dss_tab = nullptr, *send_src = nullptr;
  int *nbr = nullptr, *order = nullptr;
  // state
  double *qlev[2] = {nullptr, nullptr};   // Qdp(:,:,:,:,1) and (:,:,:,:,2): two allocations (place_fields)
  double* q(int tl) const { return qlev[tl - 1]; }
  double *T = nullptr, *B = nullptr, *C = nullptr;   // C: third scratch field (stage-3 output of the whole-step path)
  int place_n = 0, place_sel[5] = {0, 1, 2, 3, 4};   // field placement (place_fields): chunks tried, which try became T, Qdp1, Qdp2, B, C
  double place_bw[32] = {0};                         // their streaming-write GB/s, in the order tried
  double *vn0 = nullptr, *dp = nullptr, *divdp = nullptr, *divdp_proj = nullptr, *eta = nullptr, *omega_p = nullptr;
  double *dp3d = nullptr, *ps_v = nullptr, *lvl_tmp = nullptr;
  double *qmin = nullptr, *qmax = nullptr, *qmin2 = nullptr, *qmax2 = nullptr;
  // state%Q = Qdp/dp and state%lnps of the state as tse_state_q last saw it: allocated by its first call (outside place_fields), valid
  // until the next change of Qdp or ps_v (set_bounds_cache)
  double *qmix = nullptr, *lnps = nullptr;
  bool qmix_valid = false;
  // the error norms (tse_norm_*): owner mask, column weights and layer depths of tse_norm_setup; the reference field Q0 of
  // tse_norm_reference (one tracer slot, allocated by its first call; a snapshot: no state change makes it stale)
  int* norm_owner = nullptr;
  double *norm_colw = nullptr, *norm_dh = nullptr, *qref = nullptr;
  bool norm_ready = false, qref_set = false;
  int* bad = nullptr;
  int* bad_host = nullptr; hipEvent_t bad_ev[2] = {nullptr, nullptr};   // page-locked copies of `bad`, one per cycle in flight (tse_prim_run_subcycle)
  int mm_valid = 0;   // time level (1|2) whose element min/max of Q sit in qmin2/qmax2 (emitted by the previous step), 0 = none
  int mm_halo = 0;    // == mm_valid: the neighbour ranks' share of those bounds is already in recvbuf_mm (or on its way: ev_mm)
  hipEvent_t ev_mm = nullptr;   // completion of that prefetched exchange on the communication stream
  hipEvent_t view_ev[2] = {nullptr, nullptr};   // tse_view_put / tse_view_get: the caller's stream -> compute stream -> the caller's stream (created by the first such call)
  // tse_remap_view (allocated by its first call): the check kernel's verdict per element of the latest call, [nelemd][REMAP_STATUS] ints and
  // [nelemd][2] doubles (value, limit); the accumulator of the calls that gave a stream, {count, packed first offender} (tse_remap_view_status)
  int* rv_status = nullptr;
  double* rv_detail = nullptr;
  unsigned long long* rv_acc = nullptr;
  unsigned rv_seq = 0;   // calls that gave a stream since the accumulator was last read
  // tse_dss_view (allocated by its first call, grown when a call brings more layers): the staging field [nelemd][dv_layers][16] and, on a
  // rank with neighbours, its own send and receive buffers [columns][dv_layers] -- the context's own are sized by qsize
  double *dv_stage = nullptr, *dv_send = nullptr, *dv_recv = nullptr;
  size_t dv_layers = 0;
  // tse_stats_view (allocated by its first call, grown when a call needs more): the element or level shares before they go to the host
  double* st_part = nullptr;
  size_t st_cap = 0;   // doubles
  // tse_vector_setup: the per-point tables of the vector Laplacian, [nelemd][VEC_TABS][16] (k_vec_fold; allocated by its first call)
  double* vec_tab = nullptr;
  bool vec_ready = false;
  // halo: one slot per neighbour rank (Schedule(1)%SendCycle/RecvCycle), entries per slot for the two exchange kinds
  int ncol_send = 0, ncol_recv = 0, nlyr_halo = 0;
  int nmm_send = 0, nmm_recv = 0;              // entries of the compact min/max exchange
  std::vector<int> send_peer, recv_peer, send_len, recv_len;   // kind 0: edge-buffer columns per slot
  std::vector<int> mm_send_len, mm_recv_len;                   // kind 1: (element, direction) pairs per slot
  int2* mm_send_src = nullptr;
  double *sendbuf = nullptr, *recvbuf = nullptr, *sendbuf_mm = nullptr, *recvbuf_mm = nullptr;
  tse_exchange_fn exchange = nullptr; void* exchange_user = nullptr;
  // in-library exchange: RCCL communicator + communication stream; elements that touch another rank / that do not
  ncclComm_t comm = nullptr;
  hipStream_t comm_stream = nullptr;
  hipStream_t int_stream = nullptr;   // several ranks: the interior launch of a split stage runs here, beside the boundary launch's last blocks (split_stage)
  // the prescribed-wind generator of step n+1 runs beside the neighbour min/max pass that opens the step (tse_prim_run_subcycle): its own
  // stream, forked behind the last launch of step n, joined before the first kernel that reads vn0 / eta_dot_dpdn
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_inputs = nullptr;
  bool inputs_pending = false;
  std::vector<hipEvent_t> sync_events; size_t sync_next = 0;
  int *ord_bnd = nullptr, *ord_int = nullptr;
  int n_bnd = 0, n_int = 0;
  int *rl_all = nullptr, *rl_bnd = nullptr, *rl_int = nullptr;   // the same three element sets in SLOT order: the remap's block lists (k_remap)
  // element patches of the scratch layout (tse_kernels.h): slot = patch*16 + position
  int nslots = 0;
  int* slot_of = nullptr;
  PatchSet pset;                           // the patch tiling of the DSS-on-read kernels (4 x 4 elements), also the storage order
  unsigned long long* pperm = nullptr;   // point order inside every slot of the scratch layout
  unsigned char* pexp = nullptr;         // [slot] lines of the slot that hold points read from outside its patch (k_lap1<1> stores only those)
  unsigned* etab = nullptr;              // [e][16][3] entry (within a chunk) of the DSS contributions of a point: the remap's DSS on read (RemapFuse)
  int dss_deferred_n0 = 0;               // != 0: the last tracer step left C pre-DSS for the remap to assemble; value = its n0_qdp (tse_prim_run_subcycle only)
  int2* send_src_s = nullptr;   // the send columns in slot space
  unsigned cse = 0;   // entries (points, halo columns) per chunk of a scratch plane
  bool halo() const { return ncol_send || ncol_recv; }
  // dcmip
  int dcmip_test = 0;
  bool dcmip_static = false;   // dp and omega_p hold the prescribed case's time-independent values (p_i(k+1) - p_i(k); 0, which its DSS leaves 0)
  double *lat = nullptr, *lon = nullptr, *zm = nullptr, *zi = nullptr, *pint = nullptr, *dph = nullptr;
  // page-locked range of the host's elem(:) (host_pin) + timing
  uintptr_t pin_lo = 0, pin_hi = 0;            // host range registered with tse_host_register
  double* stage[2] = {nullptr, nullptr};       // page-locked staging buffers for every other host pointer
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  bool timing = false;
  // tse_comm_timing: the comm_* groups (pack / exchange / unpack of both halo kinds, the compute stream's exposed wait); their events
  // sit on the communication stream too, and a prefetched exchange may still be in flight there when they are read (comm_pending)
  bool comm_timing = false, comm_pending = false;
  std::map<std::string, KTimer> timers;
  struct Pending { const char* name; hipEvent_t a, b; };
  std::vector<Pending> pending;       // event pairs, each on one stream, resolved lazily (no sync inside the step)
  size_t drain_at = 0;                // pending.size() at which the completed pairs are taken in (drain_timers)
  std::vector<hipEvent_t> free_events;
  double *sink = nullptr;   // write-only dump of k_remap (run-in levels of its segment tasks, surplus tracer slots): 16 columns x NLEV levels, then two bounds areas
  double *eta2 = nullptr;   // with lvl_tmp: twin buffers of the level fields (k_dss_lvl writes out of place, then swap)
  bool t_zero_dirty = false;   // the per-stage stage-3 path used T as a plain [e][q][k][p] field (overwrites its zero elements)
  size_t tps = 0;   // plane stride (doubles) of the scratch fields T and B: NCHUNK chunks of (slots, a zero slot, the halo columns)
  Scr scr() const { return Scr{tps, cse}; }
  unsigned zero0() const { return (unsigned)nslots * 16; }          // entry index of the zero slot within a chunk
  unsigned halo0() const { return (unsigned)(nslots + 1) * 16; }    // entry index of halo column 0
  GatherArgs gargs(const int* order_, int nwork_, const int* plist_, int npwork_, const double* var_in = nullptr, int var_in_lev = 0,
                   double* var_out = nullptr, int var_out_lev = 0) const {
    return GatherArgs{scr(), slot_of, order_, nwork_, rspheremp, pset.pslots, pset.pring, pset.plds, plist_, npwork_, var_in, var_in_lev, var_out, var_out_lev,
                      nullptr, pset.pering, pset.pnb, pperm, nullptr};
  }
  int mm_m() const { return mm_qpad(qsize) * NLEV; }   // entries per element of the bounds arrays (tse_kernels.h: mm_idx)
  // where the kernel that leaves Qdp(np1) (final DSS, remap) emits the element bounds of the next step; null: none are emitted, unlimited
  struct Bounds { double *mn, *mx; };
  Bounds emitted() const { return lim ? Bounds{qmin2, qmax2} : Bounds{nullptr, nullptr}; }
  size_t lev() const { return (size_t)nelemd * NLEV * 16; }
  size_t trc() const { return lev() * qsize; }
  DcmipTab* dcmip_tab = nullptr;   // level-only factors of the prescribed fields
  double* dvv_d = nullptr;   // device copy of Dvv
  GeoPtrs geo() const { return GeoPtrs{Dinv, metdet, rmetdet, spheremp, rspheremp, dvv_d}; }
};

const char* tse_last_error(void) { return g_err; }
int tse_nlev(void) { return NLEV; }

// the element bounds of Qdp(tl)/dp now sit in qmin2/qmax2 (tl = 0: nothing cached); any halo of older bounds is stale.  Every entry that
// changes Qdp or ps_v passes here, so the Q / lnps of tse_state_q go stale here too.
static void set_bounds_cache(tse_ctx* c, int tl) { c->mm_valid = c->lim ? tl : 0; c->mm_halo = 0; c->qmix_valid = false; }

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

template <class T>
static int dalloc(T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, n * sizeof(T) > 0 ? n * sizeof(T) : sizeof(T)));
  return 0;
}
// H: the host element type, the same bytes as T (tse_tables.h: I2 is uploaded as int2)
template <class T, class H>
static int upload(T** p, const std::vector<H>& h) {
  static_assert(sizeof(T) == sizeof(H) && alignof(T) >= alignof(H), "host and device element of the same layout");
  if (dalloc(p, h.size())) return 1;
  if (!h.empty()) HIPCHK(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// time a group of launches with HIP events on the launch stream (only when timing is enabled)
static hipEvent_t get_event(tse_ctx* c) {
  if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
  hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
static void take_pending(tse_ctx* c, const tse_ctx::Pending& p) {
  float ms = 0; (void)hipEventElapsedTime(&ms, p.a, p.b);
  KTimer& t = c->timers[p.name]; t.ms += ms; t.n += 1;
  c->free_events.push_back(p.a); c->free_events.push_back(p.b);
}
// A long run whose timers nobody reads would hold two events per group and launch for ever: past PENDING_DRAIN pairs, the pairs whose
// second event has completed (both events of a pair are on one stream) are taken into the timers and their events recycled, and the next
// drain waits until twice as many pairs as are still in flight have piled up.  Only hipEventQuery: the host never waits here.
static const size_t PENDING_DRAIN = 1024;
static void drain_timers(tse_ctx* c) {
  size_t k = 0;
  for (size_t i = 0; i < c->pending.size(); i++) {
    if (hipEventQuery(c->pending[i].b) == hipSuccess) take_pending(c, c->pending[i]);
    else c->pending[k++] = c->pending[i];
  }
  c->pending.resize(k);
  c->drain_at = std::max(PENDING_DRAIN, 2 * k);
  (void)hipGetLastError();   // (hipErrorNotReady of the pairs still in flight)
}
struct Scope {
  tse_ctx* c; const char* name; hipEvent_t a = nullptr; hipStream_t st;
  Scope(tse_ctx* c_, const char* n, hipStream_t st_ = nullptr) : Scope(c_, n, st_, c_->timing) {}
  Scope(tse_ctx* c_, const char* n, hipStream_t st_, bool on) : c(c_), name(n), st(st_ ? st_ : c_->stream) { if (on) { a = get_event(c); (void)hipEventRecord(a, st); } }
  ~Scope() {
    if (!a) return;
    hipEvent_t b = get_event(c);
    (void)hipEventRecord(b, st);
    c->pending.push_back({name, a, b});
    if (c->pending.size() >= std::max(PENDING_DRAIN, c->drain_at)) drain_timers(c);
  }
};
// a comm_* group (tse_comm_timing): only on a context with a halo, and nothing at all while comm timing is off
struct CommScope : Scope {
  CommScope(tse_ctx* c_, const char* n, hipStream_t st_) : Scope(c_, n, st_, c_->comm_timing && c_->halo()) { if (a) c->comm_pending = true; }
};
static void resolve_timers(tse_ctx* c) {
  if (c->pending.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  if (c->comm_pending && c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);   // (a prefetched bounds exchange may be in flight)
  c->comm_pending = false;
  for (auto& p : c->pending) take_pending(c, p);
  c->pending.clear();
}

static void gather_strided(std::vector<double>& out, const double* base, size_t stride_bytes, int n, int cnt) {
  out.resize((size_t)n * cnt);
  for (int e = 0; e < n; e++)
    memcpy(&out[(size_t)e * cnt], (const char*)base + (size_t)e * stride_bytes, sizeof(double) * cnt);
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
static std::vector<void*> device_allocations(const tse_ctx* c) {
  const PatchSet& P = c->pset;
  void* ptrs[] = {c->dcmip_tab, c->dvv_d, c->Dinv, c->metdet, c->rmetdet, c->spheremp, c->rspheremp, c->hyai, c->hybi, c->dp0, c->dss_tab, c->send_src,
                  c->nbr, c->mm_send_src, c->qlev[0], c->qlev[1], c->vn0, c->dp, c->divdp, c->divdp_proj, c->eta, c->omega_p, c->dp3d, c->ps_v,
                  c->lvl_tmp, c->eta2, c->sink, c->order, c->qmin, c->qmax, c->qmin2, c->qmax2, c->qmix, c->lnps, c->norm_owner, c->norm_colw, c->norm_dh, c->qref, c->bad, c->lat, c->lon, c->zm, c->zi, c->pint, c->dph,
                  c->sendbuf, c->recvbuf, c->sendbuf_mm, c->recvbuf_mm, c->ord_bnd, c->ord_int, c->slot_of, c->send_src_s, c->pperm, c->pexp, c->etab, c->rl_all, c->rl_bnd, c->rl_int,
                  c->T, c->B, c->C, P.pslots, P.plist_bnd, P.plist_int, P.pering, P.pring, P.plds, P.pnb, c->rv_status, c->rv_detail, c->rv_acc, c->dv_stage, c->dv_send, c->dv_recv, c->vec_tab, c->st_part};
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
static int copy_field(tse_ctx* c, double* dev, size_t cnt_dev, void* host, size_t stride, size_t cnt, bool to_device) {
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
#define LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail("%s:%d kernel launch: %s", __FILE__, __LINE__, hipGetErrorString(e_)); } while (0)

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
static int halo_exchange(tse_ctx* c, int nlyr, int kind, hipStream_t st, double* sb = nullptr, double* rb = nullptr) {
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
static int halo_items(size_t tot, unsigned* blocks) {
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
static int join_inputs(tse_ctx* c) {
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

// ---- strided device views: state exchange with a GPU-resident host ------------------------------------
// tse_view_put / tse_view_get (include/transport_se_hip.h).  The descriptor logic -- fields, extents, path, footprint, overlap -- is
// host code (tse_views.cpp); here: the checks that need the runtime, the stream ordering and the launch of one conversion kernel
// (tse_kernels.h: k_view_lines, k_view_levels, k_view_generic) on the compute stream.  Nothing is enqueued before every check has passed.
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
  const __int128 a0 = (__int128)(uintptr_t)abase, a1 = a0 + (__int128)asize, p0 = (__int128)(uintptr_t)v->ptr;
  if (p0 + (__int128)p.lo * 8 < a0 || p0 + (__int128)p.hi * 8 > a1)
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

// ---- tracer forcing: Qdp(nt) += FQ of the host, on the device (k_forcing, tse_kernels.h) --------------------------
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
  const __int128 p0 = (__int128)(uintptr_t)fq->ptr, f0 = p0 + (__int128)p.lo * 8, f1 = p0 + (__int128)p.hi * 8;
  const __int128 q0 = (__int128)(uintptr_t)c->q(nt), q1 = q0 + (__int128)c->trc() * 8;
  if (f0 < q1 && q0 < f1) return fail("%s: the view [%p%+lld, %p%+lld doubles) overlaps Qdp(%d), the field it is applied to", who, fq->ptr, p.lo, fq->ptr, p.hi, nt);
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

// ---- vertical remap of a resident host's own level fields (k_remap_view_check, k_remap_view: tse_kernels.h) ------------------------
// The plans and the overlap test are host code (tse_views.cpp: remap_view_plan); here the checks that need the runtime, the stream order
// of tse_view_put and two launches on the compute stream: the check kernel decides per element whether the bracket search can end on the
// two grids (the test of check_remap_grids, on the device: the grids never visit the host), the remap kernel leaves a refused element alone
// (its instantiation: with_remap_view, tse_launch.h).
static int remap_view_buffers(tse_ctx* c) {
  if (c->rv_acc) return 0;
  for (int i = 0; i < 8; i++) {   // (the attribute is per kernel and device; set once per context, before the first launch)
    if (with_remap_view(i & 1, i & 2, i & 4, [](auto kern, size_t lds) -> int {
          HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          return 0;
        })) return 1;
  }
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

// ---- DSS of a resident host's own fields (k_dss_view_stage, k_dss_view_sum: tse_kernels.h) -----------------------------------------
// The plan is host code (tse_views.cpp: dss_view_plan); here the checks that need the runtime and one call of stage_exchange_out, which
// tse_biharmonic_view and tse_vlaplace_view share: the stream order of tse_view_put, and on the compute stream
// stage -> (pack -> halo_exchange kind 0 with nl = nf * nk layers, on a rank with neighbours) -> out.  The staging field and the halo
// buffers are these calls' own; a steady-state call allocates nothing.
static int dss_view_buffers(tse_ctx* c, size_t nl) {
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
  a.nf = nf; a.nk = nk;
  return a;
}
// the staged field's rank-boundary columns to the neighbour ranks and theirs into dv_recv
static int stage_exchange(tse_ctx* c, size_t nl, unsigned pack_blocks) {
  CommScope w(c, "comm_wait", c->stream);   // (on the compute stream: the whole exchange is exposed)
  if (c->ncol_send) {
    CommScope sc(c, "comm_pack_q", c->stream);
    hipLaunchKernelGGL(k_pack<>, dim3(pack_blocks), dim3(256), 0, c->stream, c->ncol_send, (int)nl, c->send_src, (const double*)c->dv_stage, (const double*)nullptr,
                       c->dv_send, (int)nl, 0, (int)nl);
    LAUNCH_CHECK();
  }
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

// ---- weak Laplacian / biharmonic of a resident host's own scalar fields (k_lap_view_stage, k_lap_view_out: tse_kernels.h) ------------
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

// ---- weak vector Laplacian / biharmonic of a resident host's own wind (k_vec_fold, k_vlap_view_stage, k_vlap_view_out: tse_kernels.h) ----
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

// ---- gradient, divergence and vorticity of a resident host's own fields, local or C0 (k_sphere_op_stage: tse_kernels.h) ------------
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

// ---- min, max, sums and integrals of a resident host's fields (k_stats_view: tse_kernels.h) ------------------------------------------
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
  const std::vector<void*> mine = device_allocations(c);
  bool in_library = false;
  const char* const role[3] = {"tse_stats_view (field)", "tse_stats_view (ref)", "tse_stats_view (weight)"};   // the name a runtime refusal carries
  for (int i = 0; i < 3; i++) {
    if (!v[i]) continue;
    void* alloc = nullptr;
    if (view_runtime_checks(c, role[i], "field", p[i], v[i], stream, &alloc)) return 1;
    if (alloc == c->st_part) return fail("%s: %p lies inside the call's own partials buffer", role[i], v[i]->ptr);
    in_library = in_library || std::find(mine.begin(), mine.end(), alloc) != mine.end();
  }
  if (n > c->st_cap) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->st_part) (void)hipFree(c->st_part);
    c->st_part = nullptr; c->st_cap = 0;
    if (dalloc(&c->st_part, n)) return 1;
    c->st_cap = n;
  }
  StatsViewArgs a;
  for (int i = 0; i < 3; i++) {
    a.ptr[i] = v[i] ? (const double*)v[i]->ptr : nullptr;
    a.form[i] = v[i] ? stats_form(p[i].path, view_wide(p[i].path, v[i])) : STATS_POINTS;
    for (int k = 0; k < 5; k++) a.vs[i][k] = v[i] ? v[i]->stride[k] : 0;
  }
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

// ---- pressure, geopotential and omega / p of a resident host's columns (k_column_view: tse_kernels.h) --------------------------------
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
  const std::vector<void*> mine = device_allocations(c);
  bool in_library = false;
  const char* const role[4] = {"tse_column_view (dp)", "tse_column_view (p)", "tse_column_view (a)", "tse_column_view (b)"};   // the name a runtime refusal carries
  for (int i = 0; i < 4; i++) {
    if (!v[i]) continue;
    void* alloc = nullptr;
    if (view_runtime_checks(c, role[i], "field", pl[i], v[i], stream, &alloc)) return 1;
    in_library = in_library || std::find(mine.begin(), mine.end(), alloc) != mine.end();
  }
  if (host_array_checks(c, {{who, "out", &pl[4], out}}, stream)) return 1;
  { std::string err; if (column_view_overlap(v, pl, &err)) return fail("%s", err.c_str()); }
  ColumnViewArgs ka;
  for (int i = 0; i < 4; i++) {
    ka.ptr[i] = v[i] ? (const double*)v[i]->ptr : nullptr;
    ka.form[i] = v[i] ? stats_form(pl[i].path, view_wide(pl[i].path, v[i])) : STATS_POINTS;
    for (int k = 0; k < 5; k++) ka.vs[i][k] = v[i] ? v[i]->stride[k] : 0;
  }
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
                {"recvbuf_mm", c->recvbuf_mm, (size_t)c->nmm_recv * m2}, {"remap_status", c->rv_status, (size_t)c->nelemd * REMAP_STATUS * sizeof(int)},
                {"view_stage", c->dv_stage, (size_t)c->nelemd * c->dv_layers * 16 * 8},   // (the staging field of tse_dss_view / tse_biharmonic_view: null before their first call)
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
