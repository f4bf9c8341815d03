// tse_ctx.h -- the context of libtransport_se_hip.so and what every unit that serves the C ABI shares: tse_ctx, the error channel, the
// timer groups, the allocation helpers.  Internal (not installed): included by tse_api.hip, which owns the context and sequences the
// path, and by tse_views_api.hip, the entries that work on a resident host's own arrays.  It sees the path's kernel header only for the
// argument types the context hands out (Dvv_t, GeoPtrs, GatherArgs, Scr, DcmipTab); it launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/transport_se_hip.h"
#include "tse_kernels.h"

namespace tse {

// The one error channel of the library: writes the message tse_last_error returns (one thread_local buffer, defined in tse_api.hip)
// and returns 1.  set_last_error (tse_views.h) is a call of it.
int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// The functions of tse_api.hip the view entries call (each is described where it is defined).
void set_bounds_cache(tse_ctx* c, int tl);
int join_inputs(tse_ctx* c);
int halo_exchange(tse_ctx* c, int nlyr, int kind, hipStream_t st, double* sb = nullptr, double* rb = nullptr);
int halo_items(size_t tot, unsigned* blocks);
int pack_staged(tse_ctx* c, hipStream_t st, const double* staged, int nl, unsigned blocks, double* send);
int copy_field(tse_ctx* c, double* dev, size_t cnt_dev, void* host, size_t stride, size_t cnt, bool to_device);
std::vector<void*> device_allocations(const tse_ctx* c);

}  // namespace tse

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return tse::fail("%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); } while (0)
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return tse::fail("%s:%d %s: %s", __FILE__, __LINE__, #x, ncclGetErrorString(r_)); } while (0)

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
  tse::Dvv_t D;
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
  int rv_status_ints = 0;   // ints per element of rv_status, set with the allocation (REMAP_STATUS of tse_view_kernels.h)
  double* rv_detail = nullptr;
  unsigned long long* rv_acc = nullptr;
  unsigned rv_seq = 0;   // calls that gave a stream since the accumulator was last read
  // tse_dss_view (allocated by its first call, grown when a call brings more layers): the staging field [nelemd][dv_layers][16] and, on a
  // rank with neighbours, its own send and receive buffers [columns][dv_layers] -- the context's own are sized by qsize
  double *dv_stage = nullptr, *dv_send = nullptr, *dv_recv = nullptr;
  size_t dv_layers = 0;
  // tse_hypervis_view (allocated by its first call, grown like dv_stage): the second staging field [nelemd][hv_layers][16]
  double* hv_stage = nullptr;
  size_t hv_layers = 0;
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
  tse::Scr scr() const { return tse::Scr{tps, cse}; }
  unsigned zero0() const { return (unsigned)nslots * 16; }          // entry index of the zero slot within a chunk
  unsigned halo0() const { return (unsigned)(nslots + 1) * 16; }    // entry index of halo column 0
  tse::GatherArgs gargs(const int* order_, int nwork_, const int* plist_, int npwork_, const double* var_in = nullptr, int var_in_lev = 0,
                   double* var_out = nullptr, int var_out_lev = 0) const {
    return tse::GatherArgs{scr(), slot_of, order_, nwork_, rspheremp, pset.pslots, pset.pring, pset.plds, plist_, npwork_, var_in, var_in_lev, var_out, var_out_lev,
                      nullptr, pset.pering, pset.pnb, pperm, nullptr};
  }
  int mm_m() const { return tse::mm_qpad(qsize) * NLEV; }   // entries per element of the bounds arrays (tse_kernels.h: mm_idx)
  // where the kernel that leaves Qdp(np1) (final DSS, remap) emits the element bounds of the next step; null: none are emitted, unlimited
  struct Bounds { double *mn, *mx; };
  Bounds emitted() const { return lim ? Bounds{qmin2, qmax2} : Bounds{nullptr, nullptr}; }
  size_t lev() const { return (size_t)nelemd * NLEV * 16; }
  size_t trc() const { return lev() * qsize; }
  tse::DcmipTab* dcmip_tab = nullptr;   // level-only factors of the prescribed fields
  double* dvv_d = nullptr;   // device copy of Dvv
  tse::GeoPtrs geo() const { return tse::GeoPtrs{Dinv, metdet, rmetdet, spheremp, rspheremp, dvv_d}; }
};

template <class T>
inline int dalloc(T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, n * sizeof(T) > 0 ? n * sizeof(T) : sizeof(T)));
  return 0;
}
// H: the host element type, the same bytes as T (tse_tables.h: I2 is uploaded as int2)
template <class T, class H>
inline int upload(T** p, const std::vector<H>& h) {
  static_assert(sizeof(T) == sizeof(H) && alignof(T) >= alignof(H), "host and device element of the same layout");
  if (dalloc(p, h.size())) return 1;
  if (!h.empty()) HIPCHK(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
inline void gather_strided(std::vector<double>& out, const double* base, size_t stride_bytes, int n, int cnt) {
  out.resize((size_t)n * cnt);
  for (int e = 0; e < n; e++)
    memcpy(&out[(size_t)e * cnt], (const char*)base + (size_t)e * stride_bytes, sizeof(double) * cnt);
}

// time a group of launches with HIP events on the launch stream (only when timing is enabled)
inline hipEvent_t get_event(tse_ctx* c) {
  if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
  hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
inline void take_pending(tse_ctx* c, const tse_ctx::Pending& p) {
  float ms = 0; (void)hipEventElapsedTime(&ms, p.a, p.b);
  KTimer& t = c->timers[p.name]; t.ms += ms; t.n += 1;
  c->free_events.push_back(p.a); c->free_events.push_back(p.b);
}
// A long run whose timers nobody reads would hold two events per group and launch for ever: past PENDING_DRAIN pairs, the pairs whose
// second event has completed (both events of a pair are on one stream) are taken into the timers and their events recycled, and the next
// drain waits until twice as many pairs as are still in flight have piled up.  Only hipEventQuery: the host never waits here.
constexpr size_t PENDING_DRAIN = 1024;
inline void drain_timers(tse_ctx* c) {
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

#define LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return tse::fail("%s:%d kernel launch: %s", __FILE__, __LINE__, hipGetErrorString(e_)); } while (0)
