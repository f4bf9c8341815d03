/* transport_se_hip.h -- C ABI of the MI355X-native tracer-advection engine (libtransport_se_hip.so).
 *
 * Drop-in boundary: these entry points are what a Fortran `hip_mod` binds with ISO_C_BINDING in place of
 * the reference's CUDA-Fortran seam `cuda_mod` (reference src/share/cuda_mod.F90:57-64), which the reference
 * calls through `#if USE_CUDA_FORTRAN` hooks:
 *   cuda_mod_init(elem,hybrid,deriv,hvcoord)            prim_driver_mod.F90:686-689   -> tse_init
 *   copy_qdp_h2d(elem,nt) / copy_qdp_d2h(elem,nt)       prim_driver_mod.F90:781-784,798-801 -> tse_copy_qdp_h2d/_d2h
 *   euler_step_cuda(np1_qdp,n0_qdp,dt,elem,...,DSSopt,rhs_multiplier)
 *                                                       prim_advection_mod.F90:715-718 -> tse_euler_step
 *   qdp_time_avg_cuda(elem,rkstage,n0_qdp,np1_qdp,...)  prim_advection_mod.F90:646-656 -> tse_qdp_time_avg
 *   vertical_remap_cuda(elem,hvcoord,dt,np1,np1_qdp,..) prim_advection_mod.F90:1279-1282 -> tse_vertical_remap
 * plus the whole-step call Prim_Advec_Tracers_remap_rk2 (prim_advection_mod.F90:579-640) -> tse_advec_tracers_remap_rk2,
 * which is the fast path (one call per tracer step, everything stays in HBM).
 * The Fortran-side binding is shown in INTEGRATION.md and shipped as transport_se_amd/fortran/cuda_mod_hip.F90.
 *
 * Conventions
 *   - All functions return 0 on success, nonzero on error (the Fortran side then calls abortmp, as the
 *     reference does on every failure: parallel_mod.F90:274-287); tse_last_error() gives the message.
 *   - np = 4 and nlev are compile-time constants exactly as in the reference (dimensions_mod.F90:19,27).  nlev is a build
 *     setting of the library (-DNLEV=<n>; the multiples of 8 from 16 to 72 and 80 compile; 72, 64 and 80 are tested): TSE_NLEV below is the DEFAULT build's value
 *     (72, libtransport_se_hip.so), and a host must compare tse_nlev() with its own nlev before it passes any field.
 *   - Host arrays are passed as the address of element 1's field plus the byte stride between consecutive
 *     elements (element_t is a fixed-size derived type, element_mod.F90:112-221, so `elem(:)` is strided AoS);
 *     inside one element the reference's own memory order is assumed (i fastest, then j, k, q, time level).
 *   - Time-level arguments (n0_qdp, np1_qdp, nt) are the reference's 1-based values (time_mod.F90:85-109).
 *   - DSSopt: 1 = eta_dot_dpdn, 2 = omega_p, 3 = divdp_proj (prim_advection_mod.F90:454-457).
 *   - Edge descriptors are the reference's own: putmapP/getmapP are 0-based column offsets into the edge
 *     buffer, -1 for a missing corner neighbour, reverse is a logical (edge_mod.F90:36-43, schedule_mod.F90:905,929);
 *     direction index order west,east,south,north,swest,seast,nwest,neast (control_mod.F90:173-181).
 *   - Neighbour-rank message slots are the reference's Schedule(1)%SendCycle/RecvCycle entries
 *     (schedtype_mod.F90:7-29): peer rank (0-based), ptrP (1-based first column, as stored), lengthP (columns).
 */
#ifndef TRANSPORT_SE_HIP_H
#define TRANSPORT_SE_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TSE_NP 4
#define TSE_NLEV 72   /* the default build; the library a host loads reports its own with tse_nlev() */
#define TSE_NLEVP 73

typedef struct tse_ctx tse_ctx;

/* Exchange callback = the body of bndry_exchangeV (bndry_mod.F90:21-126): send `sendbuf` slot s
 * (len[s]*nlyr doubles at entry offset sum(len[:s]), layer index fastest) to rank send_peer[s], receive the
 * mirror-image slot into `recvbuf`.  Both pointers are DEVICE pointers.  The library has finished writing
 * sendbuf (stream-synchronised) when it calls this, and reads recvbuf only after it returns.
 *   kind 0: one entry per edge-buffer column, len[s] = lengthP of the slot (the reference's message layout);
 *   kind 1: the neighbour min/max exchange (viscosity_mod.F90:748-816): the packed fields are element constants, so one
 *           entry per neighbouring (element, direction) pair is sent instead of one per column; len[s] = the number of
 *           shared edges + shared corners with that rank (tse_halo_layout gives the totals); nlyr = 2 * nlev * (qsize rounded
 *           up to a multiple of 4): a minimum set and a maximum set in the library's bounds layout, pad tracers included -- a
 *           callback sizes its buffers by the nlyr it is given. */
typedef int (*tse_exchange_fn)(void *user, double *sendbuf, double *recvbuf, int nlyr, int kind);
/* The callback is the portable form of the seam (an MPI host keeps its own communicator: cuda_mod_hip.F90 passes
 * MPI_Isend/Irecv).  The native form is tse_comm_init below: the library then performs the exchange itself with RCCL
 * send/recv on its own streams and the callback is not used. */

typedef struct {
  int nelemd;          /* elements on this rank */
  int qsize;           /* active tracers */
  int device;          /* HIP device ordinal, -1 = current */
  double nu_q;         /* control_mod nu_q */
  int limiter_option;  /* 8: the optimization-based limiter (prim_advection_mod.F90:858,880); 9: the clip-and-sum limiter (the same bounds as
                          8: one clip to them, the clipped mass redistributed in proportion to the room left; qmin is not clamped
                          at 0); 0: no limiter (control_mod's default).  Every other value is refused.  With 0 no tracer bounds are
                          kept: tse_get_qminmax fails. */
  int rsplit;          /* control_mod rsplit (vertical remap frequency): the tracer steps per remap cycle of tse_prim_run_subcycle, the only
                          entry that reads it (the step-by-step entries leave the remap to the caller).  tse_init accepts any value; on a
                          context with rsplit < 1 (the reference's default is 0) tse_prim_run_subcycle returns nonzero with a message
                          and launches nothing */
  const double *Dvv;   /* deriv%Dvv(np,np), Fortran order */
  const double *hyai;  /* hvcoord%hyai(nlevp) */
  const double *hybi;  /* hvcoord%hybi(nlevp) */
  double ps0;          /* hvcoord%ps0 */
  /* per-element metric terms: address of elem(1)%X and byte stride to elem(2)%X */
  const double *Dinv;      size_t Dinv_stride;      /* Dinv(2,2,np,np) */
  const double *metdet;    size_t metdet_stride;    /* (np,np) */
  const double *rmetdet;   size_t rmetdet_stride;
  const double *spheremp;  size_t spheremp_stride;
  const double *rspheremp; size_t rspheremp_stride;
  /* edge descriptors, dense copies [nelemd][8] */
  const int *putmapP; const int *getmapP; const int *reverse;
  /* neighbour-rank slots (0 for a single rank) */
  int nsend; const int *send_peer; const int *send_ptrP; const int *send_lengthP;
  int nrecv; const int *recv_peer; const int *recv_ptrP; const int *recv_lengthP;
  tse_exchange_fn exchange; void *exchange_user;   /* may be NULL when nsend == nrecv == 0, or when tse_comm_init follows */
  int vert_remap_q_alg; /* control_mod vert_remap_q_alg (control_mod.F90:61-66): 0|1 = PPM with mirrored ghost cells, 2 = PPM with
                         * piecewise-constant boundary cells (prim_advection_mod.F90:230-250,283-341); anything else is refused */
} tse_init_args;

int  tse_init(tse_ctx **ctx, const tse_init_args *args);
void tse_finalize(tse_ctx *ctx);
const char *tse_last_error(void);
/* the level count (nlev) this library was built for; needs no context.  Every level extent of this interface is this value. */
int tse_nlev(void);
int  tse_synchronize(tse_ctx *ctx);

/* ---- bndry_exchangeV inside the library: RCCL neighbour send/recv over xGMI (bndry_mod.F90:74-124) ----
 * One communicator rank per tse_ctx/GPU.  Rank 0 obtains an id with tse_comm_unique_id and hands it to the other ranks
 * by whatever the host has (MPI_Bcast in a Fortran/MPI host, a torch.distributed/gloo broadcast in the Python driver);
 * every rank then calls tse_comm_init (collective).  send_peer/recv_peer of tse_init_args are ranks of this
 * communicator.  Afterwards every DSS halo is one `ncclGroupStart; ncclRecv/ncclSend per neighbour slot; ncclGroupEnd`
 * on the library's communication stream, with no host synchronisation; in the whole-step call the rank-boundary
 * elements are computed first and the exchange runs under the interior elements (the reference's
 * cuda_mod.F90:358-401,961-1005 ordering). */
#define TSE_COMM_ID_BYTES 128
int tse_comm_unique_id(void *id_out /* TSE_COMM_ID_BYTES */);
int tse_comm_init(tse_ctx *ctx, const void *id /* TSE_COMM_ID_BYTES */, int rank, int nranks);
/* Everything tse_comm_init can find wrong WITHOUT the other ranks: rank/peer ranges, device, streams, and that the RCCL this
 * process resolved can serve the headers the library was built with (same major version, point-to-point capable).  ncclCommInitRank is a blocking collective, so
 * a host calls this on every rank first, agrees on the outcome over its own control plane (MPI_Allreduce, gloo) and enters
 * tse_comm_init only when every rank is ready -- a rank that failed alone inside tse_comm_init would strand its peers. */
int tse_comm_precheck(tse_ctx *ctx, int rank, int nranks);
/* the RCCL this process runs: version code of the runtime (ncclGetVersion: major*10000 + minor*100 + patch), of the headers
 * the library was built with, and the path of the shared object that provides it (bench.py prints all three) */
int tse_comm_version(int *runtime, int *built, char *path, size_t path_len);
/* rank / size as the communicator itself reports them (ncclCommUserRank/ncclCommCount); 0/1 without a communicator */
int tse_comm_info(tse_ctx *ctx, int *rank, int *nranks);
/* give the communicator up (ncclCommAbort; no-op without one): afterwards the halo goes through the exchange callback of
 * tse_init_args again.  For a host that found tse_comm_init failing on some rank and falls back to its own transport. */
int tse_comm_abort(tse_ctx *ctx);
/* number of local elements that touch another rank (computed first in every stage) and that do not */
int tse_boundary_layout(tse_ctx *ctx, int *n_boundary, int *n_interior);
/* the same in patches (the blocks of the DSS-on-read kernels): the first launch of every stage covers the boundary patches.
 * With TSE_BOUNDARY_STRIPS=1 the rank-boundary elements are grouped into patches of their own (a two-deep band), which halves it. */
int tse_patch_layout(tse_ctx *ctx, int *np_boundary, int *np_interior);

/* Optional: declare the host's element array (elem(1) .. elem(nelemd), contiguous, alive until tse_finalize).  It is page-locked
 * once and every later field copy whose host side lies inside it is a single 2-D DMA with pitch = sizeof(element_t) straight
 * from/to elem(:); host pointers outside a registered range are staged through the library's own pinned buffers.  Returns 0 also
 * when the range is not registered (larger than TSE_PIN_LIMIT_GB, default 64, or refused by the driver). */
int tse_host_register(tse_ctx *ctx, void *base, size_t bytes);
/* elem(ie)%state%Qdp(np,np,nlev,qsize_d,2) <-> device, time level nt (1|2); qsize_d = host array extent */
int tse_copy_qdp_h2d(tse_ctx *ctx, const double *qdp_elem1, size_t elem_stride, int qsize_d, int nt);
int tse_copy_qdp_d2h(tse_ctx *ctx, double *qdp_elem1, size_t elem_stride, int qsize_d, int nt);

/* per-step inputs the caller (prim_step/prim_advance_exp) leaves in elem%derived:
 * vn0(np,np,2,nlev), dp(np,np,nlev), eta_dot_dpdn(np,np,nlevp), omega_p(np,np,nlev); one common element stride per array.
 * NULL pointers are skipped. */
int tse_set_derived(tse_ctx *ctx, const double *vn0, size_t vn0_stride, const double *dp, size_t dp_stride,
                    const double *eta_dot_dpdn, size_t eta_stride, const double *omega_p, size_t omega_stride);
/* derived%divdp / derived%divdp_proj as the host computed them (Prim_Advec_Tracers_remap_rk2 does this outside the
 * hooked routines, prim_advection_mod.F90:614-623); tse_compute_divdp is the on-device equivalent. */
int tse_set_divdp(tse_ctx *ctx, const double *divdp, size_t s0, const double *divdp_proj, size_t s1);
/* outputs the path writes back into elem: derived%divdp_proj, derived%eta_dot_dpdn (DSS'd, levels 1:nlev),
 * derived%omega_p (DSS'd), derived%divdp, state%dp3d(:,:,:,np1), state%ps_v(:,:,np1).  NULL pointers are skipped. */
int tse_get_derived(tse_ctx *ctx, double *divdp_proj, size_t s1, double *eta_dot_dpdn, size_t s2, double *omega_p, size_t s3,
                    double *divdp, size_t s4, double *dp3d, size_t s5, double *ps_v, size_t s6);

/* Prim_Advec_Tracers_remap_rk2: divdp = div(vn0); 3 x euler_step(dt/2); qdp_time_avg */
int tse_advec_tracers_remap_rk2(tse_ctx *ctx, double dt, int n0_qdp, int np1_qdp);
/* the pieces, with the reference's argument meaning */
int tse_compute_divdp(tse_ctx *ctx);
int tse_euler_step(tse_ctx *ctx, int np1_qdp, int n0_qdp, double dt, int DSSopt, int rhs_multiplier);
int tse_qdp_time_avg(tse_ctx *ctx, int rkstage, int n0_qdp, int np1_qdp);
/* vertical_remap; returns 2 on "negative layer thickness" (prim_advection_mod.F90:1323).  The reference aborts the whole
 * job there (abortmp = MPI_Abort): a caller with several ranks must escalate a return of 2 the same way (every rank
 * exits non-zero), otherwise the healthy ranks block in the next halo exchange. */
int tse_vertical_remap(tse_ctx *ctx, double dt, int np1_qdp);
/* The library caches the element min/max of Qdp(np1)/dp that the last kernel of a tracer step emits and reuses them as
 * the next step's first-stage bounds (prim_advection_mod.F90:765-779 recomputes them).  Every entry point that changes
 * Qdp or dp drops the cache -- tse_dcmip_step_inputs and tse_prim_run_subcycle too, whenever they replace a dp that another entry wrote
 * (tse_set_derived, tse_view_put, tse_remap_q_ppm) by the prescribed one; a caller that writes state through tse_device_ptr must call
 * this itself. */
int tse_invalidate_cache(tse_ctx *ctx);

/* Single calls of the public routines the path is built from, on host arrays (one call covers every local element):
 *   divergence_sphere(v,deriv,elem)        derivative_mod.F90:2364-2414   v[ie][2][np*np] -> div[ie][np*np]
 *   laplace_sphere_wk(s,deriv,elem,.true.) derivative_mod.F90:2418-2460   s[ie][np*np]    -> lap[ie][np*np]
 *   remap_Q_ppm(Qdp,np,qsize,dp1,dp2)      prim_advection_mod.F90:98-214  Qdp[ie][qsize][nlev][np*np] in place,
 *                                                                          dp1, dp2[ie][nlev][np*np]
 * They run the same device routines as the fused kernels (operator-level parity checks; not used by the time loop;
 * tse_remap_q_ppm overwrites time level 1 of the device tracer state and the dp/divdp_proj/dp3d level fields).
 * Precondition of tse_remap_q_ppm, checked on the host before anything is uploaded or launched (nonzero return, and
 * tse_last_error() names the first offending element, column and level, counted from 0): every dp1 is a finite positive number,
 * every dp2 is finite and not negative, and in every column the serial fp64 partial sums of dp2 above the last level stay below
 * sum(dp1) + 1 -- the sentinel on which remap_Q_ppm's bracket search ends (prim_advection_mod.F90:142-172; the reference assumes
 * this silently).  The last level's own sum of dp2 is not used: pin(nlev+1) is set to pio(nlev+1) = sum(dp1), and its search ends on
 * the sentinel too, so sum(dp1) + 1 must exceed sum(dp1) in fp64: a column with sum(dp1) >= 2^53 is refused as well. */
int tse_divergence_sphere(tse_ctx *ctx, const double *v, double *div);
int tse_laplace_sphere_wk(tse_ctx *ctx, const double *s, double *lap);
int tse_remap_q_ppm(tse_ctx *ctx, double *Qdp, const double *dp1, const double *dp2);

/* qmin/qmax(nlev,qsize,nelemd) module state of prim_advection_mod (:459), for inspection: out[ie][q][k].  Maintained as in the
 * reference by tse_euler_step (every stage leaves the bounds its limiter used); tse_advec_tracers_remap_rk2 keeps only what a later
 * stage reads (nothing reads them after stage 2, stage 3 and the next step recompute theirs) */
int tse_get_qminmax(tse_ctx *ctx, double *qmin, double *qmax);   /* fails on a context without a limiter (limiter_option = 0) */

/* ---- "next" rows: on-device prescribed fields + device-resident prim_run loop ---- */
/* lat/lon: elem(ie)%spherep(np,np)%{lat,lon} dense [nelemd][np*np]; hyam/hybm(nlev) */
int tse_dcmip_init(tse_ctx *ctx, int test_case /*1: dcmip1-1, 2: dcmip1-2*/, const double *lat, const double *lon,
                   const double *hyam, const double *hybm);
/* set_dcmip_*_fields(time=0) + Qdp = Q*dp for both time levels (prim_driver_mod.F90:548-556,646-669) */
int tse_dcmip_set_initial(tse_ctx *ctx);
/* what prim_step + prim_advance_exp produce for the step that starts at tl%nstep = nstep */
int tse_dcmip_step_inputs(tse_ctx *ctx, int nstep, double tstep);
/* prim_run_subcycle x nsub: rsplit x (step inputs + tracer step) + vertical_remap; *nstep is tl%nstep in/out.  *nstep may lie inside
 * an rsplit cycle (steps taken through tse_advec_tracers_remap_rk2): the first of the nsub cycles then completes that cycle.
 * Refused (nonzero, tse_last_error(), nothing launched, *nstep unchanged) on a context initialised with rsplit < 1.
 * Returns 2 on "negative layer thickness" (prim_advection_mod.F90:1323) with *nstep = the step count at the end of the FIRST
 * failing cycle; the flag is polled two cycles behind the launches (the host never waits for the device), so up to two
 * further cycles may have been started on the bad state.  Several ranks: escalate as for tse_vertical_remap. */
int tse_prim_run_subcycle(tse_ctx *ctx, double tstep, int nsub, int *nstep);

/* ---- diagnostics ---- */
/* out[ie][q] = sum_k sum_ij spheremp(i,j,ie) * Qdp(i,j,k,q,nt): the element's share of global_integral of the tracer mass
 * (global_norms_mod.F90:39-86, prim_state_mod.F90:352-385), summed in a fixed order inside the element so that it is
 * bit-identical however the elements are distributed; add the elements up with an exact / fixed-order sum for the
 * reference's task-count-independent result (repro_sum's purpose, global_norms_mod.F90:66-68). */
int tse_element_mass(tse_ctx *ctx, int nt, double *out);
/* The element shares of the two integrals prim_printstate's "Q<q>,Q diss, dQ^2/dt:" line is made of (prim_state_mod.F90:352-385):
 * mass[ie][q] = sum_ij spheremp * (sum_k Qdp) and var[ie][q] = sum_ij spheremp * (sum_k Qdp*Q), Q = Qdp/dp with
 * dp = dhyai*ps0 + dhybi*ps_v(np1) (prim_diag_scalars, :604-655; prim_driver_mod.F90:810-815), operations in the reference's order
 * (levels inside a point, then the points i fastest as global_integral adds them, global_norms_mod.F90:74-80).
 * qmin/qmax[ie][q] (may be null) = the element's minimum / maximum of Q, for the "qv=" line (:184-192). */
int tse_element_qdiag(tse_ctx *ctx, int nt, double *mass, double *var, double *qmin, double *qmax);

/* ---- the diagnostic fields prim_run_subcycle leaves in elem after the remap (prim_driver_mod.F90:803-822) ----
 * tse_state_q forms, on the device, state%Q = Qdp(nt) / dp with dp = (hyai(k+1)-hyai(k))*ps0 + (hybi(k+1)-hybi(k))*ps_v -- the reference's
 * operand order, no contraction, a true division: bit for bit the reference's host expression and the Q tse_element_qdiag takes its
 * extrema of -- and state%lnps = log(ps_v), from the current ps_v.  The two fields are allocated by the first call (one tracer-sized
 * field and one level); a context that never calls it holds neither.  They stay valid until the state changes: every entry that changes
 * Qdp or ps_v (those that drop the bounds cache, see tse_invalidate_cache, and so tse_prim_run_subcycle, tse_vertical_remap,
 * tse_dcmip_set_initial, tse_copy_qdp_h2d, tse_view_put of "qdp" or "dp", tse_remap_q_ppm, the tracer steps) makes them stale, and the two copies then return nonzero
 * instead of old data. */
int tse_state_q(tse_ctx *ctx, int nt);
/* elem(ie)%state%Q(np,np,nlev,qsize_d) <- device Q: tracers 1..qsize only, no other byte of the host element is written (same 2-D DMA /
 * staged paths as tse_copy_qdp_d2h) */
int tse_copy_q_d2h(tse_ctx *ctx, double *q_elem1, size_t elem_stride, int qsize_d);
/* elem(ie)%state%lnps(:,:,np1) <- device lnps; lnps_elem1 = address of elem(1)%state%lnps(1,1,np1) */
int tse_copy_lnps_d2h(tse_ctx *ctx, double *lnps_elem1, size_t elem_stride);

/* ---- state exchange with a GPU-resident host: strided DEVICE views (no byte crosses the host link) ----
 * A view describes the host's own device array of one field: the device address of its first entry and, in doubles, the stride of each
 * of the five axes element, q (tracer; the wind component for "vn0"), level, j, i.  An axis the field does not have (q for the level
 * fields; q and level for "ps_v" / "lnps") carries stride 0.  The library side is always its dense internal array; the copy is a bit copy.
 *   tse_view_put   host view -> library.  Fields: "qdp" (time level nt, 1|2), "vn0" (q extent 2), "dp", "eta_dot_dpdn" (nlev+1 levels),
 *                  "omega_p", "divdp", "divdp_proj" -- what tse_copy_qdp_h2d, tse_set_derived and tse_set_divdp write, with the same side
 *                  effects as those: "qdp" and "dp" drop the cached element bounds and make Q / lnps stale, "dp" and "omega_p" end the
 *                  prescribed case's static inputs.  A zero stride broadcasts.
 *   tse_view_get   library -> host view.  Fields: "qdp" (nt), "q" and "lnps" (refused as stale under the rule of tse_copy_q_d2h), and the six
 *                  of tse_get_derived: "divdp_proj", "eta_dot_dpdn" (levels 1..nlev only: the view has nlev levels), "omega_p", "divdp",
 *                  "dp3d", "ps_v".  Only the addresses of the view are written (padding keeps its bytes).  No two index tuples of the view may
 *                  share an address; this is decided by the nested-extent test (the axes sorted by |stride|, each stride at least the previous
 *                  stride times its extent), which is conservative: it never accepts an overlapping view.  Zero strides are refused.
 * nt is ignored for fields with one time level.
 * stream is the caller's hipStream_t (void * keeps this header free of HIP includes).  Not null: the library's compute stream waits for
 * what the caller's stream holds at the call, the conversion runs on the compute stream, and the caller's stream waits for it -- no host
 * synchronisation; the source's producer, a caller that reuses the source after a put, and the consumer after a get are all ordered.
 * Null: the call is complete on return, as the host copies are (the source must be ready: the compute stream orders itself behind the
 * legacy default stream only).  A stream that is being captured, or one of another device, is refused.
 * Before anything is enqueued: field and direction, nt, null pointers; v->ptr must be device memory of the context's device
 * (hipPointerGetAttributes) and the footprint of the view must lie inside the allocation that holds ptr (hipMemGetAddressRange).  On
 * failure: nonzero, tse_last_error(), nothing enqueued.  Timer group "view".
 *   tse_view_plan  needs no context and no device: the path put/get take for this view -- 0 point-fastest (stride i = 1, j = 4: 128-byte
 *                  lines on both sides), 1 level-fastest (stride level = 1, i = S, j = 4S, S >= the level extent: transposed through LDS),
 *                  2 anything else (one address computation per entry) -- and the footprint [lo, hi) in doubles relative to ptr
 *                  (v->ptr itself is not read).  Nonzero with a message naming the axis for a view put/get would refuse. */
typedef struct {
  void *ptr;            /* DEVICE address of the entry (element 0, q 0, level 0, j 0, i 0) */
  long long stride[5];  /* in doubles: element, q (tracer, or wind component for "vn0"), level, j, i */
} tse_view;
int tse_view_put(tse_ctx *ctx, const char *field, int nt, const tse_view *v, void *stream);
int tse_view_get(tse_ctx *ctx, const char *field, int nt, const tse_view *v, void *stream);
int tse_view_plan(const char *field, int nelemd, int qsize, const tse_view *v, int for_get,
                  int *path, long long *lo, long long *hi);

/* ---- tracer forcing: the physics step between two tse_prim_run_subcycle calls (E3SM's applyCAMforcing_tracers; the reference carries
 * derived%FQ, element_mod.F90:69, and never applies it) ----
 * For every element, tracer q < qsize, level and point of Qdp = Qdp(nt), these operations in this order, none contracted:
 *   mode TSE_FORCING_TENDENCY:  v = dt * FQ
 *   mode TSE_FORCING_ADJUST:    dpk = (hyai(k+1)-hyai(k))*ps0 + (hybi(k+1)-hybi(k))*ps_v;  Q = Qdp / dpk;  v = dpk * (FQ - Q)
 *                               (dp and Q as tse_state_q forms them: FQ is the new mixing ratio, dt is ignored)
 *   asked = v;  if (Qdp + v < 0 && v < 0) v = (Qdp < 0) ? 0.0 : -Qdp;  Qdp(nt) = Qdp + v
 * so no tracer mass is made negative and a negative one (a limiter-sized undershoot) is left alone.  Inputs are finite: a NaN propagates,
 * nothing is checked on the device.
 * fq is a view of the shape and under the rules of a "qdp" put view (tse_view_plan("qdp", nelemd, qsize, fq, 0, ...) gives its path and
 * footprint; the same three paths; a zero stride broadcasts) and every check tse_view_put makes before it enqueues applies unchanged.
 * Refused besides: mode outside 0|1, a dt that is not finite, and a view whose footprint overlaps the library's Qdp(nt).  On failure:
 * nonzero, tse_last_error(), nothing enqueued.
 * stream orders as in tse_view_put (not null: wait for it, run on the compute stream, make it wait; null: complete on return).
 * budget may be null; otherwise a HOST array [nelemd][qsize][2]: entry 0 = sum spheremp[p] * v, the mass applied, entry 1 =
 * sum spheremp[p] * (asked - v), the mass the clip withheld (exactly 0 where nothing was clipped), both over the 16 points and all levels,
 * every term formed without contraction and added in the order of k_norm_partials (csrc/tse_kernels.h), so a share depends on the
 * element's own data alone.  With a budget the call is complete on return whatever stream is.
 * Side effects: those of tse_copy_qdp_h2d -- the cached element bounds are dropped, Q / lnps become stale; the prescribed case's static
 * inputs, the norm reference and the norm setup are untouched.  Timer group "forcing". */
#define TSE_FORCING_TENDENCY 0
#define TSE_FORCING_ADJUST   1
int tse_apply_forcing(tse_ctx *ctx, int nt, double dt, int mode, const tse_view *fq, void *stream, double *budget);
/* The same for a host whose elem(:) lives in host memory: fq_elem1 = the address of elem(1)%derived%FQ(1,1,1,1,tl), elem_stride the byte
 * stride between elements, qsize_d the host array's tracer extent.  FQ crosses by the path of tse_copy_qdp_h2d (2-D DMA from a registered
 * range, pinned staging otherwise) into the device Q field of tse_state_q, which this call leaves stale anyway (allocated here when no
 * tse_state_q has run: a context that forms Q holds no more memory than before); then the same kernel.  Complete on return. */
int tse_apply_forcing_host(tse_ctx *ctx, int nt, double dt, int mode, const double *fq_elem1, size_t elem_stride, int qsize_d, double *budget);

/* ---- vertical remap of a GPU-resident host's OWN level fields (E3SM vertical_remap -> remap1 = remap_Q_ppm, prim_advection_mod.F90:98-214) ----
 * For every element, field slot f < nf and column: remap_Q_ppm(field, np, nf, dp_src, dp_tgt) with vert_remap_q_alg = alg (0 or 1: mirrored
 * ghost cells; 2: piecewise-constant end cells; anything else is refused; independent of the context's own setting), in place in the
 * host's device array.  The result is the fixed sequence of roundings of the library's remap kernel: bit for bit what tse_remap_q_ppm
 * returns for the same column on the same grids, whatever path the views take.
 *   mode TSE_REMAP_MASS  the field is mass per layer (Qdp, u*dp)
 *   mode TSE_REMAP_MEAN  the field is a layer mean a (T, u): m = a * dp_src (one product) as a cell is read, the mass arithmetic, a' = m' /
 *                        dp_tgt (a true division) as it is written -- the bits of the host's  ttmp = T*dp_star; remap1; T = ttmp/dp
 * field: shape and rules of a "qdp" GET view with tracer extent nf (any nf >= 1, whatever the context's qsize; the q axis is whatever the
 * host stacks: u and v are nf = 2): no zero stride, no two index tuples on one address.  Only the addresses of the view are written.
 * dp_src, dp_tgt: shape and rules of a "dp" PUT view (a zero stride broadcasts).  Every view takes its own path of tse_view_plan.
 * Library state: none is read or written -- not Qdp, dp, divdp, divdp_proj, dp3d, ps_v, the cached bounds, Q / lnps or the norm fields.
 * One exception: a field whose footprint lies inside the library's "qdp1" or "qdp2" allocation (tse_device_ptr) is accepted, with the
 * side effects of tse_copy_qdp_h2d (cached bounds dropped, Q / lnps stale); a view that meets any other allocation of the library is refused.
 * Before anything is enqueued, as in tse_view_put (nonzero, tse_last_error(), nothing launched): null pointers, nf < 1, mode or alg out of
 * range, device memory of the context's device, every footprint inside its allocation, the field overlapping neither grid, a stream that
 * is being captured or belongs to another device.
 * Bad grids are decided on the device, per element (the grids of a resident host never visit the host): 1 a dp_src that is not a finite
 * positive number; 2 sum(dp_src) not finite, or so large that sum + 1 == sum; 3 a dp_tgt that is negative or not finite (MEAN: or zero);
 * 4 a partial sum of dp_tgt below the last level that reaches sum(dp_src) + 1 -- the precondition of the bracket search, the test of
 * tse_remap_q_ppm.  A refused element's field keeps every bit; the other elements are remapped.
 * stream orders as in tse_view_put.  stream == NULL: complete on return; returns 2 if any element was refused, tse_last_error() names the
 * lowest one.  Otherwise 0 after enqueueing, and tse_remap_view_status waits for the compute stream and reports what such calls refused
 * since it was last read: the count of elements, and in where[4] the element, column, level (from 0) and code of the lowest element of the
 * earliest call that refused one; then it clears.  (After a NULL-stream call tse_device_ptr "remap_status" holds [nelemd][4] ints: code,
 * column, level and a flag for the message, of that call.)  Timer group "fieldremap". */
#define TSE_REMAP_MASS 0
#define TSE_REMAP_MEAN 1
int tse_remap_view(tse_ctx *ctx, int nf, int mode, int alg, const tse_view *field, const tse_view *dp_src, const tse_view *dp_tgt, void *stream);
int tse_remap_view_status(tse_ctx *ctx, int *nrefused, int where[4] /* element, column, level, code */);
/* the path and the footprint [lo, hi) (doubles relative to ptr) of field, dp_src, dp_tgt, and every refusal that needs no device: nf, the
 * extent rules, a zero stride in field, and the field overlapping a grid (the ptr members may be offsets into one allocation; with all three
 * null only the strides are judged).  No context. */
int tse_remap_view_plan(int nelemd, int nf, const tse_view *field, const tse_view *dp_src, const tse_view *dp_tgt,
                        int path[3], long long lo[3], long long hi[3]);

/* ---- direct stiffness summation (DSS) of a GPU-resident host's OWN fields: the reference's spheremp*f -> edgeVpack -> bndry_exchangeV ->
 * edgeVunpack -> rspheremp* idiom (prim_advection_mod.F90:911-960, edge_mod.F90:366-511,648-742), in place in the host's device array ----
 * field: nf fields (the q axis of the view: whatever the host stacks; any nf >= 1, whatever the context's qsize; u and v are nf = 2) of nk
 * levels each, 1 <= nk <= nlev + 1 (a surface field, a layer field, an interface field; every layer is summed).  For every layer and every
 * GLL point p of element e
 *     out = rspheremp[e][p] * (((w + c0) + c1) + c2)
 *   mode TSE_DSS_AVERAGE  w = spheremp * f, one stored product (a nodal field: u, T, dp3d, ps_v)
 *   mode TSE_DSS_WEAK     w = f (f carries the mass weight already: the result of a weak operator)
 * c0..c2 are the contributions of the points that share the node, in the reference's order of unpacking (edges S, E, N, W, then the
 * corner); an absent one adds +0.0; one from another rank is the w that rank packed.  Nothing is contracted, so the result has the bits of
 * rspheremp * DSS(w) of the tracer engine's own DSS on every path of the view and on any number of ranks.
 * View rules: those of a "qdp" get view (tse_view_plan) with nf and nk in place of qsize and nlev -- no zero stride on an axis of extent
 * above 1 (an axis of extent 1 may carry stride 0), the axes nest so that no two index tuples share an address, device memory of the
 * context's device, the footprint inside the allocation that holds ptr, a stream that is not being captured and belongs to this device.
 * Refused besides: mode outside 0|1, nf < 1, nk outside 1..nlev+1, and a view inside any allocation of the library (qdp1 / qdp2 and this
 * call's own staging buffers included: the call works on the host's arrays).  On failure: nonzero, tse_last_error(), nothing enqueued.
 * Only the addresses of the view are written.  No library state is read or written: not Qdp, the level fields, the cached element bounds
 * or the freshness of Q / lnps.
 * Paths (tse_dss_view_plan): 0 point-fastest; 1 level-fastest (stride level = 1, i = S >= nk, j = 4S) for nk == nlev, through LDS; 2 any
 * other strides, and a level-fastest view with another nk.  The three give the same bits.
 * COLLECTIVE: on a context with neighbour ranks every rank makes the call, with the same nf, nk and mode, in the same order relative to
 * the other exchanging calls.  It uses the context's own exchange (the RCCL communicator of tse_comm_init, or the callback, kind 0) with
 * nf * nk layers per column; staging and halo buffers are the call's own, allocated by the first call, grown when a call brings more
 * layers, freed by tse_finalize.
 * stream orders as in tse_view_put (not null: wait for it, run on the compute stream, make it wait; null: complete on return).  Nothing
 * waits on the CPU on one rank or with RCCL; the callback exchange drains the compute stream first, as everywhere.
 * Timer group "fielddss" (two launches per call: stage and sum); pack and exchange count under comm_pack_q / comm_exchange_q / comm_wait. */
#define TSE_DSS_AVERAGE 0
#define TSE_DSS_WEAK    1
int tse_dss_view(tse_ctx *ctx, int nf, int nk, int mode, const tse_view *field, void *stream);
/* the path and the footprint [lo, hi) (doubles relative to ptr) such a view gets, and every refusal that needs no device (nf, nk, a zero
 * stride on an extent above 1, a view that may overlap itself, a null view).  No context, no device. */
int tse_dss_view_plan(int nelemd, int nf, int nk, const tse_view *field, int *path, long long *lo, long long *hi);

/* ---- weak Laplacian and biharmonic of a GPU-resident host's OWN scalar fields: the scalar half of its hyperviscosity, the reference's
 * laplace_sphere_wk (derivative_mod.F90:2418-2460, constant coefficient) and biharmonic_wk_scalar / the T and dp3d part of
 * biharmonic_wk_dp3d (viscosity_mod.F90:315-344, 229-279) on every layer of nf fields of nk levels, 1 <= nk <= nlev + 1 ----
 *   order TSE_LAPLACE     out = laplace_sphere_wk(in): weak (it carries spheremp), not summed over elements; no exchange, not collective
 *   order TSE_BIHARMONIC  w = laplace_sphere_wk(in);  m[p] = rspheremp[e][p] * (((w + c0) + c1) + c2), tse_dss_view's TSE_DSS_WEAK sum (table
 *                         order, +0.0 for an absent contribution, the sender's packed w for a remote one);  out = laplace_sphere_wk(m)
 * The Laplacian is tse_laplace_sphere_wk's own device routine, nothing contracted beyond what it spells out, so every slab of order 1 has
 * that entry's bits and order 2 has the bits of tse_laplace_sphere_wk -> tse_dss_view(TSE_DSS_WEAK) -> tse_laplace_sphere_wk, on one rank or
 * many and on every path of either view.  The result is the weak tendency BEFORE the final DSS: the host multiplies by -nu * dt and follows
 * with tse_dss_view(..., TSE_DSS_WEAK, ...), as advance_hypervis does.  No nu, no dp0 scaling, no hypervis_scaling tensor; the vector
 * Laplacian of u and v is not part of this entry.
 * Views: `in` and `out` each obey the rules of tse_dss_view's view and each takes its own path (0 point-fastest, 1 level-fastest for
 * nk == nlev, 2 anything else).  out may be the same view as in -- the same ptr and the same five strides: in place, like the reference's
 * qtens -- otherwise the two footprints [lo, hi) must be disjoint; any other overlap is refused.  Only the addresses of out are written;
 * with a separate out, in keeps every bit.  Refused besides: order outside 1|2, nf < 1, nk outside 1..nlev+1, either view inside an
 * allocation of the library (the staging buffers included).  On failure: nonzero, tse_last_error(), nothing enqueued.
 * No library state is read or written; the staging and halo buffers are tse_dss_view's, grown when a call brings more layers, so a
 * steady-state call allocates nothing.
 * COLLECTIVE for order 2 on a context with neighbour ranks, as tse_dss_view (exchange kind 0 with nf * nk layers); order 1 never exchanges.
 * stream orders as in tse_dss_view (not null: wait for it, run on the compute stream, make it wait; null: complete on return; a stream
 * under capture or of another device is refused).
 * Timer group "fieldlap" (two launches per call for either order: the stage kernel, in -> first Laplacian -> staging field, and the out
 * kernel, staging field -> [sum, rspheremp, second Laplacian] -> out); pack and exchange count under comm_pack_q / comm_exchange_q / comm_wait. */
#define TSE_LAPLACE    1   /* out = laplace_sphere_wk(in): weak, not summed; no exchange, not collective */
#define TSE_BIHARMONIC 2   /* out = laplace_sphere_wk(rspheremp * DSS(laplace_sphere_wk(in))): collective like tse_dss_view */
int tse_biharmonic_view(tse_ctx *ctx, int nf, int nk, int order, const tse_view *in, const tse_view *out, void *stream);
/* the paths and footprints [lo, hi) (doubles relative to each ptr) of in ([0]) and out ([1]), and every refusal that needs no device; the
 * overlap rule is applied when either ptr is not null.  Host only: no context, no device. */
int tse_biharmonic_view_plan(int nelemd, int nf, int nk, const tse_view *in, const tse_view *out,
                             int path[2], long long lo[2], long long hi[2]);

/* ---- weak vector Laplacian and biharmonic of a GPU-resident host's OWN wind: the vector half of its hyperviscosity, the reference's
 * vlaplace_sphere_wk in its constant-coefficient branch vlaplace_sphere_wk_contra (derivative_mod.F90:2545-2591, hypervis_scaling == 0) and
 * the wind's line of biharmonic_wk_dp3d (viscosity_mod.F90:177-286), on nk levels of the two components of one view, 1 <= nk <= nlev + 1 ----
 *   lap(v) = gradient_sphere_wk_testcov(nu_ratio * divergence_sphere(v)) - curl_sphere_wk_testcov(vorticity_sphere(v))
 *            + 2 * spheremp * v * rrearth^2                       (rigid rotation is not damped)
 *   order TSE_VLAPLACE     out = lap(in): weak (it carries spheremp), not summed over elements; no exchange, not collective
 *   order TSE_VBIHARMONIC  w = lap(in);  m_c[p] = rspheremp[e][p] * (((w_c + c0) + c1) + c2) per component, tse_dss_view's TSE_DSS_WEAK sum over
 *                          2 * nk layers;  out = lap(m).  nu_ratio multiplies div in BOTH Laplacians (the reference's nu_ratio1 = nu_ratio2
 *                          for hypervis_scaling == 0, its "applied twice"); the product is always formed, with 1.0 it changes no bit.  Two
 *                          different ratios: order 1, tse_dss_view(TSE_DSS_WEAK, nf = 2), order 1.
 * tse_vector_setup brings the three element fields the operator needs and tse_init_args does not carry: elem(ie)%D(2,2,np,np),
 * elem(ie)%metinv(2,2,np,np), elem(ie)%mp(np,np), each as the address of elem(1)%X and the byte stride to elem(2)%X.  They are copied to the
 * device and folded there, once, with the library's Dinv, metdet, rmetdet and spheremp into 14 tables per point (csrc/tse_device.h:
 * vlaplace_row), so the metric products are re-associated and the result need not have the reference's bits.  What holds: the routine is
 * compiled without implicit contraction, so a point's result is one fixed sequence of roundings -- it does not depend on the path of either
 * view, on the other levels of the call, on the slab's neighbours in the wavefront or on the number of ranks -- and order 2 has the bits of
 * order 1 -> tse_dss_view(TSE_DSS_WEAK, nf = 2) -> order 1.  tse_vector_setup may be called again; it completes on return.
 * Views: `in` and `out` are views of tse_dss_view with nf = 2; the q axis is the wind component, as for "vn0" (E3SM's
 * state%v(np,np,2,nlev,tl): component stride 16, level stride 32, one call per time level).  Each takes its own path; out is the same view
 * as in (in place) or has a disjoint footprint; only the addresses of out are written.  Everything tse_biharmonic_view refuses is refused
 * here, and besides: a call before tse_vector_setup, an nu_ratio that is not finite.  On failure: nonzero, tse_last_error(), nothing enqueued.
 * The result is the weak tendency BEFORE the final DSS: the host multiplies by -nu * dt and follows with tse_dss_view(TSE_DSS_WEAK).
 * Not part of this entry: the tensor / cartesian branch (hypervis_scaling > 0), variable_hyperviscosity, subcell_Laplace_fluxes.
 * No library state is read or written except the tables of tse_vector_setup; the staging and halo buffers are tse_dss_view's ("view_stage",
 * grown when a call brings more layers, here 2 * nk), so a steady-state call allocates nothing.  COLLECTIVE for order 2 on a context with
 * neighbour ranks (exchange kind 0 with 2 * nk layers); order 1 never exchanges.  stream orders as in tse_dss_view.
 * Timer group "fieldvlap" (two launches per call for either order: the stage kernel, in -> first Laplacian -> staging field, and the out
 * kernel, staging field -> [sum, rspheremp, second Laplacian] -> out); pack and exchange count under comm_pack_q / comm_exchange_q / comm_wait. */
int tse_vector_setup(tse_ctx *ctx, const double *D, size_t D_stride, const double *metinv, size_t metinv_stride,
                     const double *mp, size_t mp_stride);
#define TSE_VLAPLACE    1   /* out = vlaplace_sphere_wk(in): weak, not summed; no exchange, not collective */
#define TSE_VBIHARMONIC 2   /* out = vlaplace_sphere_wk(rspheremp * DSS(vlaplace_sphere_wk(in))): collective like tse_dss_view */
int tse_vlaplace_view(tse_ctx *ctx, int nk, int order, double nu_ratio, const tse_view *in, const tse_view *out, void *stream);
/* the paths and footprints of in ([0]) and out ([1]) and every refusal that needs no device, as tse_biharmonic_view_plan with nf = 2 */
int tse_vlaplace_view_plan(int nelemd, int nk, const tse_view *in, const tse_view *out, int path[2], long long lo[2], long long hi[2]);

/* ---- one hyperviscosity sub-step of a GPU-resident host's OWN scalars and wind in one call: the body of advance_hypervis's subcycle
 * loop for hypervis_scaling == 0 -- biharmonic_wk_dp3d (viscosity_mod.F90:229-279: ONE edge buffer for ptens, vtens and dptens, one
 * bndry_exchangeV), the factors -nu * dt / hypervis_subcycle, the final DSS (a second single exchange) and the update of the state ----
 *   per point of scalar field f (x = s) and of each wind component (x = v), one fixed sequence of roundings, nothing contracted:
 *     w = lap(x)                                  the staged first Laplacian of tse_biharmonic_view / tse_vlaplace_view
 *     b = lap(rspheremp * (((w + c0) + c1) + c2)) the bits of tse_biharmonic_view(TSE_BIHARMONIC) / tse_vlaplace_view(TSE_VBIHARMONIC, nu_ratio)
 *     t = coef * b                                one product, always formed: coef[f] for scalar field f, coef[nf] for the wind
 *     d = rspheremp * (((t + c0) + c1) + c2)      the bits of tse_dss_view(TSE_DSS_WEAK) on t
 *     in place (s_out and v_out NULL): x <- x + d, one addition;  with out views: out <- d, x keeps every bit
 * so the call has the bits of tse_biharmonic_view -> product -> tse_dss_view(TSE_DSS_WEAK) -> addition (and the same with
 * tse_vlaplace_view), on every path of every view, for a level alone or among others, on one rank or many.
 * s: nf >= 0 scalar fields of nk levels under the rules of tse_biharmonic_view's `in` (E3SM's T and dp3d, two members of elem(:) at one
 * element stride, are ONE view whose q stride is the distance between the members); nf <= TSE_HYPERVIS_MAX_FIELDS.  v: the wind under
 * the rules of tse_vlaplace_view's `in`; it needs tse_vector_setup.  Either may be absent -- nf = 0 with s = NULL, or v = NULL -- not both.
 * 1 <= nk <= nlev + 1; each view takes its own path.  coef: nf + 1 doubles of the host, formed there in double (-nu_s * dt /
 * hypervis_subcycle, -nu_p * ... for dp3d, the wind's last), each finite; coef[nf] is not read when v is NULL.
 * s_out, v_out: both NULL, or given for exactly the inputs that are present (a host that needs vtens itself: E3SM's frictional heating
 * -(v . vtens) / cp); views of the shape of their input.  Every two views of a call are disjoint: their footprints do not meet, or --
 * members of one elem(:), which interleave -- they have the same element stride and their footprints within one element are disjoint
 * and lie together inside one element stride.  Only addresses of s and v (in place) or of the out views are written.
 * Not in this call: the heating itself, nu_top, hypervis_scaling > 0, subcell_Laplace_fluxes, two different nu_ratios.
 * Refused, with nonzero return, tse_last_error() and nothing enqueued: everything tse_biharmonic_view or tse_vlaplace_view refuses for
 * any of the views, the overlap and presence rules above, v before tse_vector_setup, a coef or nu_ratio that is not finite, a stream
 * under capture or of another device, a view inside an allocation of the library, nelemd * (nf + 2) * nk >= 2^27.
 * Device: at most five launches (the two first Laplacians, the two second ones, ONE final kernel for both halves) and, on a context with
 * neighbour ranks, exactly TWO exchanges (kind 0) of nl = (nf + 2) * nk layers (nf * nk without v) -- the loop of the separate entries
 * makes four.  COLLECTIVE there: every rank calls with the same nf, nk and presence of v, in the same order among the exchanging calls.
 * The first staging field and the halo buffers are tse_dss_view's ("view_stage"); the second staging field ("hypervis_stage") is this
 * call's own; both grow when a call brings more layers, so a steady-state call allocates nothing.  Both exchanges are ordered on the
 * compute stream, so the second cannot reach the receive buffer before the kernel that reads the first has finished.  No library state
 * is read or written except the tables of tse_vector_setup.  stream orders as in tse_dss_view.  Timer group "fieldhv" (one count per
 * launch); pack and exchange count under comm_pack_q / comm_exchange_q / comm_wait. */
#define TSE_HYPERVIS_MAX_FIELDS 64
int tse_hypervis_view(tse_ctx *ctx, int nf, int nk, const double *coef, double nu_ratio, const tse_view *s, const tse_view *v,
                      const tse_view *s_out, const tse_view *v_out, void *stream);
/* the paths and footprints of s ([0]), v ([1]), s_out ([2]) and v_out ([3]) -- path -1 and an empty footprint for an absent view -- and
 * every refusal that needs no device; the overlap rule is applied when any ptr is not null.  Host only: no context, no device. */
int tse_hypervis_view_plan(int nelemd, int nf, int nk, const tse_view *s, const tse_view *v, const tse_view *s_out, const tse_view *v_out,
                           int path[4], long long lo[4], long long hi[4]);

/* ---- first-order sphere operators of a GPU-resident host's OWN fields, element-local or continuous (C0): gradient_sphere,
 * divergence_sphere and vorticity_sphere of derivative_mod.F90 on nk levels of one view, 1 <= nk <= nlev + 1, and with TSE_OP_C0 the
 * make_C0 / make_C0_vector of viscosity_mod.F90:445-535 behind them -- compute_zeta_C0, compute_div_C0 (:542-745), the continuous
 * vorticity and divergence of a dycore's history and physics ----
 *   TSE_OP_LOCAL  out = op(in) on every element by itself: no exchange, not collective
 *   TSE_OP_C0     out = rspheremp * (((w + c0) + c1) + c2), w = spheremp * op(in) rounded once: the bits of TSE_OP_LOCAL followed by
 *                 tse_dss_view(TSE_DSS_AVERAGE, nf_out) on the output array.  COLLECTIVE on a context with neighbour ranks, as tse_dss_view.
 * Views: `in` and `out` are views of tse_dss_view with nf_in, nf_out = 1, 2 (gradient) or 2, 1 (divergence, vorticity); the q axis of the
 * two-field side is the component (lat/lon, as "vn0"; state%v(np,np,2,nlev,tl) is {elem_stride, 16, 32, 4, 1}), and the q stride of the
 * one-field side is free (0 will do).  Each view takes its own path.  The shapes differ, so there is no in-place form: the two footprints
 * must be disjoint (touching is disjoint).  Only addresses of `out` are written.
 * The routines are compiled without implicit contraction (divergence spells out the operations of tse_divergence_sphere and has its bits), so a point's
 * result is one fixed sequence of roundings whatever the paths, the other levels of the call and the number of ranks.  Gradient follows the
 * reference's operations (rrearth * d/dx, rrearth * d/dy, then Dinv^T); vorticity reads the tables rrearth * D of tse_vector_setup.
 * Refused: everything tse_biharmonic_view refuses, an op outside 0..2, a c0 outside 0|1, TSE_OP_VORTICITY before tse_vector_setup (it needs
 * elem%D; gradient and divergence need no set-up).  On failure: nonzero, tse_last_error(), nothing enqueued.
 * Not part of this entry: the _contra variants (contravariant input), ugradv_sphere, curl_sphere and the weak forms (*_wk).
 * No library state is read but the geometry and the tables of tse_vector_setup, none is written; the staging and halo buffers are
 * tse_dss_view's ("view_stage", nf_out * nk layers).  stream orders as in tse_dss_view.  Timer group "fieldop", two launches per call
 * (the stage kernel; then tse_dss_view's sum kernel for C0, tse_biharmonic_view's copy kernel for LOCAL). */
#define TSE_OP_GRADIENT   0   /* in: 1 scalar field  -> out: 2 components   gradient_sphere   (derivative_mod.F90:1660-1700) */
#define TSE_OP_DIVERGENCE 1   /* in: 2 components    -> out: 1 scalar field divergence_sphere (:2364-2414) */
#define TSE_OP_VORTICITY  2   /* in: 2 components    -> out: 1 scalar field vorticity_sphere  (:2250-2301) */
#define TSE_OP_LOCAL 0        /* out = op(in): element-local, no exchange, not collective */
#define TSE_OP_C0    1        /* out = rspheremp * DSS(spheremp * op(in)): make_C0 / make_C0_vector, collective like tse_dss_view */
int tse_sphere_op_view(tse_ctx *ctx, int nk, int op, int c0, const tse_view *in, const tse_view *out, void *stream);
/* the paths and footprints of in ([0]) and out ([1]) and every refusal that needs no device, the overlap rule included when either
 * pointer is non-null */
int tse_sphere_op_view_plan(int nelemd, int nk, int op, const tse_view *in, const tse_view *out,
                            int path[2], long long lo[2], long long hi[2]);

/* ---- min, max, sums and integrals of a GPU-resident host's fields from element partials: what prim_printstate prints at every statefreq
 * (prim_state_mod.F90:186-348: MIN, MAX and SUM of u, v, T, ps, dp3d, omega and the forcings, and the mass M = global_integral(ps_v)) and
 * what global_integral, global_maximum, l1_snorm, l2_snorm and linf_snorm of global_norms_mod.F90 are made of, without the field crossing
 * to the host.  The device forms every ELEMENT's share in one fixed order that depends on the element's own data alone; the host adds the
 * shares exactly (math.fsum, repro_sum) and gets the same digits on any number of ranks (diagnostics.stats_from_partials).
 * field: nf fields of nk levels, 1 <= nk <= nlev + 1, under the view rules of tse_dss_view.  ref (may be NULL): a view of the same nf and
 * nk, the "true solution" ht of the *_snorm functions.  weight (may be NULL): a view of ONE field of nk levels, such as dp3d; its q stride
 * is not looked at and every field uses the same weight.  Each view takes its own path (tse_stats_view_plan).
 * out (HOST memory): [nelemd][nf][TSE_STATS] for per_level = 0, [nelemd][nf][nk][TSE_STATS] for per_level = 1.  For one (element, field,
 * level) slab, h the field, ht the reference, d = h - ht, m = spheremp[e][p] without a weight and spheremp[e][p] * w with one (one
 * product per point and level; spheremp is the context's own), every term one rounded operation per arithmetic sign, nothing contracted:
 *    0 min h            1 max h              2 sum h (unweighted whatever `weight` is: prim_printstate's SUM)
 *    3 sum m*h (global_integral's J_tmp: the host divides by 4 pi)     4 sum m*fabs(h)      5 sum m*(h*h)      6 max fabs(h)
 *    7 the number of values of h that are NaN or +-inf, an exact double
 *    8 sum m*fabs(d)    9 sum m*fabs(ht)    10 sum m*(d*d)    11 sum m*(ht*ht)    12 max fabs(d)    13 max fabs(ht)    (0 without ref)
 *   14 sum m (the area, or the mass when weight = dp)                 15 0
 * A NaN is skipped by the extrema (fmin / fmax): a slab of NaNs gives +inf, -inf for entries 0, 1 and 0 for 6, 12, 13; it does enter the
 * sums.  Where an extremum is zero and zeros of both signs occur, its sign is not specified.
 * THE ORDER OF ADDITION (csrc/tse_view_kernels.h: k_stats_view; tests/stats_model.py adds in the same one):
 *   level share L(k): the 16 terms of the slab, points in memory order p = 4j + i, as the pairwise tree
 *     (((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7))) + (((t8 + t9) + (t10 + t11)) + ((t12 + t13) + (t14 + t15)));
 *   element share (per_level = 0): S = L(0); S = S + L(1); ... ascending in k.  Extrema take the same route.
 * So every number is a function of that element's own values and of spheremp[e] and of nothing else -- not of the path of a view, of the
 * block index, of the other elements or of how elements are dealt to ranks -- and the per_level = 0 output is the ascending sum of the
 * per_level = 1 output, bit for bit.
 * Nothing on the device is written except the call's own partials buffer ("stats_partials": allocated by the first call, grown when a
 * call needs more, freed by tse_finalize).  No library state is read or written.  The views are read-only, so they may overlap each other,
 * and unlike the in-place entries a view may lie inside an allocation of the library (tse_device_ptr: "ps_v", "dp3d", "qdp1", ...): the
 * library's own fields can be looked at the same way.
 * Refused, with nonzero, tse_last_error() and nothing enqueued: a null field or out, nf < 1, nk outside 1..nlev+1, per_level outside 0|1,
 * and everything else tse_dss_view refuses of a view (a zero stride on an extent above 1, a view that may overlap itself, memory that is
 * not device memory of the context's device, a footprint that leaves its allocation, a stream that is being captured or belongs to another
 * device), and a view inside the partials buffer itself.
 * stream: not null: waited for, as in tse_view_put.  The call is complete on return whatever stream is: it returns host data, as
 * tse_apply_forcing does with a budget.  Not collective, no exchange.  Timer group "fieldstats", one launch per call. */
#define TSE_STATS 16
int tse_stats_view(tse_ctx *ctx, int nf, int nk, int per_level,
                   const tse_view *field, const tse_view *ref /* may be NULL */, const tse_view *weight /* may be NULL */,
                   void *stream, double *out /* HOST */);
/* the paths and footprints of field ([0]), ref ([1]) and weight ([2]) and every refusal that needs no device; an absent view gives path -1
 * and lo = hi = 0.  No context, no device. */
int tse_stats_view_plan(int nelemd, int nf, int nk, const tse_view *field, const tse_view *ref, const tse_view *weight,
                        int path[3], long long lo[3], long long hi[3]);

/* ---- the three vertical scans of the primitive equations on a GPU-resident host's columns: pressure from dp3d, the hydrostatic
 * geopotential (preq_hydrostatic, src/asp_tests.F90:1708-1757) and omega / p (E3SM's preq_omega_ps), without dp3d or T crossing to the
 * host.  Levels count from 0 at the model top, n = tse_nlev().  One op per call:
 *   op              dp           p                    a                 b                                        out
 *   TSE_COL_PINT    n levels     NULL                 NULL              NULL                                     n + 1 levels
 *   TSE_COL_PMID    n levels     NULL                 NULL              NULL                                     n levels
 *   TSE_COL_PHI     n levels     n levels or NULL     T_v, n levels     phis, ONE level (level stride not read)  n levels
 *   TSE_COL_OMEGA   iff p NULL   n levels or NULL     vgrad_p, n        divdp, n levels                          n levels
 * A view where the table says NULL is refused, and so is a NULL where it says a view; TSE_COL_OMEGA takes dp exactly when p is NULL.
 * The q axis has extent 1 in every view: its stride is not read.  ptop = hyai(1) * ps0 is read by every op that forms a pressure (all but
 * PHI and OMEGA with p given), rgas by PHI alone.  No library state is read or written: not the cached bounds, not the freshness of
 * q / lnps, not the prescribed-wind state.
 * THE ARITHMETIC: one rounded fp64 operation per arithmetic sign, left to right, nothing contracted; every / a true division; *0.5 and 2*
 * are exact (csrc/tse_view_kernels.h: k_column_view; tests/column_model.py follows the same lines).
 *   PINT   pi[0] = ptop;  pi[k+1] = pi[k] + dp[k]
 *   PMID   p[0] = ptop + dp[0]*0.5;  p[k] = (p[k-1] + dp[k-1]*0.5) + dp[k]*0.5        (E3SM: p(k) = p(k-1) + dp(k-1)/2 + dp(k)/2)
 *   PHI    hkk = (dp[k]*0.5)/p[k], hkl = 2*hkk, t = rgas*T_v[k]:
 *          phii[n-1] = t*hkl,  phi[n-1] = phis + t*hkk;   k = n-2 .. 1: phii[k] = phii[k+1] + t*hkl,  phi[k] = (phis + phii[k+1]) + t*hkk;
 *          phi[0] = (phis + phii[1]) + t*hkk  (no phii[0] is formed)
 *   OMEGA  ckk = 0.5/p[k], ckl = 2*ckk, term = divdp[k]:
 *          om[0] = vgrad_p[0]/p[0] - ckk*term,  s = term;   0 < k < n: om[k] = (vgrad_p[k]/p[k] - ckl*s) - ckk*term,  then s = s + term
 * With p NULL, PHI and OMEGA use PMID's p, formed inside the kernel with PMID's roundings: PHI(p = NULL) has the bits of PMID followed by
 * PHI(p = that output), and the pressure need never exist in memory.  With p given the host's own pressure is used (an Eulerian
 * coordinate's p = hyam*ps0 + hybm*ps is no prefix sum).  Inputs are finite and pressures positive: a NaN propagates, nothing is checked
 * on the device.
 * VIEWS: every view takes its own path of tse_dss_view_plan with nf = 1 and nk = n, 1 (phis) or n + 1 (PINT's out; level-fastest it takes
 * the generic path, as in tse_dss_view for nk != nlev).  An input may carry stride 0 on an axis of extent 1 only (so phis's level stride
 * may be 0); out follows the rules of a get view (no zero stride on an extent above 1, no two index tuples on one address).  Only
 * addresses of out are written, and out's footprint must not meet that of any input (refused by the plan when any pointer is given, and
 * by the entry from the real addresses).  Inputs may lie in the library's own fields (tse_device_ptr: "dp3d", "ps_v", "omega_p", "divdp",
 * ...), as in tse_stats_view; out may not lie in any allocation of the library.
 * Refused, with nonzero, tse_last_error() and nothing enqueued: an op outside 0..3, a view against the table, a ptop that is not finite
 * or is negative, an rgas that is not finite, and everything tse_view_put refuses of a view or a stream (memory that is not device memory
 * of the context's device, a footprint that leaves its allocation, a stream that is being captured or belongs to another device).
 * stream orders as in tse_view_put.  Not collective, no exchange.  Timer group "fieldcol", one launch per call. */
#define TSE_COL_PINT  0   /* dp -> interface pressure, nlev + 1 levels */
#define TSE_COL_PMID  1   /* dp -> mid-point pressure, nlev levels */
#define TSE_COL_PHI   2   /* T_v, dp, phis [, p] -> geopotential at mid-points */
#define TSE_COL_OMEGA 3   /* vgrad_p, divdp, dp | p -> omega / p at mid-points */
int tse_column_view(tse_ctx *ctx, int op, double ptop, double rgas,
                    const tse_view *dp, const tse_view *p, const tse_view *a, const tse_view *b,
                    const tse_view *out, void *stream);
/* the paths and footprints of dp ([0]), p ([1]), a ([2]), b ([3]) and out ([4]) and every refusal that needs no device, the overlap rule
 * included when any pointer is non-null; an absent view gives path -1 and lo = hi = 0.  No context, no device. */
int tse_column_view_plan(int nelemd, int op, const tse_view *dp, const tse_view *p, const tse_view *a,
                         const tse_view *b, const tse_view *out, int path[5], long long lo[5], long long hi[5]);

/* ---- the DCMIP error norms from element partials (test/dcmip1-1/dcmip1-1_error_norm_ng.ncl:39-77: the line L1 L2 Linf q_max q_min) ----
 * The norm line is four sums and four extrema over the unique GLL columns and the levels.  The device forms every ELEMENT's share over the
 * points that element owns, in one fixed order (csrc/tse_kernels.h: k_norm_partials) that depends on the element's own data alone; the host
 * adds the shares exactly (math.fsum, repro_sum) and gets the same bits on any number of ranks.  No tracer field crosses to the host.
 * tse_norm_setup:
 *   owner[nelemd][16]: 1 where this element's point is the owner of its GLL column (dof_mod.F90:43-57), else 0;
 *   colw[nelemd][16]: horizontal weight of the column (the NCL script's R cos(lat) dlon * R dlat), read only where owner = 1;
 *   dh[nlev]: layer depths of the script's "2*(h-base)" recursion.  Copied to the device; may be called again. */
int tse_norm_setup(tse_ctx *ctx, const int *owner, const double *colw, const double *dh);
/* snapshot Q0 = Qdp(nt)[tracer q]/dp as the reference field (one tracer-slot field, allocated by the first call; stays valid through
 * every later state change; a second call overwrites it) and return sum0[nelemd] = sum over owned points and levels of Q0 (unweighted).
 * q counts from 0.  Q is formed as tse_state_q forms it (dp from the current ps_v, a true division): bit for bit the host's Qdp/dp. */
int tse_norm_reference(tse_ctx *ctx, int nt, int q, double *sum0);
/* out[nelemd][8] for Qf = Qdp(nt)[q]/dp(current ps_v), dq = Qf - Q0, dev = |Q0 - avg|, dV = colw*dh(k), owned points only:
 *   0 sum |dq| dV   1 sum dev dV   2 sum dq*dq dV   3 sum dev*dev dV   4 max |dq| dV   5 max dev dV   6 max Qf   7 min Qf
 * Every term is the host expression's in every bit (no contraction); only the order of addition is the device's.  An element without an
 * owned point gives 0 for entries 0 to 5 and -inf / +inf for entries 6 and 7.  All three calls return nonzero (and launch nothing) when
 * tse_norm_setup has not been called, tse_norm_partials also before the first tse_norm_reference, for q outside 0..qsize-1 and nt outside 1|2. */
int tse_norm_partials(tse_ctx *ctx, int nt, int q, double avg, double *out);

/* ---- the numerical-mixing and filament diagnostics from element partials (Lauritzen and Thuburn 2012, QJRMS 138: l_r, l_u, l_o, l_f) ----
 * Two tracers chi = Q[qa], xi = Q[qb] (Q = Qdp(nt)/dp(current ps_v), formed as tse_state_q forms it) that started on the curve
 * xi = psi(chi) = c0 + c2*(chi*chi), c2 < 0, with chi in [xmin, xmax] (DCMIP 1-1: qa = 0, qb = 1, c0 = 0.9, c2 = -0.8).  Every owned
 * (point, level) is put into class A (real mixing: xmin <= chi <= xmax and chord(chi) <= xi <= psi(chi), the chord joining the curve's two
 * ends), B (range-preserving unmixing: not A, chi in [xmin, xmax] and xi in [psi(xmax), psi(xmin)]) or C (overshooting: the rest), and
 * d = its distance to the curve over chi in [xmin, xmax], normalised by the ranges xmax - xmin and psi(xmin) - psi(xmax) (csrc/tse_kernels.h:
 * mix_distance -- + - * / sqrt, comparisons and selects only, no contraction, fixed trip counts).  Weights and owner mask are those of
 * tse_norm_setup, dV = colw*dh(k).  out[nelemd][32], owned points only, sums in the order of k_norm_partials:
 *   0 sum_A d dV   1 sum_B d dV   2 sum_C d dV   3 sum dV   4 5 6 the number of (point, level) in A, B, C (exact)   7 max d
 *   8+j sum dV [chi >= tau[j]], j < ntau   the remaining entries 0
 * An element without an owned point gives 0 everywhere.  The host adds entries 0 to 3 and 8.. exactly over elements and ranks:
 * l_r, l_u, l_o = S0, S1, S2 / S3;  l_f(tau_j) = 100 * S(8+j)(t) / S(8+j)(t0).  All inputs finite.  Returns nonzero with a message (and
 * launches nothing) before tse_norm_setup, for nt outside 1|2, qa or qb outside 0..qsize-1, xmax <= xmin, c2 >= 0, ntau outside 0..24 and
 * a null out (or a null tau with ntau > 0). */
int tse_mix_partials(tse_ctx *ctx, int nt, int qa, int qb, double xmin, double xmax, double c0, double c2, const double *tau, int ntau, double *out);

/* ---- introspection for tests and the benchmark harness ---- */
/* device pointers of internal fields: "qdp1", "qdp2" [nelemd][qsize][nlev][16] (the two time levels are two allocations), "vn0", "dp", "divdp", "divdp_proj",
 * "eta_dot_dpdn", "omega_p", "dp3d", "ps_v", "qmin", "qmax", "sendbuf", "recvbuf", "q" [nelemd][qsize][nlev][16] and "lnps" [nelemd][16]
 * (both null before the first tse_state_q; "q" is also the staging field of tse_apply_forcing_host, which allocates it), "qref" [nelemd][nlev][16] (null before the first tse_norm_reference),
 * "remap_status" [nelemd][4] ints (null before the first tse_remap_view), "view_stage" [nelemd][layers][16] the staging field tse_dss_view,
 * tse_biharmonic_view, tse_vlaplace_view and tse_sphere_op_view share (null before the first call of any; it moves only when a call brings more layers than any before),
 * "hypervis_stage" the second staging field of tse_hypervis_view (null before its first call; the same shape and growth rule),
 * "stats_partials" the partials buffer of tse_stats_view (null before its first call; it moves only when a call needs more than any before) */
void *tse_device_ptr(tse_ctx *ctx, const char *name, size_t *nbytes);
/* accumulated HIP-event time (ms) and launch count of a named kernel group since the last reset; names:
 * "advance" (= "advance0" + "advance1" + "advance2", the three RK stages), "dss", "lap", "minmax", "remap", "level", "dcmip", "avg", "stateq", "norms"
 * (tse_norm_reference and tse_norm_partials), "mixing" (tse_mix_partials), "view" (tse_view_put and tse_view_get), "forcing" (tse_apply_forcing and tse_apply_forcing_host), "fieldremap" (tse_remap_view: its check kernel and its remap kernel), "fielddss" (tse_dss_view: its stage and its sum kernel), "fieldlap" (tse_biharmonic_view: its stage and its out kernel), "fieldvlap" (tse_vlaplace_view: its stage and its out kernel), "fieldhv" (tse_hypervis_view: one count per launch, at most five), "fieldop" (tse_sphere_op_view: its stage kernel and the sum or copy kernel behind it), "fieldstats" (tse_stats_view: its one kernel), "fieldcol" (tse_column_view: its one kernel), and the comm_* groups of tse_comm_timing.  A name matches every group it is a prefix of. */
int tse_kernel_time(tse_ctx *ctx, const char *name, double *ms, long *launches);
int tse_timing(tse_ctx *ctx, int enable); /* enable/disable + reset per-kernel event timing (not the comm_* groups) */
/* enable/disable + reset the timers of the halo exchange, read through tse_kernel_time like the kernel groups (and reset by this call
 * alone; tse_timing neither turns them on nor clears them):
 *   "comm_pack_q", "comm_pack_mm"          pack launches of the tracer halo (kind 0) / of the element bounds (kind 1), on the stream
 *                                          they run on
 *   "comm_exchange_q", "comm_exchange_mm"  the whole exchange of that kind: ncclGroupStart .. ncclGroupEnd, or the callback (with the
 *                                          host's wait for the packs before it)
 *   "comm_unpack_q", "comm_unpack_mm"      unpack launches
 *   "comm_wait"                            the exposed wait: the time the compute stream could not go on because communication was not
 *                                          done.  Where the exchange runs on the communication stream (the whole-step call and
 *                                          tse_prim_run_subcycle on several ranks), one event pair on the compute stream brackets each
 *                                          of its waits for that stream (after every split stage; at the first stage's bounds).  Where
 *                                          the exchange runs on the compute stream itself (tse_euler_step, and the whole-step call with
 *                                          TSE_DSS_ON_READ=0), all of it is exposed: the pair brackets the pack -> exchange -> unpack
 *                                          sequence, so its time is their sum (with the launch gaps between them).
 * "comm" gives the total of all seven, "comm_exchange" both kinds.  Off by default; while off no event is created or recorded and the
 * launches and stream dependencies are those of a context without it.  A context without neighbour ranks records nothing: 0 ms and 0
 * launches for every comm_* name.  The events resolve when they are read (the read waits for the compute and communication streams). */
int tse_comm_timing(tse_ctx *ctx, int enable);
/* where the five tracer-sized fields were placed (device memory is not uniform for writes and the rate is a property of the
 * allocation: tse_init tries field-sized chunks -- up to TSE_PLACEMENT, default 20, in all, up to 8 held at a time, the slowest given
 * back and the next one allocated behind a small pad -- until three of them take a streaming write at TSE_PLACEMENT_GOOD, default
 * 6000 GB/s, and keeps the five fastest): number of chunks tried (0: no choice was made), their write rates in
 * GB/s in the order tried, and which try became T, Qdp(1), Qdp(2), B, C */
int tse_placement(tse_ctx *ctx, int *ntried, double *write_gbs /* [32] */, int *chosen /* [5] */);
int tse_halo_layout(tse_ctx *ctx, int *ncol_send, int *ncol_recv);
/* per-slot entry counts of the kind-1 (min/max) exchange, in send-slot / recv-slot order */
int tse_halo_minmax_layout(tse_ctx *ctx, int *send_len, int *recv_len);

#ifdef __cplusplus
}
#endif
#endif
