! cuda_mod_hip.F90 -- the Fortran half of the drop-in boundary.
!
! Provides a module named `cuda_mod` with the public names the reference's accelerator seam expects
! (reference src/share/cuda_mod.F90:57-64), implemented over the C ABI of include/transport_se_hip.h with
! ISO_C_BINDING.  Compiling the reference's prim_advection_mod.F90 with -DUSE_CUDA_FORTRAN=1 against THIS module
! makes its own hooks
!     euler_step      -> call euler_step_cuda(np1_qdp,n0_qdp,dt,elem,hvcoord,hybrid,deriv,nets,nete,DSSopt,rhs_multiplier)
!                                                                      (prim_advection_mod.F90:715-718)
!     qdp_time_avg    -> call qdp_time_avg_cuda(elem,rkstage,n0_qdp,np1_qdp,limiter_option,0d0,nets,nete)   (:653-656)
!     vertical_remap  -> call vertical_remap_cuda(elem,hvcoord,dt,np1,np1_qdp,nets,nete)                    (:1279-1282)
! land in the HIP library; the driver calls cuda_mod_init / copy_qdp_h2d / copy_qdp_d2h exactly where
! prim_driver_mod.F90:686-689,726-728,781-784,798-801 does.  Host code stays Fortran; elem(:) stays the host copy.
! One MPI rank drives one GPU.  Threading as in the CUDA seam (cuda_mod.F90:6-8,211-212,408-409,549-550,587-594): the entries are
! called by ALL horizontal OpenMP threads of the rank (the time loop runs inside !$OMP PARALLEL, prim_main.F90:143-162), each with
! its own nets:nete; every entry is  !$OMP BARRIER / !$OMP MASTER ... !$OMP END MASTER / !$OMP BARRIER  and the master thread acts for
! elements 1:nelemd (elem(:) is the rank's whole shared array).  Outside a parallel region, or built without -fopenmp, the
! directives are no-ops.
module cuda_mod
  use iso_c_binding
  use kinds,          only : real_kind
  use dimensions_mod, only : np, nlev, nlevp, nelemd, qsize, qsize_d
  use element_mod,    only : element_t
  use derivative_mod, only : derivative_t
  use hybvcoord_mod,  only : hvcoord_t
  use hybrid_mod,     only : hybrid_t
  use parallel_mod,   only : abortmp
  use control_mod,    only : nu_q, limiter_option, rsplit, qsplit, vert_remap_q_alg, hypervis_subcycle_q, hypervis_power, &
                             hypervis_scaling
  use schedtype_mod,  only : schedule
  use time_mod,       only : TimeLevel_t, TimeLevel_update, TimeLevel_Qdp
  implicit none
  private
#include <mpif.h>
  public :: cuda_mod_init, euler_step_cuda, qdp_time_avg_cuda, vertical_remap_cuda, copy_qdp_d2h, copy_qdp_h2d
  ! not in the reference's list: the whole tracer step in one device call (the fast path, INTEGRATION.md section 2)
  public :: advec_tracers_remap_rk2_hip
  ! wall time spent inside the seam (everything between entering a cuda_mod routine and returning to the host code), by entry
  public :: hip_seam_report
  real(kind=8), save :: t_seam(5) = 0d0   ! 1 copy_qdp_h2d, 2 copy_qdp_d2h, 3 euler_step_cuda/qdp_time_avg_cuda, 4 whole-step call, 5 vertical_remap_cuda
  ! not in the reference's list either: the device-resident prim_run loop (INTEGRATION.md section 2b) -- prescribed DCMIP fields on the
  ! device, nsub whole prim_run_subcycle calls in one device call, and the download of what prim_run_subcycle leaves in elem
  public :: dcmip_init_hip, prim_run_subcycle_hip, copy_state_d2h_hip, hip_resident_report
  ! the DCMIP error norms from element partials (INTEGRATION.md section 2c): the device forms every element's share of the norm line's
  ! sums and extrema, the host reduces them over elements and ranks (repro_sum for the sums)
  public :: norm_setup_hip, norm_reference_hip, norm_partials_hip
  ! the numerical-mixing and filament diagnostics of two correlated tracers from element partials (INTEGRATION.md section 2d)
  public :: mix_partials_hip
  ! state exchange with a GPU-resident host (INTEGRATION.md section 2e): fields move between the host's own DEVICE arrays and the library
  ! on the device, through strided views; nothing crosses the host link
  public :: tse_view, view_put_hip, view_get_hip
  ! tracer forcing, the physics step between two prim_run_subcycle_hip calls (INTEGRATION.md section 2f): Qdp(nt) = Qdp(nt) + dt*FQ, never
  ! below zero, from a device array (apply_forcing_hip) or from elem(:)%derived%FQ in host memory (apply_forcing_elem_hip)
  public :: apply_forcing_hip, apply_forcing_elem_hip
  integer, parameter, public :: forcing_tendency = 0, forcing_adjust = 1   ! TSE_FORCING_TENDENCY, TSE_FORCING_ADJUST
  ! vertical remap of the host's own level fields on its own grids (INTEGRATION.md section 2g): remap_Q_ppm in place in a device array
  public :: remap_view_hip, remap_view_status_hip
  integer, parameter, public :: remap_mass = 0, remap_mean = 1   ! TSE_REMAP_MASS, TSE_REMAP_MEAN
  ! DSS of the host's own device-resident fields (tse_dss_view)
  public :: dss_view_hip
  integer, parameter, public :: dss_average = 0, dss_weak = 1   ! TSE_DSS_AVERAGE, TSE_DSS_WEAK
  ! weak Laplacian / biharmonic of the host's own device-resident scalar fields (tse_biharmonic_view)
  public :: biharmonic_view_hip
  integer, parameter, public :: lap_order1 = 1, lap_order2 = 2   ! TSE_LAPLACE, TSE_BIHARMONIC
  ! weak vector Laplacian / biharmonic of the host's own device-resident wind (tse_vector_setup, tse_vlaplace_view)
  public :: vector_setup_hip, vlaplace_view_hip
  ! one hyperviscosity sub-step of the host's own device-resident scalars and wind in one call (tse_hypervis_view)
  public :: hypervis_view_hip
  integer, parameter, public :: vlap_order1 = 1, vlap_order2 = 2   ! TSE_VLAPLACE, TSE_VBIHARMONIC
  ! gradient, divergence and vorticity of the host's own device-resident fields, element-local or C0 (tse_sphere_op_view)
  public :: sphere_op_view_hip
  integer, parameter, public :: op_gradient = 0, op_divergence = 1, op_vorticity = 2   ! TSE_OP_GRADIENT, TSE_OP_DIVERGENCE, TSE_OP_VORTICITY
  integer, parameter, public :: op_local = 0, op_c0 = 1                                ! TSE_OP_LOCAL, TSE_OP_C0
  ! min, max, sums and integrals of the host's own device-resident fields from element partials (tse_stats_view)
  public :: stats_view_hip
  integer, parameter, public :: tse_stats = 16   ! TSE_STATS
  ! pressure, geopotential and omega / p of the host's own device-resident columns (tse_column_view)
  public :: column_view_hip
  integer, parameter, public :: col_pint = 0, col_pmid = 1, col_phi = 2, col_omega = 3   ! TSE_COL_PINT, TSE_COL_PMID, TSE_COL_PHI, TSE_COL_OMEGA
  logical, save :: remap_refused = .false.            ! remap_view_hip / remap_view_status_hip: the master thread's answer, read by every thread
  integer(c_int), save :: remap_nrefused = 0, remap_where(4) = 0
  real(kind=8), save :: t_res(3) = 0d0    ! 1 dcmip_init_hip, 2 prim_run_subcycle_hip, 3 copy_state_d2h_hip
  integer(c_int), save :: res_nstep = 0   ! the library's step count after the last prim_run_subcycle_hip
  integer(kind=8), save :: t_c0

  ! mirror of tse_init_args (include/transport_se_hip.h)
  type, bind(C) :: tse_init_args
     integer(c_int) :: nelemd, qsize, device
     real(c_double) :: nu_q
     integer(c_int) :: limiter_option, rsplit
     type(c_ptr)    :: Dvv, hyai, hybi
     real(c_double) :: ps0
     type(c_ptr)    :: Dinv;      integer(c_size_t) :: Dinv_stride
     type(c_ptr)    :: metdet;    integer(c_size_t) :: metdet_stride
     type(c_ptr)    :: rmetdet;   integer(c_size_t) :: rmetdet_stride
     type(c_ptr)    :: spheremp;  integer(c_size_t) :: spheremp_stride
     type(c_ptr)    :: rspheremp; integer(c_size_t) :: rspheremp_stride
     type(c_ptr)    :: putmapP, getmapP, reverse
     integer(c_int) :: nsend;  type(c_ptr) :: send_peer, send_ptrP, send_lengthP
     integer(c_int) :: nrecv;  type(c_ptr) :: recv_peer, recv_ptrP, recv_lengthP
     type(c_funptr) :: exchange; type(c_ptr) :: exchange_user
     integer(c_int) :: vert_remap_q_alg
  end type tse_init_args

  ! mirror of tse_view (include/transport_se_hip.h): the DEVICE address of the entry (element 1, q 1, level 1, j 1, i 1) and the strides, in
  ! doubles, of the axes element, q (tracer; wind component for 'vn0'), level, j, i; 0 for an axis the field does not have
  type, bind(C) :: tse_view
     type(c_ptr)          :: ptr
     integer(c_long_long) :: stride(5)
  end type tse_view

  interface
     integer(c_int) function tse_init(ctx, args) bind(C, name='tse_init')
       import; type(c_ptr), intent(out) :: ctx; type(tse_init_args), intent(in) :: args
     end function
     integer(c_int) function tse_host_register(ctx, base, bytes) bind(C, name='tse_host_register')
       import; type(c_ptr), value :: ctx, base; integer(c_size_t), value :: bytes
     end function
     integer(c_int) function tse_comm_unique_id(id) bind(C, name='tse_comm_unique_id')
       import; type(c_ptr), value :: id
     end function
     integer(c_int) function tse_comm_abort(ctx) bind(C, name='tse_comm_abort')
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function tse_comm_init(ctx, id, rank, nranks) bind(C, name='tse_comm_init')
       import; type(c_ptr), value :: ctx, id; integer(c_int), value :: rank, nranks
     end function
     integer(c_int) function tse_comm_precheck(ctx, rank, nranks) bind(C, name='tse_comm_precheck')
       import; type(c_ptr), value :: ctx; integer(c_int), value :: rank, nranks
     end function
     integer(c_int) function tse_copy_qdp_h2d(ctx, q, stride, qsize_d, nt) bind(C, name='tse_copy_qdp_h2d')
       import; type(c_ptr), value :: ctx, q; integer(c_size_t), value :: stride; integer(c_int), value :: qsize_d, nt
     end function
     integer(c_int) function tse_copy_qdp_d2h(ctx, q, stride, qsize_d, nt) bind(C, name='tse_copy_qdp_d2h')
       import; type(c_ptr), value :: ctx, q; integer(c_size_t), value :: stride; integer(c_int), value :: qsize_d, nt
     end function
     integer(c_int) function tse_set_derived(ctx, vn0, s0, dp, s1, eta, s2, omega, s3) bind(C, name='tse_set_derived')
       import; type(c_ptr), value :: ctx, vn0, dp, eta, omega; integer(c_size_t), value :: s0, s1, s2, s3
     end function
     integer(c_int) function tse_set_divdp(ctx, divdp, s0, divdp_proj, s1) bind(C, name='tse_set_divdp')
       import; type(c_ptr), value :: ctx, divdp, divdp_proj; integer(c_size_t), value :: s0, s1
     end function
     integer(c_int) function tse_get_derived(ctx, a, s1, b, s2, c, s3, d, s4, e, s5, f, s6) bind(C, name='tse_get_derived')
       import; type(c_ptr), value :: ctx, a, b, c, d, e, f; integer(c_size_t), value :: s1, s2, s3, s4, s5, s6
     end function
     integer(c_int) function tse_euler_step(ctx, np1_qdp, n0_qdp, dt, DSSopt, rhs) bind(C, name='tse_euler_step')
       import; type(c_ptr), value :: ctx; integer(c_int), value :: np1_qdp, n0_qdp, DSSopt, rhs; real(c_double), value :: dt
     end function
     integer(c_int) function tse_advec_tracers_remap_rk2(ctx, dt, n0_qdp, np1_qdp) bind(C, name='tse_advec_tracers_remap_rk2')
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt; integer(c_int), value :: n0_qdp, np1_qdp
     end function
     integer(c_int) function tse_qdp_time_avg(ctx, rkstage, n0_qdp, np1_qdp) bind(C, name='tse_qdp_time_avg')
       import; type(c_ptr), value :: ctx; integer(c_int), value :: rkstage, n0_qdp, np1_qdp
     end function
     integer(c_int) function tse_vertical_remap(ctx, dt, np1_qdp) bind(C, name='tse_vertical_remap')
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt; integer(c_int), value :: np1_qdp
     end function
     function tse_last_error() bind(C, name='tse_last_error') result(p)
       import; type(c_ptr) :: p
     end function
     integer(c_int) function tse_nlev() bind(C, name='tse_nlev')
       import
     end function
     integer(c_int) function tse_halo_layout(ctx, ns, nr) bind(C, name='tse_halo_layout')
       import; type(c_ptr), value :: ctx; integer(c_int), intent(out) :: ns, nr
     end function
     integer(c_int) function tse_halo_minmax_layout(ctx, sl, rl) bind(C, name='tse_halo_minmax_layout')
       import; type(c_ptr), value :: ctx, sl, rl
     end function
     integer(c_int) function tse_dcmip_init(ctx, test, lat, lon, hyam, hybm) bind(C, name='tse_dcmip_init')
       import; type(c_ptr), value :: ctx, lat, lon, hyam, hybm; integer(c_int), value :: test
     end function
     integer(c_int) function tse_dcmip_set_initial(ctx) bind(C, name='tse_dcmip_set_initial')
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function tse_prim_run_subcycle(ctx, tstep, nsub, nstep) bind(C, name='tse_prim_run_subcycle')
       import; type(c_ptr), value :: ctx; real(c_double), value :: tstep; integer(c_int), value :: nsub
       integer(c_int), intent(inout) :: nstep
     end function
     integer(c_int) function tse_state_q(ctx, nt) bind(C, name='tse_state_q')
       import; type(c_ptr), value :: ctx; integer(c_int), value :: nt
     end function
     integer(c_int) function tse_copy_q_d2h(ctx, q, stride, qsize_d) bind(C, name='tse_copy_q_d2h')
       import; type(c_ptr), value :: ctx, q; integer(c_size_t), value :: stride; integer(c_int), value :: qsize_d
     end function
     integer(c_int) function tse_copy_lnps_d2h(ctx, lnps, stride) bind(C, name='tse_copy_lnps_d2h')
       import; type(c_ptr), value :: ctx, lnps; integer(c_size_t), value :: stride
     end function
     integer(c_int) function tse_norm_setup(ctx, owner, colw, dh) bind(C, name='tse_norm_setup')
       import; type(c_ptr), value :: ctx, owner, colw, dh
     end function
     integer(c_int) function tse_norm_reference(ctx, nt, q, sum0) bind(C, name='tse_norm_reference')
       import; type(c_ptr), value :: ctx, sum0; integer(c_int), value :: nt, q
     end function
     integer(c_int) function tse_norm_partials(ctx, nt, q, avg, out) bind(C, name='tse_norm_partials')
       import; type(c_ptr), value :: ctx, out; integer(c_int), value :: nt, q; real(c_double), value :: avg
     end function
     integer(c_int) function tse_mix_partials(ctx, nt, qa, qb, xmin, xmax, c0, c2, tau, ntau, out) bind(C, name='tse_mix_partials')
       import; type(c_ptr), value :: ctx, tau, out; integer(c_int), value :: nt, qa, qb, ntau; real(c_double), value :: xmin, xmax, c0, c2
     end function
     integer(c_int) function tse_view_put(ctx, field, nt, v, stream) bind(C, name='tse_view_put')
       import; type(c_ptr), value :: ctx, stream; character(kind=c_char), intent(in) :: field(*); integer(c_int), value :: nt
       type(tse_view), intent(in) :: v
     end function
     integer(c_int) function tse_view_get(ctx, field, nt, v, stream) bind(C, name='tse_view_get')
       import; type(c_ptr), value :: ctx, stream; character(kind=c_char), intent(in) :: field(*); integer(c_int), value :: nt
       type(tse_view), intent(in) :: v
     end function
     integer(c_int) function tse_apply_forcing(ctx, nt, dt, mode, fq, stream, budget) bind(C, name='tse_apply_forcing')
       import; type(c_ptr), value :: ctx, stream, budget; integer(c_int), value :: nt, mode; real(c_double), value :: dt
       type(tse_view), intent(in) :: fq
     end function
     integer(c_int) function tse_apply_forcing_host(ctx, nt, dt, mode, fq_elem1, elem_stride, qsize_d, budget) &
          bind(C, name='tse_apply_forcing_host')
       import; type(c_ptr), value :: ctx, fq_elem1, budget; integer(c_int), value :: nt, mode, qsize_d; real(c_double), value :: dt
       integer(c_size_t), value :: elem_stride
     end function
     integer(c_int) function tse_remap_view(ctx, nf, mode, alg, field, dp_src, dp_tgt, stream) bind(C, name='tse_remap_view')
       import; type(c_ptr), value :: ctx, stream; integer(c_int), value :: nf, mode, alg
       type(tse_view), intent(in) :: field, dp_src, dp_tgt
     end function
     integer(c_int) function tse_remap_view_status(ctx, nrefused, first) bind(C, name='tse_remap_view_status')
       import; type(c_ptr), value :: ctx; integer(c_int), intent(out) :: nrefused, first(4)
     end function
     integer(c_int) function tse_dss_view(ctx, nf, nk, mode, field, stream) bind(C, name='tse_dss_view')
       import; type(c_ptr), value :: ctx, stream; integer(c_int), value :: nf, nk, mode
       type(tse_view), intent(in) :: field
     end function
     integer(c_int) function tse_biharmonic_view(ctx, nf, nk, order, vin, vout, stream) bind(C, name='tse_biharmonic_view')
       import; type(c_ptr), value :: ctx, stream; integer(c_int), value :: nf, nk, order
       type(tse_view), intent(in) :: vin, vout
     end function
     integer(c_int) function tse_vector_setup(ctx, D, D_stride, metinv, metinv_stride, mp, mp_stride) bind(C, name='tse_vector_setup')
       import; type(c_ptr), value :: ctx, D, metinv, mp; integer(c_size_t), value :: D_stride, metinv_stride, mp_stride
     end function
     integer(c_int) function tse_vlaplace_view(ctx, nk, order, nu_ratio, vin, vout, stream) bind(C, name='tse_vlaplace_view')
       import; type(c_ptr), value :: ctx, stream; integer(c_int), value :: nk, order; real(c_double), value :: nu_ratio
       type(tse_view), intent(in) :: vin, vout
     end function
     integer(c_int) function tse_hypervis_view(ctx, nf, nk, coef, nu_ratio, s, v, s_out, v_out, stream) bind(C, name='tse_hypervis_view')
       import; type(c_ptr), value :: ctx, s, v, s_out, v_out, stream; integer(c_int), value :: nf, nk
       real(c_double), intent(in) :: coef(*); real(c_double), value :: nu_ratio
     end function
     integer(c_int) function tse_sphere_op_view(ctx, nk, op, c0, vin, vout, stream) bind(C, name='tse_sphere_op_view')
       import; type(c_ptr), value :: ctx, stream; integer(c_int), value :: nk, op, c0
       type(tse_view), intent(in) :: vin, vout
     end function
     integer(c_int) function tse_stats_view(ctx, nf, nk, per_level, field, ref, weight, stream, out) bind(C, name='tse_stats_view')
       import; type(c_ptr), value :: ctx, ref, weight, stream, out; integer(c_int), value :: nf, nk, per_level
       type(tse_view), intent(in) :: field
     end function
     integer(c_int) function tse_column_view(ctx, op, ptop, rgas, dp, p, a, b, out, stream) bind(C, name='tse_column_view')
       import; type(c_ptr), value :: ctx, dp, p, a, b, stream; integer(c_int), value :: op; real(c_double), value :: ptop, rgas
       type(tse_view), intent(in) :: out
     end function
     ! HIP runtime (libamdhip64): staging copies of the packed slots for a non-GPU-aware MPI
     integer(c_int) function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy')
       import; type(c_ptr), value :: dst, src; integer(c_size_t), value :: nbytes; integer(c_int), value :: kind
     end function
  end interface

  type(c_ptr), save :: ctx = c_null_ptr
  integer(c_int), allocatable, target, save :: putm(:,:), getm(:,:), revm(:,:)
  integer(c_int), allocatable, target, save :: speer(:), sptr(:), slen(:), rpeer(:), rptr(:), rlen(:)
  real(c_double), allocatable, target, save :: dvv_c(:,:), hyai_c(:), hybi_c(:)
  ! multi-rank halo exchange state (the bndry_exchangeV body, bndry_mod.F90:74-124, on staged host copies)
  integer, save :: x_comm = -1, x_nsend = 0, x_nrecv = 0
  integer(c_int), allocatable, target, save :: x_slen(:,:), x_rlen(:,:)     ! (slot, kind+1)
  real(c_double), allocatable, target, save :: x_hsend(:), x_hrecv(:)

contains

  subroutine check(rc, where)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    character(len=400) :: text
    integer :: i
    if (rc == 0) return
    call c_f_pointer(tse_last_error(), msg, [400])
    text = ' '
    do i = 1, 400
       if (msg(i) == c_null_char) exit
       text(i:i) = msg(i)
    enddo
    call seam_abort(where//': '//trim(text))
  end subroutine check

  ! abortmp (parallel_mod.F90:274-287) writes its message to buffered stdout and then calls MPI_Abort, which loses it whenever
  ! stdout is a pipe or a file; the message goes to stderr first (and both units are flushed)
  ! and abortmp hands MPI_Abort an uninitialised error code (often 0: the launcher then reports success), so the job is ended
  ! here with a defined one; abortmp stays behind it as the reference's own route
  subroutine seam_abort(text)
    character(len=*), intent(in) :: text
    integer :: ierr
    write(0,'(a)') ' cuda_mod_hip: ABORTING WITH ERROR: '//text
    flush(0); flush(6)
    call MPI_Abort(MPI_COMM_WORLD, 1, ierr)
    call abortmp(text)
  end subroutine seam_abort

  ! The library is built for one level count (tse_nlev(); include/transport_se_hip.h): a host built with another PLEV must not
  ! drive it -- every level extent it passes would be read with the library's.
  subroutine check_nlev(where)
    character(len=*), intent(in) :: where
    character(len=200) :: text
    if (tse_nlev() == nlev) return
    write(text, '(a,a,i0,a,i0,a)') where, ': the HIP library is built for nlev = ', tse_nlev(), ', this host for nlev = ', nlev, &
         ' (PLEV): link the library built with -DNLEV=<PLEV>'
    call seam_abort(trim(text))
  end subroutine check_nlev

  subroutine tic()
    call system_clock(t_c0)
  end subroutine tic
  subroutine toc(i)
    integer, intent(in) :: i
    integer(kind=8) :: c1, rate
    call system_clock(c1, rate)
    t_seam(i) = t_seam(i) + dble(c1 - t_c0)/dble(rate)
  end subroutine toc
  subroutine hip_seam_report(nsteps)
    integer, intent(in) :: nsteps
    write(*,'(a,i6,a)') ' hip seam: wall seconds inside the cuda_mod entries over ', nsteps, ' tracer steps'
    write(*,'(a,5f10.4)') ' hip seam: copy_qdp_h2d copy_qdp_d2h euler_step+time_avg whole_step vertical_remap =', t_seam
    write(*,'(a,es14.6)') ' hip seam: tracer-DOF-steps/s of the seam alone = ', &
         dble(nelemd)*np*np*nlev*qsize*nsteps/max(sum(t_seam), 1d-30)
  end subroutine hip_seam_report

  integer(c_size_t) function stride_of(a, b)
    type(c_ptr), intent(in) :: a, b
    stride_of = transfer(b, 0_c_size_t) - transfer(a, 0_c_size_t)
  end function stride_of

  ! cuda_mod_init(elem,hybrid,deriv,hvcoord)   (called at the end of prim_init2, prim_driver_mod.F90:686-689)
  subroutine cuda_mod_init(elem, hybrid, deriv, hvcoord)
    type(element_t),    intent(in), target :: elem(:)
    type(hybrid_t),     intent(in) :: hybrid
    type(derivative_t), intent(in) :: deriv
    type(hvcoord_t),    intent(in) :: hvcoord
    type(tse_init_args) :: a
    integer :: ie, j, ns, nr, e2, ierr, rc_comm, rc_any
    integer(c_int) :: ncs, ncr
    character(len=16) :: xmode
    logical :: use_rccl
    character(kind=c_char), target, save :: comm_id(128)
    !$OMP BARRIER
    !$OMP MASTER
    ! What the device path does not implement is refused here, with the reference's own error route, instead of being silently
    ! replaced by the default behaviour: the tracer time levels assume qsplit = 1 (TimeLevel_Qdp, time_mod.F90:85-109), the
    ! hyperviscosity is the single constant-coefficient application of euler_step (prim_advection_mod.F90:796-826; no tracer
    ! subcycling, no variable / tensor coefficient: derivative_mod.F90:2438-2445), the remap is remap_Q_ppm with ghost-cell
    ! variant 0|1 or 2 (prim_advection_mod.F90:230-341).  limiter_option needs no check here: control_mod's value goes into
    ! tse_init_args below, and tse_init takes 8 (optimization-based), 9 (clip-and-sum) and 0 (none) and refuses every other value.
    if (qsplit /= 1) call seam_abort('cuda_mod_init(hip): qsplit must be 1')
    if (hypervis_subcycle_q /= 1) call seam_abort('cuda_mod_init(hip): hypervis_subcycle_q must be 1')
    if (hypervis_power /= 0 .or. hypervis_scaling /= 0) call seam_abort('cuda_mod_init(hip): hypervis_power and hypervis_scaling must be 0')
    if (vert_remap_q_alg < 0 .or. vert_remap_q_alg > 2) call seam_abort('cuda_mod_init(hip): vert_remap_q_alg must be 0, 1 or 2')
    call check_nlev('cuda_mod_init(hip)')
    allocate(putm(8,nelemd), getm(8,nelemd), revm(8,nelemd))
    do ie = 1, nelemd
       putm(:,ie) = elem(ie)%desc%putmapP(1:8)
       getm(:,ie) = elem(ie)%desc%getmapP(1:8)
       do j = 1, 8
          revm(j,ie) = merge(1, 0, elem(ie)%desc%reverse(j))
       enddo
    enddo
    allocate(dvv_c(np,np), hyai_c(nlevp), hybi_c(nlevp))
    dvv_c = deriv%Dvv; hyai_c = hvcoord%hyai; hybi_c = hvcoord%hybi
    ! neighbour-rank slots exactly as genEdgeSched built them (schedule_mod.F90:36-239, schedtype_mod.F90:7-29)
    ns = schedule(1)%nSendCycles; nr = schedule(1)%nRecvCycles
    allocate(speer(max(ns,1)), sptr(max(ns,1)), slen(max(ns,1)), rpeer(max(nr,1)), rptr(max(nr,1)), rlen(max(nr,1)))
    do j = 1, ns
       speer(j) = schedule(1)%SendCycle(j)%dest - 1
       sptr(j)  = schedule(1)%SendCycle(j)%ptrP
       slen(j)  = schedule(1)%SendCycle(j)%lengthP
    enddo
    do j = 1, nr
       rpeer(j) = schedule(1)%RecvCycle(j)%source - 1
       rptr(j)  = schedule(1)%RecvCycle(j)%ptrP
       rlen(j)  = schedule(1)%RecvCycle(j)%lengthP
    enddo
    x_comm = hybrid%par%comm; x_nsend = ns; x_nrecv = nr
    e2 = min(2, nelemd)
    a%nelemd = nelemd; a%qsize = qsize; a%device = -1; a%nu_q = nu_q
    a%limiter_option = limiter_option; a%rsplit = rsplit
    a%Dvv = c_loc(dvv_c); a%hyai = c_loc(hyai_c); a%hybi = c_loc(hybi_c); a%ps0 = hvcoord%ps0
    a%Dinv = c_loc(elem(1)%Dinv);           a%Dinv_stride = stride_of(c_loc(elem(1)%Dinv), c_loc(elem(e2)%Dinv))
    a%metdet = c_loc(elem(1)%metdet);       a%metdet_stride = stride_of(c_loc(elem(1)%metdet), c_loc(elem(e2)%metdet))
    a%rmetdet = c_loc(elem(1)%rmetdet);     a%rmetdet_stride = stride_of(c_loc(elem(1)%rmetdet), c_loc(elem(e2)%rmetdet))
    a%spheremp = c_loc(elem(1)%spheremp);   a%spheremp_stride = stride_of(c_loc(elem(1)%spheremp), c_loc(elem(e2)%spheremp))
    a%rspheremp = c_loc(elem(1)%rspheremp); a%rspheremp_stride = stride_of(c_loc(elem(1)%rspheremp), c_loc(elem(e2)%rspheremp))
    a%putmapP = c_loc(putm); a%getmapP = c_loc(getm); a%reverse = c_loc(revm)
    a%nsend = ns; a%send_peer = c_loc(speer); a%send_ptrP = c_loc(sptr); a%send_lengthP = c_loc(slen)
    a%nrecv = nr; a%recv_peer = c_loc(rpeer); a%recv_ptrP = c_loc(rptr); a%recv_lengthP = c_loc(rlen)
    a%exchange = c_null_funptr; a%exchange_user = c_null_ptr
    a%vert_remap_q_alg = vert_remap_q_alg
    ! bndry_exchangeV: TSE_EXCHANGE=rccl (one rank per GPU) lets the library exchange the halo itself with RCCL send/recv on its
    ! own stream -- the communicator id travels over MPI once, below; otherwise the MPI body of tse_f_exchange is the callback
    call get_environment_variable('TSE_EXCHANGE', xmode)
    use_rccl = (trim(xmode) == 'rccl') .and. hybrid%par%nprocs > 1
    ! (with rccl the MPI body stays registered but dormant: the transport of last resort if the communicator cannot be built)
    if (ns + nr > 0) a%exchange = c_funloc(tse_f_exchange)
    call get_environment_variable('TSE_DEVICE_PER_RANK', xmode)
    if (trim(xmode) == '1') a%device = hybrid%par%rank        ! single node: MPI rank r drives GPU r
    call check(tse_init(ctx, a), 'cuda_mod_init')
    ! elem(:) is one contiguous allocation (prim_driver_mod.F90:221): page-lock it once, so that copy_qdp_h2d/d2h and the
    ! per-step derived fields are single 2-D DMAs straight out of / into the element structures
    if (nelemd > 1) then
       call check(tse_host_register(ctx, c_loc(elem(1)), stride_of(c_loc(elem(1)), c_loc(elem(2)))*int(nelemd,c_size_t)), &
                  'tse_host_register')
    endif
    if (use_rccl) then
       ! ncclCommInitRank is a blocking collective: every rank first checks what it can check alone, and only if ALL are ready
       ! does anyone enter it (a rank failing alone inside would strand the others in the bootstrap)
       rc_comm = tse_comm_precheck(ctx, int(hybrid%par%rank,c_int), int(hybrid%par%nprocs,c_int))
       call MPI_Allreduce(rc_comm, rc_any, 1, MPI_INTEGER, MPI_MAX, hybrid%par%comm, ierr)
       if (rc_any == 0) then
          if (hybrid%par%rank == 0) call check(tse_comm_unique_id(c_loc(comm_id)), 'tse_comm_unique_id')
          call MPI_Bcast(comm_id, 128, MPI_CHARACTER, 0, hybrid%par%comm, ierr)
          rc_comm = tse_comm_init(ctx, c_loc(comm_id), int(hybrid%par%rank,c_int), int(hybrid%par%nprocs,c_int))
          call MPI_Allreduce(rc_comm, rc_any, 1, MPI_INTEGER, MPI_MAX, hybrid%par%comm, ierr)
       endif
       if (rc_any /= 0) then     ! every rank leaves RCCL together: the halo goes through tse_f_exchange (MPI) instead
          call check(tse_comm_abort(ctx), 'tse_comm_abort')
          if (hybrid%par%rank == 0) write(*,'(a)') ' cuda_mod_hip: WARNING: RCCL communicator could not be initialised; halo exchange over MPI'
       endif
    endif
    if (ns + nr > 0) then
       allocate(x_slen(max(ns,1),2), x_rlen(max(nr,1),2))
       x_slen(1:ns,1) = slen(1:ns); x_rlen(1:nr,1) = rlen(1:nr)
       call check(tse_halo_minmax_layout(ctx, c_loc(x_slen(1,2)), c_loc(x_rlen(1,2))), 'tse_halo_minmax_layout')
       call check(tse_halo_layout(ctx, ncs, ncr), 'tse_halo_layout')
       ! largest message: max(qsize*nlev + nlev, 2*qpad*nlev) layers per column (the bounds arrays carry the tracer count rounded up
       ! to a multiple of 4, transport_se_hip.h)
       allocate(x_hsend(max(1,ncs)*max(qsize*nlev + nlev, 2*((qsize+3)/4*4)*nlev)), x_hrecv(max(1,ncr)*max(qsize*nlev + nlev, 2*((qsize+3)/4*4)*nlev)))
    endif
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine cuda_mod_init

  ! bndry_exchangeV (bndry_mod.F90:74-124) on the packed slots: MPICH here is not GPU-aware, so the slots are staged
  ! through host buffers; with a GPU-aware MPI the two hipMemcpy calls disappear and the device pointers go to MPI.
  integer(c_int) function tse_f_exchange(user, sendbuf, recvbuf, nlyr, kind) bind(C)
    type(c_ptr),    value :: user, sendbuf, recvbuf
    integer(c_int), value :: nlyr, kind
    integer :: i, off, ierr, nreq, ntot_s, ntot_r
    integer :: req(x_nsend + x_nrecv), stat(MPI_STATUS_SIZE, x_nsend + x_nrecv)
    tse_f_exchange = 1
    ntot_s = sum(x_slen(1:x_nsend, kind+1)); ntot_r = sum(x_rlen(1:x_nrecv, kind+1))
    if (ntot_s > 0) then
       if (hipMemcpy(c_loc(x_hsend), sendbuf, int(ntot_s,c_size_t)*nlyr*8_c_size_t, 2_c_int) /= 0) return
    endif
    nreq = 0; off = 0
    do i = 1, x_nrecv
       if (x_rlen(i,kind+1) > 0) then
          nreq = nreq + 1
          call MPI_Irecv(x_hrecv(off*nlyr + 1), x_rlen(i,kind+1)*nlyr, MPI_DOUBLE_PRECISION, rpeer(i), 10, x_comm, req(nreq), ierr)
       endif
       off = off + x_rlen(i,kind+1)
    enddo
    off = 0
    do i = 1, x_nsend
       if (x_slen(i,kind+1) > 0) then
          nreq = nreq + 1
          call MPI_Isend(x_hsend(off*nlyr + 1), x_slen(i,kind+1)*nlyr, MPI_DOUBLE_PRECISION, speer(i), 10, x_comm, req(nreq), ierr)
       endif
       off = off + x_slen(i,kind+1)
    enddo
    call MPI_Waitall(nreq, req, stat, ierr)
    if (ntot_r > 0) then
       if (hipMemcpy(recvbuf, c_loc(x_hrecv), int(ntot_r,c_size_t)*nlyr*8_c_size_t, 1_c_int) /= 0) return
    endif
    tse_f_exchange = 0
  end function tse_f_exchange

  integer(c_size_t) function estride(elem)
    type(element_t), intent(in), target :: elem(:)
    estride = stride_of(c_loc(elem(1)%state%Qdp), c_loc(elem(min(2,size(elem)))%state%Qdp))
  end function estride

  subroutine copy_qdp_h2d(elem, nt)
    type(element_t), intent(in), target :: elem(:)
    integer, intent(in) :: nt
    !$OMP BARRIER
    !$OMP MASTER
    call tic()
    call check(tse_copy_qdp_h2d(ctx, c_loc(elem(1)%state%Qdp), estride(elem), int(qsize_d,c_int), int(nt,c_int)), 'copy_qdp_h2d')
    call toc(1)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine copy_qdp_h2d

  subroutine copy_qdp_d2h(elem, nt)
    type(element_t), intent(in), target :: elem(:)
    integer, intent(in) :: nt
    !$OMP BARRIER
    !$OMP MASTER
    call tic()
    call check(tse_copy_qdp_d2h(ctx, c_loc(elem(1)%state%Qdp), estride(elem), int(qsize_d,c_int), int(nt,c_int)), 'copy_qdp_d2h')
    call toc(2)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine copy_qdp_d2h

  subroutine euler_step_cuda(np1_qdp, n0_qdp, dt, elem, hvcoord, hybrid, deriv, nets, nete, DSSopt, rhs_multiplier)
    integer,              intent(in)            :: np1_qdp, n0_qdp
    real(kind=real_kind), intent(in)            :: dt
    type(element_t),      intent(inout), target :: elem(:)
    type(hvcoord_t),      intent(in)            :: hvcoord
    type(hybrid_t),       intent(in)            :: hybrid
    type(derivative_t),   intent(in)            :: deriv
    integer,              intent(in)            :: nets, nete, DSSopt, rhs_multiplier
    integer(c_size_t) :: s
    type(c_ptr) :: pdiv, peta, pomg
    ! (every thread arrives with its own nets:nete: the barrier makes the host-side writes of all of them -- elem%derived of the
    ! tracer step -- visible before the master stages them, and the closing barrier keeps the others out of Qdp until it is back)
    !$OMP BARRIER
    !$OMP MASTER
    call tic()
    s = estride(elem)   ! every field lives in the same fixed-size element_t, so one stride serves all
    ! The CUDA seam stages elem%derived on every call (cuda_mod.F90:535-547, 564-586).  Nothing on the host changes vn0, dp,
    ! divdp, eta_dot_dpdn or omega_p between the three euler_step calls of a tracer step (prim_advection_mod.F90:614-637), and
    ! the DSS'd divdp_proj / eta_dot_dpdn of the earlier stages are already on the device, so the inputs are uploaded once per
    ! tracer step (with the first stage, rhs_multiplier = 0) and only the variable this stage DSSes is copied back.
    if (rhs_multiplier == 0) then
       call check(tse_set_derived(ctx, c_loc(elem(1)%derived%vn0), s, c_loc(elem(1)%derived%dp), s, &
                                  c_loc(elem(1)%derived%eta_dot_dpdn), s, c_loc(elem(1)%derived%omega_p), s), 'tse_set_derived')
       call check(tse_set_divdp(ctx, c_loc(elem(1)%derived%divdp), s, c_loc(elem(1)%derived%divdp_proj), s), 'tse_set_divdp')
    endif
    call check(tse_euler_step(ctx, int(np1_qdp,c_int), int(n0_qdp,c_int), dt, int(DSSopt,c_int), int(rhs_multiplier,c_int)), &
               'euler_step_cuda')
    pdiv = c_null_ptr; peta = c_null_ptr; pomg = c_null_ptr
    if (DSSopt == 3) pdiv = c_loc(elem(1)%derived%divdp_proj)   ! DSSdiv_vdp_ave (prim_advection_mod.F90:454-456)
    if (DSSopt == 1) peta = c_loc(elem(1)%derived%eta_dot_dpdn)
    if (DSSopt == 2) pomg = c_loc(elem(1)%derived%omega_p)
    call check(tse_get_derived(ctx, pdiv, s, peta, s, pomg, s, c_null_ptr, 0_c_size_t, c_null_ptr, 0_c_size_t, &
                               c_null_ptr, 0_c_size_t), 'tse_get_derived')
    call toc(3)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine euler_step_cuda

  ! The body of Prim_Advec_Tracers_remap_rk2 (prim_advection_mod.F90:600-636: divdp = div(vn0), three euler_steps, qdp_time_avg)
  ! as ONE call.  Only this entry may leave Qdp(np1) un-materialised between the stages (DSS on read), which makes it ~20 %
  ! faster than the three per-stage hooks.  The reference has no hook at this level; a maintainer adds, after
  ! `call TimeLevel_Qdp(tl, qsplit, n0_qdp, np1_qdp)` (prim_advection_mod.F90:604):
  !     #if USE_CUDA_FORTRAN
  !       call advec_tracers_remap_rk2_hip(elem, dt, n0_qdp, np1_qdp); call t_stopf('prim_advec_tracers_remap_rk2'); return
  !     #endif
  subroutine advec_tracers_remap_rk2_hip(elem, dt, n0_qdp, np1_qdp)
    type(element_t),      intent(inout), target :: elem(:)
    real(kind=real_kind), intent(in)            :: dt
    integer,              intent(in)            :: n0_qdp, np1_qdp
    integer(c_size_t) :: s
    !$OMP BARRIER
    !$OMP MASTER
    call tic()
    s = estride(elem)
    call check(tse_set_derived(ctx, c_loc(elem(1)%derived%vn0), s, c_loc(elem(1)%derived%dp), s, &
                               c_loc(elem(1)%derived%eta_dot_dpdn), s, c_loc(elem(1)%derived%omega_p), s), 'tse_set_derived')
    call check(tse_advec_tracers_remap_rk2(ctx, dt, int(n0_qdp,c_int), int(np1_qdp,c_int)), 'advec_tracers_remap_rk2_hip')
    ! what the three stages leave in elem%derived: DSS'd divdp_proj, eta_dot_dpdn, omega_p, and divdp
    call check(tse_get_derived(ctx, c_loc(elem(1)%derived%divdp_proj), s, c_loc(elem(1)%derived%eta_dot_dpdn), s, &
                               c_loc(elem(1)%derived%omega_p), s, c_loc(elem(1)%derived%divdp), s, c_null_ptr, 0_c_size_t, &
                               c_null_ptr, 0_c_size_t), 'tse_get_derived')
    call toc(4)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine advec_tracers_remap_rk2_hip

  subroutine qdp_time_avg_cuda(elem, rkstage, n0_qdp, np1_qdp, limiter_option, nu_p, nets, nete)
    type(element_t),      intent(inout) :: elem(:)
    real(kind=real_kind), intent(in)    :: nu_p
    integer,              intent(in)    :: rkstage, n0_qdp, np1_qdp, nets, nete, limiter_option
    !$OMP BARRIER
    !$OMP MASTER
    call tic()
    call check(tse_qdp_time_avg(ctx, int(rkstage,c_int), int(n0_qdp,c_int), int(np1_qdp,c_int)), 'qdp_time_avg_cuda')
    call toc(3)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine qdp_time_avg_cuda

  ! call site: vertical_remap_cuda(elem,hvcoord,dt,np1,np1_qdp,nets,nete)   (prim_advection_mod.F90:1280)
  subroutine vertical_remap_cuda(elem, hvcoord, dt, np1, np1_qdp, nets, nete)
    type(element_t),      intent(inout), target :: elem(:)
    type(hvcoord_t),      intent(in)    :: hvcoord
    real(kind=real_kind), intent(in)    :: dt
    integer,              intent(in)    :: np1, np1_qdp, nets, nete
    integer(c_size_t) :: s
    integer :: ie
    real(kind=real_kind), allocatable, target :: dp3d(:,:,:,:), psv(:,:,:)
    !$OMP BARRIER
    !$OMP MASTER
    call tic()
    s = estride(elem)
    call check(tse_set_derived(ctx, c_null_ptr, 0_c_size_t, c_loc(elem(1)%derived%dp), s, c_null_ptr, 0_c_size_t, &
                               c_null_ptr, 0_c_size_t), 'tse_set_derived')
    call check(tse_set_divdp(ctx, c_null_ptr, 0_c_size_t, c_loc(elem(1)%derived%divdp_proj), s), 'tse_set_divdp')
    call check(tse_vertical_remap(ctx, dt, int(np1_qdp,c_int)), 'vertical_remap_cuda')
    ! state%dp3d(:,:,:,np1) and state%ps_v(:,:,np1) are time-level slices: stage through dense arrays
    allocate(dp3d(np,np,nlev,nelemd), psv(np,np,nelemd))
    call check(tse_get_derived(ctx, c_null_ptr, 0_c_size_t, c_null_ptr, 0_c_size_t, c_null_ptr, 0_c_size_t, c_null_ptr, &
                               0_c_size_t, c_loc(dp3d), int(np*np*nlev*8,c_size_t), c_loc(psv), int(np*np*8,c_size_t)), &
               'tse_get_derived')
    do ie = 1, nelemd
       elem(ie)%state%dp3d(:,:,:,np1) = dp3d(:,:,:,ie)
       elem(ie)%state%ps_v(:,:,np1)   = psv(:,:,ie)
    enddo
    call toc(5)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine vertical_remap_cuda

  ! ---- the device-resident prim_run loop ---------------------------------------------------------------------------------
  ! A host that lets the library run whole prim_run_subcycle calls replaces, in prim_run (prim_driver_mod.F90:686-689, 701-943):
  !     call cuda_mod_init(elem, hybrid, deriv, hvcoord)                  ! as for the per-stage hooks
  !     call dcmip_init_hip(elem, hvcoord, 1)                             ! prescribed DCMIP 1-1 fields and initial state, on the device
  !     call prim_run_subcycle_hip(elem, hvcoord, tl, dt, nsub)           ! nsub x prim_run_subcycle; Qdp never leaves the device
  !     call copy_state_d2h_hip(elem, tl, want_qdp=.false., want_q=.true.) ! only when the host reads the state (output, diagnostics)
  ! Qdp, dp3d and ps_v live on the device between the calls; elem(:) holds them only after copy_state_d2h_hip.

  subroutine tic_res()
    call system_clock(t_c0)
  end subroutine tic_res
  subroutine toc_res(i)
    integer, intent(in) :: i
    integer(kind=8) :: c1, rate
    call system_clock(c1, rate)
    t_res(i) = t_res(i) + dble(c1 - t_c0)/dble(rate)
  end subroutine toc_res
  subroutine hip_resident_report(nsteps)
    integer, intent(in) :: nsteps
    write(*,'(a,i6,a)') ' hip resident: wall seconds inside the resident-loop entries over ', nsteps, ' tracer steps'
    write(*,'(a,3f10.4)') ' hip resident: dcmip_init_hip prim_run_subcycle_hip copy_state_d2h_hip =', t_res
    write(*,'(a,es14.6)') ' hip resident: tracer-DOF-steps/s of prim_run_subcycle_hip + copy_state_d2h_hip = ', &
         dble(nelemd)*np*np*nlev*qsize*nsteps/max(t_res(2) + t_res(3), 1d-30)
  end subroutine hip_resident_report

  ! the prescribed DCMIP fields of test_case (1: dcmip1-1, 2: dcmip1-2) on the device, and the initial state they define: what
  ! set_dcmip_1_1_fields / set_dcmip_1_2_fields at time 0 and prim_init2's Qdp = Q*dp do (dcmip_wrapper_mod.F90:49-243,
  ! prim_driver_mod.F90:646-669), for both Qdp time levels, dp3d and ps_v.  elem(:) is not written.
  subroutine dcmip_init_hip(elem, hvcoord, test_case)
    type(element_t), intent(in), target :: elem(:)
    type(hvcoord_t), intent(in) :: hvcoord
    integer,         intent(in) :: test_case
    real(c_double), allocatable, target :: lat(:,:,:), lon(:,:,:), hyam(:), hybm(:)
    integer :: ie, i, j
    !$OMP BARRIER
    !$OMP MASTER
    call check_nlev('dcmip_init_hip')
    call tic_res()
    allocate(lat(np,np,nelemd), lon(np,np,nelemd), hyam(nlev), hybm(nlev))
    do ie = 1, nelemd
       do j = 1, np
          do i = 1, np
             lat(i,j,ie) = elem(ie)%spherep(i,j)%lat
             lon(i,j,ie) = elem(ie)%spherep(i,j)%lon
          enddo
       enddo
    enddo
    hyam = hvcoord%hyam; hybm = hvcoord%hybm
    call check(tse_dcmip_init(ctx, int(test_case,c_int), c_loc(lat), c_loc(lon), c_loc(hyam), c_loc(hybm)), 'dcmip_init_hip')
    call check(tse_dcmip_set_initial(ctx), 'dcmip_init_hip')
    deallocate(lat, lon, hyam, hybm)
    call toc_res(1)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine dcmip_init_hip

  ! nsub calls of prim_run_subcycle (prim_driver_mod.F90:701-850) in one device call: per cycle rsplit x (the prescribed step inputs
  ! + Prim_Advec_Tracers_remap_rk2) and vertical_remap, Qdp device-resident throughout.  tl advances as nsub calls of the reference's
  ! routine advance it (qsplit = 1: rsplit leapfrog updates per cycle, time_mod.F90:111-140), and the library's step count must
  ! then equal tl%nstep (it does unless tl%nstep lay inside an rsplit cycle).
  subroutine prim_run_subcycle_hip(elem, hvcoord, tl, dt, nsub)
    type(element_t),      intent(inout), target :: elem(:)
    type(hvcoord_t),      intent(in)    :: hvcoord
    type(TimeLevel_t),    intent(inout) :: tl
    real(kind=real_kind), intent(in)    :: dt
    integer,              intent(in)    :: nsub
    integer(c_int) :: rc
    integer :: n
    character(len=120) :: text
    !$OMP BARRIER
    !$OMP MASTER
    call tic_res()
    res_nstep = int(tl%nstep, c_int)
    rc = tse_prim_run_subcycle(ctx, dt*qsplit, int(nsub,c_int), res_nstep)
    ! the reference aborts the job in vertical_remap (prim_advection_mod.F90:1323)
    if (rc == 2) call seam_abort('negative layer thickness.  timestep or remap time too large')
    call check(rc, 'prim_run_subcycle_hip')
    call toc_res(2)
#ifndef HORIZ_OPENMP
    do n = 1, nsub*rsplit
       call TimeLevel_update(tl, "leapfrog")
    enddo
#endif
    !$OMP END MASTER
    !$OMP BARRIER
#ifdef HORIZ_OPENMP
    do n = 1, nsub*rsplit    ! (every thread: TimeLevel_update synchronises the threads itself, time_mod.F90:118-139)
       call TimeLevel_update(tl, "leapfrog")
    enddo
#endif
    !$OMP MASTER
    if (tl%nstep /= res_nstep) then
       write(text,'(a,i0,a,i0)') 'prim_run_subcycle_hip: the library stepped to nstep = ', res_nstep, ', tl%nstep = ', tl%nstep
       call seam_abort(trim(text))
    endif
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine prim_run_subcycle_hip

  ! What prim_run_subcycle leaves in elem (prim_driver_mod.F90:795-822), after prim_run_subcycle_hip: state%ps_v and state%dp3d of the
  ! new dynamics level, state%lnps = log(ps_v) there, and -- only on request -- state%Q(:,:,:,1:qsize) = Qdp/dp (formed on the device)
  ! and state%Qdp of the new tracer level (Q on request only: the first request allocates a tracer-sized device field).  The reference fills level np1 / np1_qdp and then advances tl once more (:840), so these are
  ! tl%n0 and the n0 of TimeLevel_Qdp when the host calls this.  Nothing else is downloaded.
  subroutine copy_state_d2h_hip(elem, tl, want_qdp, want_q)
    type(element_t),   intent(inout), target :: elem(:)
    type(TimeLevel_t), intent(in) :: tl
    logical,           intent(in) :: want_qdp, want_q
    integer(c_size_t) :: s
    integer :: ie, nt, nq
    real(kind=real_kind), allocatable, target :: dp3d(:,:,:,:)
    !$OMP BARRIER
    !$OMP MASTER
    call tic_res()
    s = estride(elem)
    nt = tl%n0
    call TimeLevel_Qdp(tl, qsplit, nq)
    ! ps_v(:,:,nt) is one contiguous (np,np) block per element: straight into elem; dp3d(:,:,:,nt) is a slice of a 4-D field: staged
    allocate(dp3d(np,np,nlev,nelemd))
    call check(tse_get_derived(ctx, c_null_ptr, 0_c_size_t, c_null_ptr, 0_c_size_t, c_null_ptr, 0_c_size_t, c_null_ptr, &
                               0_c_size_t, c_loc(dp3d), int(np*np*nlev*8,c_size_t), c_loc(elem(1)%state%ps_v(1,1,nt)), s), &
               'copy_state_d2h_hip')
    do ie = 1, nelemd
       elem(ie)%state%dp3d(:,:,:,nt) = dp3d(:,:,:,ie)
    enddo
    deallocate(dp3d)
    if (want_q) then     ! Q and lnps from one device pass
       call check(tse_state_q(ctx, int(nq,c_int)), 'copy_state_d2h_hip')
       call check(tse_copy_q_d2h(ctx, c_loc(elem(1)%state%Q), s, int(qsize_d,c_int)), 'copy_state_d2h_hip')
       call check(tse_copy_lnps_d2h(ctx, c_loc(elem(1)%state%lnps(1,1,nt)), s), 'copy_state_d2h_hip')
    else                 ! no Q requested: the device holds no Q field, and lnps is the reference's own host expression (:809)
       do ie = 1, nelemd
          elem(ie)%state%lnps(:,:,nt) = LOG(elem(ie)%state%ps_v(:,:,nt))
       enddo
    endif
    if (want_qdp) call check(tse_copy_qdp_d2h(ctx, c_loc(elem(1)%state%Qdp), s, int(qsize_d,c_int), int(nq,c_int)), &
                             'copy_state_d2h_hip')
    call toc_res(3)
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine copy_state_d2h_hip

  ! ---- the DCMIP error norms from element partials (tse_norm_*, include/transport_se_hip.h) ----
  ! owner(np,np,nelemd) = 1 where this element's point owns its GLL column (the smallest global dof among the sharers, dof_mod.F90:43-57),
  ! colw(np,np,nelemd) = the column's horizontal weight (read where owner = 1), dh(nlev) = the layer depths.  May be called again.
  subroutine norm_setup_hip(owner, colw, dh)
    integer(c_int), intent(in), target :: owner(np,np,nelemd)
    real(c_double), intent(in), target :: colw(np,np,nelemd), dh(nlev)
    !$OMP BARRIER
    !$OMP MASTER
    call check_nlev('norm_setup_hip')
    call check(tse_norm_setup(ctx, c_loc(owner), c_loc(colw), c_loc(dh)), 'norm_setup_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine norm_setup_hip

  ! snapshot Q0 = Qdp(:,:,:,q,nt)/dp on the device as the reference field (q counts from 1 here, as Fortran's tracer index does);
  ! sum0(ie) = the element's unweighted sum of Q0 over its owned points and levels: avg = repro_sum(sum0) / (nlev * ncol)
  subroutine norm_reference_hip(nt, q, sum0)
    integer,        intent(in)          :: nt, q
    real(c_double), intent(out), target :: sum0(nelemd)
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_norm_reference(ctx, int(nt,c_int), int(q-1,c_int), c_loc(sum0)), 'norm_reference_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine norm_reference_hip

  ! out(1:8,ie): sum |dq| dV, sum dev dV, sum dq*dq dV, sum dev*dev dV, max |dq| dV, max dev dV, max Qf, min Qf over the element's owned
  ! points, Qf = Qdp(:,:,:,q,nt)/dp(ps_v), dq = Qf - Q0, dev = |Q0 - avg|.  The host adds rows 1:4 over elements and ranks with repro_sum
  ! and reduces rows 5:8 with max / min: L1 = s1/s2, L2 = sqrt(s3)/sqrt(s4), Linf = m5/m6, q_max = m7, q_min = m8.
  subroutine norm_partials_hip(nt, q, avg, out)
    integer,        intent(in)          :: nt, q
    real(c_double), intent(in)          :: avg
    real(c_double), intent(out), target :: out(8,nelemd)
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_norm_partials(ctx, int(nt,c_int), int(q-1,c_int), avg, c_loc(out)), 'norm_partials_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine norm_partials_hip

  ! out(1:32,ie): the element's share of the mixing and filament diagnostics (Lauritzen and Thuburn 2012) of tracers qa (chi) and qb (xi),
  ! counted from 1, against the curve xi = c0 + c2*chi**2 (c2 < 0) over chi in [xmin, xmax], with the weights of norm_setup_hip:
  ! rows 1:3 sum d*dV over class A (real mixing), B (range-preserving unmixing), C (overshooting), row 4 sum dV, rows 5:7 the class counts,
  ! row 8 max d, rows 9:8+ntau sum dV where chi >= tau(j).  The host adds rows 1:4 and 9: over elements and ranks with repro_sum:
  ! l_r, l_u, l_o = s1, s2, s3 / s4; l_f(tau_j) = 100 * s(8+j)(t) / s(8+j)(t0).  ntau <= 24.
  subroutine mix_partials_hip(nt, qa, qb, xmin, xmax, c0, c2, tau, ntau, out)
    integer,        intent(in)          :: nt, qa, qb, ntau
    real(c_double), intent(in)          :: xmin, xmax, c0, c2
    real(c_double), intent(in),  target :: tau(*)
    real(c_double), intent(out), target :: out(32,nelemd)
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_mix_partials(ctx, int(nt,c_int), int(qa-1,c_int), int(qb-1,c_int), xmin, xmax, c0, c2, c_loc(tau), int(ntau,c_int), &
                                c_loc(out)), 'mix_partials_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine mix_partials_hip

  ! field (the names of tse_view_put: 'qdp', 'vn0', 'dp', 'eta_dot_dpdn', 'omega_p', 'divdp', 'divdp_proj') <- the host's device array at
  ! ptr (a DEVICE address: c_loc of an OpenMP-target / OpenACC device pointer, a hipMalloc'ed buffer), strides(1:5) in doubles for the axes
  ! element, q, level, j, i (0 for an axis the field does not have); nt: time level of 'qdp' (1|2), ignored otherwise.  stream: the host's
  ! hipStream_t (the copy is ordered behind its work and it behind the copy, nothing waits on the host), or c_null_ptr: complete on return.
  subroutine view_put_hip(field, nt, ptr, strides, stream)
    character(len=*),     intent(in) :: field
    integer,              intent(in) :: nt
    type(c_ptr),          intent(in) :: ptr, stream
    integer(c_long_long), intent(in) :: strides(5)
    type(tse_view) :: v
    v%ptr = ptr; v%stride = strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_view_put(ctx, trim(field)//c_null_char, int(nt,c_int), v, stream), 'view_put_hip('//trim(field)//')')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine view_put_hip

  ! the host's device array <- field ('qdp', 'q', 'lnps', 'divdp_proj', 'eta_dot_dpdn' (levels 1:nlev), 'omega_p', 'divdp', 'dp3d', 'ps_v');
  ! only the addresses the view names are written, and the view may not overlap itself
  subroutine view_get_hip(field, nt, ptr, strides, stream)
    character(len=*),     intent(in) :: field
    integer,              intent(in) :: nt
    type(c_ptr),          intent(in) :: ptr, stream
    integer(c_long_long), intent(in) :: strides(5)
    type(tse_view) :: v
    v%ptr = ptr; v%stride = strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_view_get(ctx, trim(field)//c_null_char, int(nt,c_int), v, stream), 'view_get_hip('//trim(field)//')')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine view_get_hip

  ! Qdp(:,:,:,1:qsize,nt) <- Qdp + the source term of the host's device array at ptr (a "qdp" view: strides(1:5) in doubles for element, q,
  ! level, j, i), clipped so that no tracer mass becomes negative (include/transport_se_hip.h: tse_apply_forcing).  mode forcing_tendency:
  ! dt * FQ is added; forcing_adjust: FQ is the new mixing ratio and dt is ignored.  nt: the level the next tracer step reads as n0
  ! (TimeLevel_Qdp).  stream as in view_put_hip.
  subroutine apply_forcing_hip(nt, dt, mode, ptr, strides, stream)
    integer,              intent(in) :: nt, mode
    real(kind=real_kind), intent(in) :: dt
    type(c_ptr),          intent(in) :: ptr, stream
    integer(c_long_long), intent(in) :: strides(5)
    type(tse_view) :: v
    v%ptr = ptr; v%stride = strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_apply_forcing(ctx, int(nt,c_int), real(dt,c_double), int(mode,c_int), v, stream, c_null_ptr), 'apply_forcing_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine apply_forcing_hip

  ! the same from elem(:)%derived%FQ(:,:,:,:,tl) in host memory (the path of copy_qdp_h2d brings it over); complete on return
  subroutine apply_forcing_elem_hip(elem, nt, tl, dt, mode)
    type(element_t), intent(in), target :: elem(:)
    integer,              intent(in) :: nt, tl, mode
    real(kind=real_kind), intent(in) :: dt
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_apply_forcing_host(ctx, int(nt,c_int), real(dt,c_double), int(mode,c_int), c_loc(elem(1)%derived%FQ(1,1,1,1,tl)), &
                                      estride(elem), int(qsize_d,c_int), c_null_ptr), 'apply_forcing_elem_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine apply_forcing_elem_hip

  ! field(:,:,:,1:nf) of the host's DEVICE array at ptr <- remap_Q_ppm of it from the layer thicknesses at src_ptr to those at tgt_ptr, in
  ! place (include/transport_se_hip.h: tse_remap_view).  strides(1:5) in doubles for element, q, level, j, i; the grids have no q axis
  ! (stride 0).  mode remap_mass: the field is mass per layer (Qdp, u*dp); remap_mean: a layer mean (T, u).  alg: vert_remap_q_alg of
  ! this call.  stream as in view_put_hip.  nrefused (with c_null_ptr as the stream): elements whose grids the device refused and left
  ! as they were (the message names the first); with a stream it is 0 and remap_view_status_hip reports.  Every other failure aborts.
  subroutine remap_view_hip(nf, mode, alg, ptr, strides, src_ptr, src_strides, tgt_ptr, tgt_strides, stream, refused)
    integer,              intent(in)  :: nf, mode, alg
    type(c_ptr),          intent(in)  :: ptr, src_ptr, tgt_ptr, stream
    integer(c_long_long), intent(in)  :: strides(5), src_strides(5), tgt_strides(5)
    logical,              intent(out) :: refused
    type(tse_view) :: vf, vs, vt
    integer(c_int) :: rc
    vf%ptr = ptr; vf%stride = strides
    vs%ptr = src_ptr; vs%stride = src_strides
    vt%ptr = tgt_ptr; vt%stride = tgt_strides
    !$OMP BARRIER
    !$OMP MASTER
    rc = tse_remap_view(ctx, int(nf,c_int), int(mode,c_int), int(alg,c_int), vf, vs, vt, stream)
    if (rc /= 0 .and. rc /= 2) call check(rc, 'remap_view_hip')
    remap_refused = (rc == 2)
    !$OMP END MASTER
    !$OMP BARRIER
    refused = remap_refused
  end subroutine remap_view_hip

  ! what remap_view_hip calls with a stream refused since the last read: the number of elements, and in first(1:4) the element, column,
  ! level (all counted from 0) and code (1..4) of the first one; waits for the library's compute stream, then clears
  subroutine remap_view_status_hip(nrefused, first)
    integer, intent(out) :: nrefused, first(4)
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_remap_view_status(ctx, remap_nrefused, remap_where), 'remap_view_status_hip')
    !$OMP END MASTER
    !$OMP BARRIER
    nrefused = remap_nrefused; first = remap_where
  end subroutine remap_view_status_hip

  ! field(:,:,1:nk,1:nf) of the host's DEVICE array at ptr <- rspheremp * DSS(w) of it, in place (include/transport_se_hip.h:
  ! tse_dss_view): the spheremp* -> edgeVpack -> bndry_exchangeV -> edgeVunpack -> rspheremp* idiom in one call.  strides(1:5) in doubles
  ! for element, q, level, j, i (an axis of extent 1 may carry stride 0).  mode dss_average: w = spheremp * f (a nodal field: u, T, dp3d,
  ! ps_v); dss_weak: w = f (the result of a weak operator).  nk: 1 to nlev + 1 levels.  COLLECTIVE: every rank calls with the same nf, nk
  ! and mode.  stream as in view_put_hip.  A refusal aborts.
  subroutine dss_view_hip(nf, nk, mode, ptr, strides, stream)
    integer,              intent(in) :: nf, nk, mode
    type(c_ptr),          intent(in) :: ptr, stream
    integer(c_long_long), intent(in) :: strides(5)
    type(tse_view) :: v
    v%ptr = ptr; v%stride = strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_dss_view(ctx, int(nf,c_int), int(nk,c_int), int(mode,c_int), v, stream), 'dss_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine dss_view_hip

  ! out(1:16, [1:nk,] 1:nf, 1:nelemd) <- the element shares of min, max, sum, integral, norms and the non-finite count of
  ! field(:,:,1:nk,1:nf) of the host's DEVICE array at ptr (include/transport_se_hip.h: tse_stats_view names the 16 entries and the order
  ! of addition): what prim_printstate and global_integral / l1_snorm / l2_snorm / linf_snorm need, without the field leaving the device.
  ! out is HOST memory, tse_stats * nf * nelemd doubles (per_level = 0) or tse_stats * nk * nf * nelemd (per_level = 1); the host adds the
  ! shares of all elements and ranks (repro_sum).  strides(1:5) in doubles for element, q, level, j, i.  ref_ptr / ref_strides: the true
  ! solution ht of the *_snorm functions, a view of the same nf and nk, or c_null_ptr for none; w_ptr / w_strides: ONE field of nk levels
  ! that multiplies spheremp (dp3d), its q stride not looked at, or c_null_ptr for none.  Nothing is written on the device; the arrays may
  ! be the library's own.  Not collective.  stream is waited for; the call is complete on return.  A refusal aborts.
  subroutine stats_view_hip(nf, nk, per_level, ptr, strides, ref_ptr, ref_strides, w_ptr, w_strides, stream, out)
    integer,              intent(in) :: nf, nk, per_level
    type(c_ptr),          intent(in) :: ptr, ref_ptr, w_ptr, stream
    integer(c_long_long), intent(in) :: strides(5), ref_strides(5), w_strides(5)
    real(c_double), intent(out), target :: out(*)
    type(tse_view), target :: v, r, w
    type(c_ptr) :: rp, wp
    v%ptr = ptr; v%stride = strides
    r%ptr = ref_ptr; r%stride = ref_strides
    w%ptr = w_ptr; w%stride = w_strides
    rp = c_null_ptr; wp = c_null_ptr
    if (c_associated(ref_ptr)) rp = c_loc(r)
    if (c_associated(w_ptr)) wp = c_loc(w)
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_stats_view(ctx, int(nf,c_int), int(nk,c_int), int(per_level,c_int), v, rp, wp, stream, c_loc(out)), 'stats_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine stats_view_hip

  ! out at out_ptr <- one vertical scan of the host's DEVICE arrays, levels from 1 at the model top (include/transport_se_hip.h:
  ! tse_column_view states the arithmetic):
  !   col_pint   dp3d(:,:,1:nlev)                                  -> p_i(:,:,1:nlev+1), p_i(1) = ptop
  !   col_pmid   dp3d(:,:,1:nlev)                                  -> p(:,:,1:nlev)
  !   col_phi    a = T_v(:,:,1:nlev), b = phis(:,:), dp3d [, p]    -> phi(:,:,1:nlev)      preq_hydrostatic; rgas = Rgas
  !   col_omega  a = vgrad_p(:,:,1:nlev), b = divdp(:,:,1:nlev), p or else dp3d -> omega_p(:,:,1:nlev)   preq_omega_ps
  ! An absent view is c_null_ptr (its strides are not read): p, a and b of col_pint / col_pmid; p of col_phi and col_omega when the
  ! mid-point pressure is to be formed from dp3d on the fly; dp of col_omega when p is given.  ptop = hvcoord%hyai(1) * hvcoord%ps0.
  ! strides(1:5) in doubles for element, q, level, j, i; the q stride is never stepped, nor the level stride of phis:
  ! state%dp3d(np,np,nlev,timelevels) at time level n0 is (/ s_e, 0, 16, 4, 1 /) from the address of dp3d(1,1,1,n0).  The inputs may be
  ! the library's own fields; out may not, and may not overlap an input.  Not collective.  stream as in view_put_hip.  A refusal aborts.
  subroutine column_view_hip(op, ptop, rgas, dp_ptr, dp_strides, p_ptr, p_strides, a_ptr, a_strides, b_ptr, b_strides, out_ptr, out_strides, stream)
    integer,              intent(in) :: op
    real(c_double),       intent(in) :: ptop, rgas
    type(c_ptr),          intent(in) :: dp_ptr, p_ptr, a_ptr, b_ptr, out_ptr, stream
    integer(c_long_long), intent(in) :: dp_strides(5), p_strides(5), a_strides(5), b_strides(5), out_strides(5)
    type(tse_view), target :: vd, vp, va, vb
    type(tse_view) :: vo
    type(c_ptr) :: d, p, a, b
    vd%ptr = dp_ptr; vd%stride = dp_strides
    vp%ptr = p_ptr;  vp%stride = p_strides
    va%ptr = a_ptr;  va%stride = a_strides
    vb%ptr = b_ptr;  vb%stride = b_strides
    vo%ptr = out_ptr; vo%stride = out_strides
    d = c_null_ptr; p = c_null_ptr; a = c_null_ptr; b = c_null_ptr
    if (c_associated(dp_ptr)) d = c_loc(vd)
    if (c_associated(p_ptr)) p = c_loc(vp)
    if (c_associated(a_ptr)) a = c_loc(va)
    if (c_associated(b_ptr)) b = c_loc(vb)
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_column_view(ctx, int(op,c_int), ptop, rgas, d, p, a, b, vo, stream), 'column_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine column_view_hip

  ! out(:,:,1:nk,1:nf) at out_ptr <- laplace_sphere_wk of field(:,:,1:nk,1:nf) of the host's DEVICE array at ptr (order lap_order1: weak,
  ! not summed, no exchange) or laplace_sphere_wk(rspheremp * DSS(laplace_sphere_wk(field))) (lap_order2: biharmonic_wk_scalar before its
  ! final DSS; include/transport_se_hip.h: tse_biharmonic_view).  strides(1:5) and out_strides(1:5) in doubles for element, q, level, j, i.
  ! out_ptr and out_strides equal to ptr and strides: in place; otherwise the two arrays may not overlap.  nk: 1 to nlev + 1 levels.
  ! COLLECTIVE for lap_order2: every rank calls with the same nf and nk.  The host scales by -nu*dt and follows with
  ! dss_view_hip(..., dss_weak, ...).  stream as in view_put_hip.  A refusal aborts.
  subroutine biharmonic_view_hip(nf, nk, order, ptr, strides, out_ptr, out_strides, stream)
    integer,              intent(in) :: nf, nk, order
    type(c_ptr),          intent(in) :: ptr, out_ptr, stream
    integer(c_long_long), intent(in) :: strides(5), out_strides(5)
    type(tse_view) :: vi, vo
    vi%ptr = ptr; vi%stride = strides
    vo%ptr = out_ptr; vo%stride = out_strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_biharmonic_view(ctx, int(nf,c_int), int(nk,c_int), int(order,c_int), vi, vo, stream), 'biharmonic_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine biharmonic_view_hip

  ! elem(:)%D, %metinv and %mp -> the device, folded there into the tables of vlaplace_view_hip (include/transport_se_hip.h:
  ! tse_vector_setup).  Once after cuda_mod_init, before the first vlaplace_view_hip; may be called again.
  subroutine vector_setup_hip(elem)
    type(element_t), intent(in), target :: elem(:)
    integer :: e2
    e2 = min(2, size(elem))
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_vector_setup(ctx, c_loc(elem(1)%D), stride_of(c_loc(elem(1)%D), c_loc(elem(e2)%D)), &
                                c_loc(elem(1)%metinv), stride_of(c_loc(elem(1)%metinv), c_loc(elem(e2)%metinv)), &
                                c_loc(elem(1)%mp), stride_of(c_loc(elem(1)%mp), c_loc(elem(e2)%mp))), 'vector_setup_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine vector_setup_hip

  ! out(:,:,1:2,1:nk) at out_ptr <- vlaplace_sphere_wk of v(:,:,1:2,1:nk) of the host's DEVICE array at ptr (order vlap_order1: weak, not
  ! summed, no exchange) or vlaplace_sphere_wk(rspheremp * DSS(vlaplace_sphere_wk(v))) (vlap_order2: the wind's line of biharmonic_wk_dp3d
  ! before its final DSS; include/transport_se_hip.h: tse_vlaplace_view).  nu_ratio multiplies the divergence in every Laplacian.
  ! strides(1:5) and out_strides(1:5) in doubles for element, component, level, j, i: state%v(np,np,2,nlev,tl) is (/ s_e, 16, 32, 4, 1 /)
  ! with one call per time level.  out_ptr and out_strides equal to ptr and strides: in place; otherwise the two arrays may not overlap.
  ! COLLECTIVE for vlap_order2: every rank calls with the same nk.  The host scales by -nu*dt and follows with
  ! dss_view_hip(2, nk, dss_weak, ...).  stream as in view_put_hip.  A refusal aborts.
  subroutine vlaplace_view_hip(nk, order, nu_ratio, ptr, strides, out_ptr, out_strides, stream)
    integer,              intent(in) :: nk, order
    real(c_double),       intent(in) :: nu_ratio
    type(c_ptr),          intent(in) :: ptr, out_ptr, stream
    integer(c_long_long), intent(in) :: strides(5), out_strides(5)
    type(tse_view) :: vi, vo
    vi%ptr = ptr; vi%stride = strides
    vo%ptr = out_ptr; vo%stride = out_strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_vlaplace_view(ctx, int(nk,c_int), int(order,c_int), nu_ratio, vi, vo, stream), 'vlaplace_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine vlaplace_view_hip

  ! One sub-step of advance_hypervis on the host's DEVICE arrays (include/transport_se_hip.h: tse_hypervis_view):
  !   x <- x + rspheremp * DSS(coef * biharmonic(x))
  ! for the nf scalar fields s(:,:,1:nk,1:nf) at s_ptr -- T and dp3d of elem(:), two members at one element stride, are ONE view whose
  ! q stride is the distance between the members -- and the wind v(:,:,1:2,1:nk) at v_ptr (state%v(np,np,2,nlev,tl): (/ s_e, 16, 32, 4, 1 /)),
  ! with two exchanges where biharmonic_view_hip, vlaplace_view_hip and two dss_view_hip make four.  coef(1:nf+1): the host's
  ! -nu*dt/hypervis_subcycle for each scalar field and, last, for the wind.  nu_ratio as in vlaplace_view_hip.  A half is absent with
  ! nf = 0 and s_ptr = c_null_ptr, or v_ptr = c_null_ptr.  so_ptr / vo_ptr (optional, with their strides): device arrays that receive
  ! the tendencies rspheremp * DSS(coef * biharmonic(x)) instead -- given for exactly the halves that are present; s and v then keep
  ! every bit; absent or c_null_ptr: in place.  COLLECTIVE: every rank calls with the same nf, nk and presence of v.  Needs
  ! vector_setup_hip with a wind.  stream as in view_put_hip.  A refusal aborts.
  subroutine hypervis_view_hip(nf, nk, coef, nu_ratio, s_ptr, s_strides, v_ptr, v_strides, stream, so_ptr, so_strides, vo_ptr, vo_strides)
    integer,              intent(in) :: nf, nk
    real(c_double),       intent(in) :: coef(nf+1), nu_ratio
    type(c_ptr),          intent(in) :: s_ptr, v_ptr, stream
    integer(c_long_long), intent(in) :: s_strides(5), v_strides(5)
    type(c_ptr),          intent(in), optional :: so_ptr, vo_ptr
    integer(c_long_long), intent(in), optional :: so_strides(5), vo_strides(5)
    type(tse_view), target :: vs, vv, vso, vvo
    type(c_ptr) :: s, v, so, vo
    vs%ptr = s_ptr; vs%stride = s_strides
    vv%ptr = v_ptr; vv%stride = v_strides
    s = c_null_ptr; v = c_null_ptr; so = c_null_ptr; vo = c_null_ptr
    if (c_associated(s_ptr)) s = c_loc(vs)
    if (c_associated(v_ptr)) v = c_loc(vv)
    if (present(so_ptr) .and. present(so_strides)) then
      vso%ptr = so_ptr; vso%stride = so_strides
      if (c_associated(so_ptr)) so = c_loc(vso)
    end if
    if (present(vo_ptr) .and. present(vo_strides)) then
      vvo%ptr = vo_ptr; vvo%stride = vo_strides
      if (c_associated(vo_ptr)) vo = c_loc(vvo)
    end if
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_hypervis_view(ctx, int(nf,c_int), int(nk,c_int), coef, nu_ratio, s, v, so, vo, stream), 'hypervis_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine hypervis_view_hip

  ! out at out_ptr <- op of nk levels of the host's DEVICE array at ptr (include/transport_se_hip.h: tse_sphere_op_view):
  !   op_gradient    s(:,:,1:nk)     -> out(:,:,1:2,1:nk)   gradient_sphere
  !   op_divergence  v(:,:,1:2,1:nk) -> out(:,:,1:nk)       divergence_sphere
  !   op_vorticity   v(:,:,1:2,1:nk) -> out(:,:,1:nk)       vorticity_sphere (needs vector_setup_hip)
  ! c0 = op_local: on every element by itself, no exchange.  c0 = op_c0: rspheremp * DSS(spheremp * op(...)), the make_C0 of
  ! viscosity_mod (compute_zeta_C0, compute_div_C0); COLLECTIVE: every rank calls with the same nk and op.
  ! strides(1:5) and out_strides(1:5) in doubles for element, component, level, j, i: state%v(np,np,2,nlev,tl) is (/ s_e, 16, 32, 4, 1 /)
  ! with one call per time level; the component stride of the scalar side is free (0).  The two arrays may not overlap: there is no
  ! in-place form.  stream as in view_put_hip.  A refusal aborts.
  subroutine sphere_op_view_hip(nk, op, c0, ptr, strides, out_ptr, out_strides, stream)
    integer,              intent(in) :: nk, op, c0
    type(c_ptr),          intent(in) :: ptr, out_ptr, stream
    integer(c_long_long), intent(in) :: strides(5), out_strides(5)
    type(tse_view) :: vi, vo
    vi%ptr = ptr; vi%stride = strides
    vo%ptr = out_ptr; vo%stride = out_strides
    !$OMP BARRIER
    !$OMP MASTER
    call check(tse_sphere_op_view(ctx, int(nk,c_int), int(op,c_int), int(c0,c_int), vi, vo, stream), 'sphere_op_view_hip')
    !$OMP END MASTER
    !$OMP BARRIER
  end subroutine sphere_op_view_hip

end module cuda_mod
