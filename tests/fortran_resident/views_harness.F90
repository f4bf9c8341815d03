! views_harness.F90 -- TEST INFRASTRUCTURE (built into oracle/_ref/dropin by tests/fortran_resident/Makefile; never shipped).
!
! A Fortran host that calls every view wrapper of the seam (transport_se_amd/fortran/cuda_mod_hip.F90) on device arrays of its own,
! laid out as E3SM lays its state out, and dumps what went in and what came back (tests/test_gpu_fortran_views.py reads it):
!     view_put_hip, view_get_hip, apply_forcing_hip, apply_forcing_elem_hip, remap_view_hip, remap_view_status_hip, dss_view_hip,
!     biharmonic_view_hip, vector_setup_hip, vlaplace_view_hip, sphere_op_view_hip, norm_setup_hip, norm_reference_hip,
!     norm_partials_hip, mix_partials_hip  (and dcmip_init_hip, copy_state_d2h_hip)
! The mesh is set up with the reference's own public routines as resident_harness.F90 does; the operator inputs are
! oracle/ref/fieldops_fill.F90's, so they are those of tests/golden/ref_ne2_fieldops.npz.  The host arrays are
!     v(np,np,2,nlev,3)  T(np,np,nlev,3)  ps(np,np,3)  Qdp(np,np,nlev,qsize_d,2)   per element, and lf(nlev,np,np,qsize) level-fastest;
! every call works on time level 2, so that neither the base offset nor the element stride of a view is the trivial one.  Every operator
! call is made twice: with c_null_ptr as the stream (suffix _s0) and on a created stream followed by hipStreamSynchronize (_s1).
! Every return code is checked; the first failure stops the program with a message and a non-zero exit.
!
! stdin (list-directed): ne qsize  /  'outdir'  /  'vcoord dir'.   outdir/weights.bin (written by the test from diagnostics.column_weights):
!     nelem, ntau (int4); owner(16,nelem) (int4); colw(16,nelem); dh(nlev); tau(ntau); xmin, xmax, c0, c2   -- by global element number
! Output: static_000000_r<rank>.bin in the layout of ref_harness's dump_static, and views_000000_r<rank>.bin, a sequence of records
!     name (24 characters), ndim (int4), dims(ndim) (int4), data (real8, Fortran order)
program views_harness
  use iso_c_binding
  use kinds,              only : real_kind
  use dimensions_mod,     only : np, nlev, nlevp, ne, nelem, nelemd, nelemdmax, qsize, qsize_d, npart, nnodes, nmpi_per_node
  use control_mod,        only : topology, partmethod, nu_q, limiter_option, hypervis_order, hypervis_subcycle_q, rsplit, &
                                 qsplit, test_case, cubed_sphere_map, hypervis_power, hypervis_scaling, integration, &
                                 tstep_type, nu, nu_p, nu_s
  use params_mod,         only : SFCURVE
  use parallel_mod,       only : parallel_t, initmp, iam, haltmp, global_shared_buf, nrepro_vars, mpiinteger_t
  use hybrid_mod,         only : hybrid_t, hybrid_create
  use thread_mod,         only : nthreads
  use element_mod,        only : element_t, allocate_element_desc
  use gridgraph_mod,      only : gridvertex_t, gridedge_t, allocate_gridvertex_nbrs
  use metagraph_mod,      only : metavertex_t, localelemcount, initmetagraph
  use schedtype_mod,      only : schedule
  use schedule_mod,       only : genEdgeSched
  use spacecurve_mod,     only : genspacepart
  use cube_mod,           only : cubeedgecount, cubeelemcount, cubetopology, cube_init_atomic, rotation_init_atomic, &
                                 set_corner_coordinates, assign_node_numbers_to_elem
  use quadrature_mod,     only : quadrature_t, gausslobatto
  use mass_matrix_mod,    only : mass_matrix
  use repro_sum_mod,      only : repro_sum, repro_sum_defaultopts, repro_sum_setopts
  use physical_constants, only : dd_pi
  use hybvcoord_mod,      only : hvcoord_t, hvcoord_init
  use time_mod,           only : timelevel_t, timelevel_init, timelevel_qdp, tstep
  use derivative_mod,     only : derivative_t, derivinit
  use fieldops_fill,      only : fo_nk, fo_fill, fo_lcg
  use cuda_mod,           only : cuda_mod_init, dcmip_init_hip, copy_state_d2h_hip, view_put_hip, view_get_hip, apply_forcing_hip, &
                                 apply_forcing_elem_hip, forcing_tendency, remap_view_hip, remap_view_status_hip, remap_mass, &
                                 remap_mean, dss_view_hip, dss_average, dss_weak, biharmonic_view_hip, lap_order1, lap_order2, &
                                 vector_setup_hip, vlaplace_view_hip, vlap_order1, vlap_order2, sphere_op_view_hip, op_gradient, &
                                 op_divergence, op_vorticity, op_local, op_c0, norm_setup_hip, norm_reference_hip, &
                                 norm_partials_hip, mix_partials_hip
  implicit none
#include <mpif.h>

  interface
     integer(c_int) function hipMalloc(p, nbytes) bind(C, name='hipMalloc')
       import; type(c_ptr), intent(out) :: p; integer(c_size_t), value :: nbytes
     end function
     integer(c_int) function hipFree(p) bind(C, name='hipFree')
       import; type(c_ptr), value :: p
     end function
     integer(c_int) function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy')
       import; type(c_ptr), value :: dst, src; integer(c_size_t), value :: nbytes; integer(c_int), value :: kind
     end function
     integer(c_int) function hipStreamCreate(s) bind(C, name='hipStreamCreate')
       import; type(c_ptr), intent(out) :: s
     end function
     integer(c_int) function hipStreamSynchronize(s) bind(C, name='hipStreamSynchronize')
       import; type(c_ptr), value :: s
     end function
     integer(c_int) function hipStreamDestroy(s) bind(C, name='hipStreamDestroy')
       import; type(c_ptr), value :: s
     end function
  end interface

  real(kind=real_kind), parameter :: SENT = -7.25d0
  integer, parameter :: nk = fo_nk, TL2 = 2
  type (element_t), pointer :: elem(:)
  type (parallel_t)   :: par
  type (hybrid_t)     :: hybrid
  type (timelevel_t)  :: tl
  type (hvcoord_t)    :: hvcoord
  type (derivative_t) :: deriv
  type (quadrature_t) :: gp
  type (GridVertex_t), target, allocatable :: GridVertex(:)
  type (GridEdge_t),   target, allocatable :: GridEdge(:)
  type (MetaVertex_t), target, allocatable :: MetaVertex(:)
  real(kind=real_kind), allocatable :: aratio(:,:)
  real(kind=real_kind) :: area(1)
  logical :: rs_ddpdd, rs_recompute
  real(kind=real_kind) :: rs_rel
  integer :: ne_in, qsize_in, nelem_edge, ie, j, ierr, m
  character(len=256) :: outdir, vdir
  character(len=512) :: fname
  ! the host's arrays, E3SM's shapes with the element last, and their device copies
  real(c_double), allocatable, target :: hv(:,:,:,:,:,:), hT(:,:,:,:,:), hps(:,:,:,:), hQ(:,:,:,:,:,:), hlf(:,:,:,:,:)
  real(c_double), allocatable, target :: wv(:,:,:,:,:,:), wT(:,:,:,:,:), wQ(:,:,:,:,:,:), sv_(:,:,:,:,:,:), sT_(:,:,:,:,:)
  real(c_double), allocatable, target :: hF(:,:,:,:,:,:), hG1(:,:,:,:,:), hG2(:,:,:,:,:), hB(:,:,:,:,:)
  type(c_ptr) :: dV, dV2, dT, dT2, dQ, dF, dLF, dG1, dG2, dPS, stream
  integer(c_size_t) :: nV, nT, nQ, nLF, nPS
  integer(c_long_long) :: sV(5), sT(5), sT0(5), sQ(5), sLF(5), sLF0(5), sPS(5), oV, oT, oQ, oPS

  par = initmp()
  if (par%masterproc) then
     read(*,*) ne_in, qsize_in
     read(*,*) outdir
     read(*,*) vdir
  endif
  call MPI_Bcast(ne_in,   1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(qsize_in,1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(outdir, 256, MPI_CHARACTER, 0, par%comm, ierr)
  call MPI_Bcast(vdir,   256, MPI_CHARACTER, 0, par%comm, ierr)

  ! ---- the namelist values of the DCMIP 1-1 runs ----
  ne = ne_in;  qsize = qsize_in;  tstep = 1800.0d0
  topology = "cube";  partmethod = SFCURVE;  npart = par%nprocs
  nmpi_per_node = 1;  nnodes = npart;  nthreads = 1
  nu = 0; nu_p = 0; nu_s = 0; nu_q = 1.0d19
  limiter_option = 8; hypervis_order = 2; hypervis_subcycle_q = 1
  hypervis_power = 0; hypervis_scaling = 0
  qsplit = 1; rsplit = 3; tstep_type = 1; integration = "explicit"
  cubed_sphere_map = 0
  test_case = "dcmip1-1"
  call repro_sum_defaultopts(repro_sum_use_ddpdd_out=rs_ddpdd, repro_sum_rel_diff_max_out=rs_rel, &
                             repro_sum_recompute_out=rs_recompute)
  call repro_sum_setopts(repro_sum_use_ddpdd_in=rs_ddpdd, repro_sum_rel_diff_max_in=rs_rel, &
                         repro_sum_recompute_in=rs_recompute, repro_sum_master=par%masterproc, repro_sum_logunit=6)

  ! ---- cube topology, space-filling-curve partition, edge schedule (prim_init1) ----
  nelem      = CubeElemCount()
  nelem_edge = CubeEdgeCount()
  allocate(GridVertex(nelem), GridEdge(nelem_edge))
  do j = 1, nelem
     call allocate_gridvertex_nbrs(GridVertex(j))
  enddo
  call CubeTopology(GridEdge, GridVertex)
  call genspacepart(GridEdge, GridVertex)
  allocate(MetaVertex(1), Schedule(1))
  call initMetaGraph(iam, MetaVertex(1), GridVertex, GridEdge)
  nelemd = LocalElemCount(MetaVertex(1))
  call mpi_allreduce(nelemd, nelemdmax, 1, MPIinteger_t, MPI_MAX, par%comm, ierr)
  allocate(elem(nelemd))
  call allocate_element_desc(elem)
  call genEdgeSched(elem, iam, Schedule(1), MetaVertex(1))
  allocate(global_shared_buf(nelemd, nrepro_vars)); global_shared_buf = 0

  ! ---- element geometry, mass matrix, and the area correction that makes the sphere's area 4 pi ----
  gp = gausslobatto(np)
  do ie = 1, nelemd
     call set_corner_coordinates(elem(ie))
  enddo
  call assign_node_numbers_to_elem(elem, GridVertex)
  do ie = 1, nelemd
     call cube_init_atomic(elem(ie), gp%points)
  enddo
  call mass_matrix(par, elem)
  allocate(aratio(nelemd,1))
  do ie = 1, nelemd
     aratio(ie,1) = sum(elem(ie)%mp(:,:)*elem(ie)%metdet(:,:))
  enddo
  call repro_sum(aratio, area, nelemd, nelemd, 1, commid=par%comm)
  area(1) = 4*dd_pi/area(1)
  deallocate(aratio)
  do ie = 1, nelemd
     call cube_init_atomic(elem(ie), gp%points, area(1))
     call rotation_init_atomic(elem(ie), "contravariant")
  enddo
  call mass_matrix(par, elem)
  do ie = 1, nelemd
     elem(ie)%state%Qdp = 0; elem(ie)%state%Q = 0; elem(ie)%state%dp3d = 0; elem(ie)%state%ps_v = 0; elem(ie)%state%lnps = 0
     elem(ie)%derived%vn0 = 0; elem(ie)%derived%dp = 0; elem(ie)%derived%divdp = 0; elem(ie)%derived%divdp_proj = 0
     elem(ie)%derived%eta_dot_dpdn = 0; elem(ie)%derived%omega_p = 0; elem(ie)%derived%FQ = 0
  enddo

  ! ---- prim_init2: time levels, vertical coordinate, derivative operator; then the seam ----
  call TimeLevel_init(tl)
  hybrid = hybrid_create(par, 0, 1)
  hvcoord = hvcoord_init(trim(vdir)//'/acme-72m.ascii', trim(vdir)//'/acme-72i.ascii', .false., par%masterproc, ierr)
  if (ierr /= 0) call fail('hvcoord_init failed')
  call derivinit(deriv)
  call cuda_mod_init(elem, hybrid, deriv, hvcoord)
  call vector_setup_hip(elem)
  call dump_static()

  ! ---- the host's arrays and views (strides in doubles: element, q, level, j, i; every view starts at time level 2) ----
  allocate(hv(np,np,2,nlev,3,nelemd), wv(np,np,2,nlev,3,nelemd), sv_(np,np,2,nlev,3,nelemd))
  allocate(hT(np,np,nlev,3,nelemd), wT(np,np,nlev,3,nelemd), sT_(np,np,nlev,3,nelemd))
  allocate(hG1(np,np,nlev,3,nelemd), hG2(np,np,nlev,3,nelemd), hB(np,np,nlev,3,nelemd))
  allocate(hps(np,np,3,nelemd), hQ(np,np,nlev,qsize_d,2,nelemd), wQ(np,np,nlev,qsize_d,2,nelemd), hF(np,np,nlev,qsize_d,2,nelemd))
  allocate(hlf(nlev,np,np,qsize,nelemd))
  nV = size(hv); nT = size(hT); nQ = size(hQ); nLF = size(hlf); nPS = size(hps)
  sV   = (/ 96_8*nlev, 16_8, 32_8, 4_8, 1_8 /);                    oV = 32_8*nlev
  sT   = (/ 48_8*nlev, 16_8*nlev, 16_8, 4_8, 1_8 /);               oT = 16_8*nlev       ! (one field: the q stride is never stepped)
  sT0  = (/ 48_8*nlev, 0_8, 16_8, 4_8, 1_8 /)                                          ! the same for a field without a q axis
  sQ   = (/ 32_8*nlev*qsize_d, 16_8*nlev, 16_8, 4_8, 1_8 /);      oQ = 16_8*nlev*qsize_d
  sLF  = (/ 16_8*nlev*qsize, 16_8*nlev, 1_8, 4_8*nlev, 1_8*nlev /)
  sLF0 = (/ 16_8*nlev*qsize, 0_8, 1_8, 4_8*nlev, 1_8*nlev /)
  sPS  = (/ 48_8, 0_8, 0_8, 4_8, 1_8 /);                           oPS = 16_8
  call hipck(hipMalloc(dV, nV*8), 'hipMalloc');   call hipck(hipMalloc(dV2, nV*8), 'hipMalloc')
  call hipck(hipMalloc(dT, nT*8), 'hipMalloc');   call hipck(hipMalloc(dT2, nT*8), 'hipMalloc')
  call hipck(hipMalloc(dG1, nT*8), 'hipMalloc');  call hipck(hipMalloc(dG2, nT*8), 'hipMalloc')
  call hipck(hipMalloc(dQ, nQ*8), 'hipMalloc');   call hipck(hipMalloc(dF, nQ*8), 'hipMalloc')
  call hipck(hipMalloc(dLF, nLF*8), 'hipMalloc'); call hipck(hipMalloc(dPS, nPS*8), 'hipMalloc')
  call hipck(hipStreamCreate(stream), 'hipStreamCreate')
  sv_ = SENT; sT_ = SENT

  write(fname,'(a,a,i4.4,a)') trim(outdir), '/views_000000_r', par%rank, '.bin'
  open(unit=32, file=trim(fname), form='unformatted', access='stream', status='replace')
  do ie = 1, nelemd
     hps(1,1,1,ie) = dble(elem(ie)%GlobalId)
  enddo
  call rec('gid', hps(1,1,1,:), (/ nelemd /))
  call dump_metinv()

  ! ---- the operators on nk levels of fieldops_fill's inputs ----
  hv = SENT; hT = SENT
  do ie = 1, nelemd
     call fo_fill(elem(ie)%GlobalId, np, nk, hT(:,:,1:nk,TL2,ie), hv(:,:,:,1:nk,TL2,ie))
  enddo
  call rec('in_s', hT(:,:,1:nk,TL2,:), (/ np, np, nk, nelemd /))
  call rec('in_v', hv(:,:,:,1:nk,TL2,:), (/ np, np, 2, nk, nelemd /))
  do m = 0, 1
     call run_ops(m)
  enddo

  ! ---- put / get, forcing, remap ----
  call run_state()

  ! ---- the norm and mixing partials of the DCMIP 1-1 initial state ----
  call run_norms()

  close(32)
  call hipck(hipStreamDestroy(stream), 'hipStreamDestroy')
  call hipck(hipFree(dV), 'hipFree');  call hipck(hipFree(dV2), 'hipFree'); call hipck(hipFree(dT), 'hipFree')
  call hipck(hipFree(dT2), 'hipFree'); call hipck(hipFree(dG1), 'hipFree'); call hipck(hipFree(dG2), 'hipFree')
  call hipck(hipFree(dQ), 'hipFree');  call hipck(hipFree(dF), 'hipFree');  call hipck(hipFree(dLF), 'hipFree')
  call hipck(hipFree(dPS), 'hipFree')
  ! (not haltmp: its STOP statement writes behind the last line)
  call MPI_Barrier(par%comm, ierr)
  call MPI_Finalize(ierr)
  if (par%masterproc) then
     write(*,'(a)') 'views_harness done'
     flush(6)
  endif

contains

  subroutine fail(text)
    character(len=*), intent(in) :: text
    integer :: ierr
    write(0,'(a)') ' views_harness: FAILED: '//text
    flush(0); flush(6)
    call MPI_Abort(MPI_COMM_WORLD, 1, ierr)
    stop 1
  end subroutine fail

  subroutine hipck(rc, what)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: what
    character(len=80) :: text
    if (rc == 0) return
    write(text,'(a,a,i0)') what, ' returned ', rc
    call fail(trim(text))
  end subroutine hipck

  function off(p, ndoubles) result(q)
    type(c_ptr), intent(in) :: p
    integer(c_long_long), intent(in) :: ndoubles
    type(c_ptr) :: q
    q = transfer(transfer(p, 0_c_intptr_t) + 8_c_intptr_t*ndoubles, q)
  end function off

  subroutine h2d(d, a, n)
    type(c_ptr), intent(in) :: d
    integer(c_size_t), intent(in) :: n
    real(c_double), intent(in), target :: a(*)
    call hipck(hipMemcpy(d, c_loc(a), n*8, 1_c_int), 'hipMemcpy (host to device)')
  end subroutine h2d

  subroutine d2h(a, d, n)
    type(c_ptr), intent(in) :: d
    integer(c_size_t), intent(in) :: n
    real(c_double), intent(inout), target :: a(*)
    call hipck(hipMemcpy(c_loc(a), d, n*8, 2_c_int), 'hipMemcpy (device to host)')
  end subroutine d2h

  subroutine rec(name, a, dims)
    character(len=*), intent(in) :: name
    real(c_double), intent(in) :: a(*)
    integer, intent(in) :: dims(:)
    character(len=24) :: nm
    nm = name
    write(32) nm, int(size(dims),4), int(dims,4), a(1:product(dims))
  end subroutine rec

  subroutine sync(m)
    integer, intent(in) :: m
    if (m == 1) call hipck(hipStreamSynchronize(stream), 'hipStreamSynchronize')
  end subroutine sync

  ! a downloaded T-shaped / v-shaped array: the nk levels of time level 2 are the result, every other entry still holds SENT
  subroutine rec_s(name, m, w)
    character(len=*), intent(in) :: name
    integer, intent(in) :: m
    real(c_double), intent(in) :: w(:,:,:,:,:)
    character(len=3) :: sfx
    write(sfx,'(a,i1)') '_s', m
    if (count(w /= SENT) /= count(w(:,:,1:nk,TL2,:) /= SENT)) call fail('a write outside the view: '//name//sfx)
    call rec(name//sfx, w(:,:,1:nk,TL2,:), (/ np, np, nk, nelemd /))
  end subroutine rec_s
  subroutine rec_v(name, m, w)
    character(len=*), intent(in) :: name
    integer, intent(in) :: m
    real(c_double), intent(in) :: w(:,:,:,:,:,:)
    character(len=3) :: sfx
    write(sfx,'(a,i1)') '_s', m
    if (count(w /= SENT) /= count(w(:,:,:,1:nk,TL2,:) /= SENT)) call fail('a write outside the view: '//name//sfx)
    call rec(name//sfx, w(:,:,:,1:nk,TL2,:), (/ np, np, 2, nk, nelemd /))
  end subroutine rec_v

  subroutine run_ops(m)
    integer, intent(in) :: m
    type(c_ptr) :: strm
    integer :: c0
    real(c_double) :: nu_ratio
    character(len=8) :: tag
    strm = c_null_ptr
    if (m == 1) strm = stream
    nu_ratio = 2.5d0
    ! dss_view_hip, both modes, in place
    call h2d(dT, hT, nT)
    call dss_view_hip(1, nk, dss_average, off(dT,oT), sT, strm); call sync(m)
    call d2h(wT, dT, nT); call rec_s('dss_average', m, wT)
    call h2d(dT, hT, nT)
    call dss_view_hip(1, nk, dss_weak, off(dT,oT), sT, strm); call sync(m)
    call d2h(wT, dT, nT); call rec_s('dss_weak', m, wT)
    ! biharmonic_view_hip: order 1 in place, order 2 into a second array
    call h2d(dT, hT, nT)
    call biharmonic_view_hip(1, nk, lap_order1, off(dT,oT), sT, off(dT,oT), sT, strm); call sync(m)
    call d2h(wT, dT, nT); call rec_s('lap', m, wT)
    call h2d(dT, hT, nT); call h2d(dT2, sT_, nT)
    call biharmonic_view_hip(1, nk, lap_order2, off(dT,oT), sT, off(dT2,oT), sT, strm); call sync(m)
    call d2h(wT, dT2, nT); call rec_s('bih', m, wT)
    ! vlaplace_view_hip, orders 1 and 2
    call h2d(dV, hv, nV); call h2d(dV2, sv_, nV)
    call vlaplace_view_hip(nk, vlap_order1, nu_ratio, off(dV,oV), sV, off(dV2,oV), sV, strm); call sync(m)
    call d2h(wv, dV2, nV); call rec_v('vlap', m, wv)
    call h2d(dV2, sv_, nV)
    call vlaplace_view_hip(nk, vlap_order2, nu_ratio, off(dV,oV), sV, off(dV2,oV), sV, strm); call sync(m)
    call d2h(wv, dV2, nV); call rec_v('vbih', m, wv)
    ! sphere_op_view_hip: three ops, element-local and C0
    do c0 = op_local, op_c0
       tag = ''; if (c0 == op_c0) tag = '_c0'
       call h2d(dT, hT, nT); call h2d(dV2, sv_, nV)
       call sphere_op_view_hip(nk, op_gradient, c0, off(dT,oT), sT, off(dV2,oV), sV, strm); call sync(m)
       call d2h(wv, dV2, nV); call rec_v('grad'//trim(tag), m, wv)
       call h2d(dT2, sT_, nT)
       call sphere_op_view_hip(nk, op_divergence, c0, off(dV,oV), sV, off(dT2,oT), sT, strm); call sync(m)
       call d2h(wT, dT2, nT); call rec_s('div'//trim(tag), m, wT)
       call h2d(dT2, sT_, nT)
       call sphere_op_view_hip(nk, op_vorticity, c0, off(dV,oV), sV, off(dT2,oT), sT, strm); call sync(m)
       call d2h(wT, dT2, nT); call rec_s('vor'//trim(tag), m, wT)
    enddo
  end subroutine run_ops

  subroutine run_state()
    integer(kind=8) :: seed
    integer :: ie, i, j, k, q, ebad, nref, first(4)
    logical :: ref1, ref2, ref3
    real(kind=real_kind) :: fdt, sh, stat(8)
    seed = 424243_8 + 1000_8*par%rank
    ! 'qdp': in from the E3SM layout, out into the level-fastest array
    hQ = SENT
    do ie = 1, nelemd; do q = 1, qsize; do k = 1, nlev; do j = 1, np; do i = 1, np
       hQ(i,j,k,q,TL2,ie) = 1.0d0 + 10.0d0*fo_lcg(seed)
    enddo; enddo; enddo; enddo; enddo
    call rec('put_qdp', hQ(:,:,:,1:qsize,TL2,:), (/ np, np, nlev, qsize, nelemd /))
    call h2d(dQ, hQ, nQ)
    call view_put_hip('qdp', 2, off(dQ,oQ), sQ, c_null_ptr)
    hlf = SENT; call h2d(dLF, hlf, nLF)
    call view_get_hip('qdp', 2, dLF, sLF, c_null_ptr)
    call d2h(hlf, dLF, nLF)
    call rec('get_qdp', hlf, (/ nlev, np, np, qsize, nelemd /))
    ! a field without a q axis, both ways, on the stream: 'omega_p'
    hT = SENT
    do ie = 1, nelemd; do k = 1, nlev; do j = 1, np; do i = 1, np
       hT(i,j,k,TL2,ie) = 250.0d0 + 50.0d0*fo_lcg(seed)
    enddo; enddo; enddo; enddo
    call rec('put_omega_p', hT(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
    call h2d(dT, hT, nT)
    call view_put_hip('omega_p', 0, off(dT,oT), sT0, stream)
    hlf = SENT; call h2d(dLF, hlf, nLF)
    call view_get_hip('omega_p', 0, dLF, sLF0, stream); call sync(1)
    call d2h(hlf, dLF, nLF)
    if (count(hlf(:,:,:,2:qsize,:) /= SENT) /= 0) call fail('a write outside the view: get omega_p')
    call rec('get_omega_p', hlf(:,:,:,1,:), (/ nlev, np, np, nelemd /))
    ! forcing: the same FQ through elem(:)%derived%FQ(:,:,:,:,2) and through a device view; time level 1 of FQ holds another field
    fdt = 100.0d0
    hF = SENT
    do ie = 1, nelemd
       elem(ie)%derived%FQ = 1.0d30
       do q = 1, qsize; do k = 1, nlev; do j = 1, np; do i = 1, np
          elem(ie)%derived%FQ(i,j,k,q,TL2) = 0.2d0*(fo_lcg(seed) - 0.5d0)
          hF(i,j,k,q,TL2,ie) = elem(ie)%derived%FQ(i,j,k,q,TL2)
       enddo; enddo; enddo; enddo
    enddo
    call rec('fq', hF(:,:,:,1:qsize,TL2,:), (/ np, np, nlev, qsize, nelemd /))
    stat(1) = fdt; call rec('forcing_dt', stat, (/ 1 /))
    call apply_forcing_elem_hip(elem, 2, TL2, fdt, forcing_tendency)
    hlf = SENT; call h2d(dLF, hlf, nLF)
    call view_get_hip('qdp', 2, dLF, sLF, c_null_ptr)
    call d2h(hlf, dLF, nLF); call rec('forcing_elem', hlf, (/ nlev, np, np, qsize, nelemd /))
    call view_put_hip('qdp', 2, off(dQ,oQ), sQ, c_null_ptr)          ! Qdp as it was
    call h2d(dF, hF, nQ)
    call apply_forcing_hip(2, fdt, forcing_tendency, off(dF,oQ), sQ, stream); call sync(1)
    hlf = SENT; call h2d(dLF, hlf, nLF)
    call view_get_hip('qdp', 2, dLF, sLF, c_null_ptr)
    call d2h(hlf, dLF, nLF); call rec('forcing_view', hlf, (/ nlev, np, np, qsize, nelemd /))
    ! remap: the source grid the reference thickness moved by up to 2 %, the target the reference thickness of the same column mass
    hG1 = SENT; hG2 = SENT
    do ie = 1, nelemd; do j = 1, np; do i = 1, np
       do k = 1, nlev
          hG2(i,j,k,TL2,ie) = ( hvcoord%hyai(k+1) - hvcoord%hyai(k) )*hvcoord%ps0 + ( hvcoord%hybi(k+1) - hvcoord%hybi(k) )*hvcoord%ps0
          hG1(i,j,k,TL2,ie) = hG2(i,j,k,TL2,ie)*(1.0d0 + 0.04d0*(fo_lcg(seed) - 0.5d0))
       enddo
       sh = sum(hG1(i,j,:,TL2,ie))/sum(hG2(i,j,:,TL2,ie))
       hG2(i,j,:,TL2,ie) = hG2(i,j,:,TL2,ie)*sh
    enddo; enddo; enddo
    call rec('dp_src', hG1(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
    call rec('dp_tgt', hG2(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
    call h2d(dG1, hG1, nT); call h2d(dG2, hG2, nT)
    call h2d(dQ, hQ, nQ)
    call remap_view_hip(qsize, remap_mass, 0, off(dQ,oQ), sQ, off(dG1,oT), sT0, off(dG2,oT), sT0, c_null_ptr, ref1)
    call d2h(wQ, dQ, nQ)
    if (count(wQ /= SENT) /= count(wQ(:,:,:,1:qsize,TL2,:) /= SENT)) call fail('a write outside the view: remap mass')
    call rec('remap_mass', wQ(:,:,:,1:qsize,TL2,:), (/ np, np, nlev, qsize, nelemd /))
    call h2d(dT, hT, nT)
    call remap_view_hip(1, remap_mean, 0, off(dT,oT), sT, off(dG1,oT), sT0, off(dG2,oT), sT0, stream, ref2); call sync(1)
    call d2h(wT, dT, nT)
    if (count(wT /= SENT) /= count(wT(:,:,:,TL2,:) /= SENT)) call fail('a write outside the view: remap mean')
    call rec('remap_mean', wT(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
    call remap_view_status_hip(nref, first)
    stat(1) = merge(1.0d0, 0.0d0, ref1); stat(2) = merge(1.0d0, 0.0d0, ref2); stat(3) = nref
    call rec('remap_good', stat, (/ 3 /))
    ! the refusal: one layer of one column of one element's source grid is negative; on a stream, so the status call reports it
    ebad = min(2, nelemd)
    hB = hG1; hB(2,3,5,TL2,ebad) = -1.0d0
    call h2d(dG1, hB, nT); call h2d(dQ, hQ, nQ)
    call remap_view_hip(qsize, remap_mass, 0, off(dQ,oQ), sQ, off(dG1,oT), sT0, off(dG2,oT), sT0, stream, ref3); call sync(1)
    call remap_view_status_hip(nref, first)
    call d2h(wQ, dQ, nQ)
    call rec('remap_bad', wQ(:,:,:,1:qsize,TL2,:), (/ np, np, nlev, qsize, nelemd /))
    stat(1) = merge(1.0d0, 0.0d0, ref3); stat(2) = nref; stat(3:6) = first; stat(7) = ebad - 1
    call rec('remap_bad_status', stat, (/ 7 /))
  end subroutine run_state

  subroutine run_norms()
    integer(c_int), allocatable, target :: owner(:,:,:)
    integer(c_int), allocatable :: owner_all(:,:)
    real(c_double), allocatable, target :: colw(:,:,:), dh(:), tau(:), sum0(:), out8(:,:), out32(:,:)
    real(c_double), allocatable :: colw_all(:,:)
    real(c_double) :: par4(4), avg, loc(2), glob(2)
    integer(kind=4) :: hdr(2)
    integer :: ie, nqdp, ierr
    open(unit=33, file=trim(outdir)//'/weights.bin', form='unformatted', access='stream', status='old', iostat=ierr)
    if (ierr /= 0) call fail('cannot open '//trim(outdir)//'/weights.bin')
    read(33) hdr
    if (hdr(1) /= nelem .or. hdr(2) < 0 .or. hdr(2) > 24) call fail('weights.bin: element or threshold count')
    allocate(owner_all(16,nelem), colw_all(16,nelem), dh(nlev), tau(max(1,hdr(2))))
    allocate(owner(np,np,nelemd), colw(np,np,nelemd), sum0(nelemd), out8(8,nelemd), out32(32,nelemd))
    read(33) owner_all, colw_all, dh, tau(1:hdr(2)), par4
    close(33)
    do ie = 1, nelemd
       owner(:,:,ie) = reshape(owner_all(:,elem(ie)%GlobalId), (/ np, np /))
       colw(:,:,ie)  = reshape(colw_all(:,elem(ie)%GlobalId), (/ np, np /))
    enddo
    call dcmip_init_hip(elem, hvcoord, 1)
    call norm_setup_hip(owner, colw, dh)
    call norm_reference_hip(1, 2, sum0)
    loc(1) = sum(sum0); loc(2) = count(owner == 1)
    call MPI_Allreduce(loc, glob, 2, MPI_DOUBLE_PRECISION, MPI_SUM, par%comm, ierr)
    avg = glob(1)/(nlev*glob(2))
    call norm_partials_hip(1, 2, avg, out8)
    call mix_partials_hip(1, 1, 2, par4(1), par4(2), par4(3), par4(4), tau, int(hdr(2)), out32)
    call copy_state_d2h_hip(elem, tl, .true., .true.)
    call rec('sum0', sum0, (/ nelemd /))
    loc(1) = avg; call rec('avg', loc, (/ 1 /))
    call rec('norm_partials', out8, (/ 8, nelemd /))
    call rec('mix_partials', out32, (/ 32, nelemd /))
    call TimeLevel_Qdp(tl, qsplit, nqdp)
    do ie = 1, nelemd
       hQ(:,:,:,1:qsize,1,ie) = elem(ie)%state%Qdp(:,:,:,1:qsize,nqdp)
       hQ(:,:,:,1:qsize,2,ie) = elem(ie)%state%Q(:,:,:,1:qsize)
       hps(:,:,1,ie) = elem(ie)%state%ps_v(:,:,tl%n0)
    enddo
    call rec('state_qdp', hQ(:,:,:,1:qsize,1,:), (/ np, np, nlev, qsize, nelemd /))
    call rec('state_q', hQ(:,:,:,1:qsize,2,:), (/ np, np, nlev, qsize, nelemd /))
    call rec('state_ps_v', hps(:,:,1,:), (/ np, np, nelemd /))
    ! ps_v has neither a q nor a level axis: out through a view into ps(np,np,3), time level 2
    hps = SENT; call h2d(dPS, hps, nPS)
    call view_get_hip('ps_v', 0, off(dPS,oPS), sPS, c_null_ptr)
    call d2h(hps, dPS, nPS)
    if (count(hps(:,:,1,:) /= SENT) + count(hps(:,:,3,:) /= SENT) /= 0) call fail('a write outside the view: get ps_v')
    call rec('get_ps_v', hps(:,:,TL2,:), (/ np, np, nelemd /))
  end subroutine run_norms

  subroutine dump_metinv()
    real(c_double), allocatable :: mi(:,:,:,:,:)
    integer :: ie
    allocate(mi(2,2,np,np,nelemd))
    do ie = 1, nelemd
       mi(:,:,:,:,ie) = elem(ie)%metinv
    enddo
    call rec('metinv', mi, (/ 2, 2, np, np, nelemd /))
  end subroutine dump_metinv

  ! the geometry in the record layout of oracle/ref/ref_harness.F90's dump_static (oracle/pyoracle.py: read_static)
  subroutine dump_static()
    integer :: ie, i, j
    integer :: rev(8)
    write(fname,'(a,a,i4.4,a)') trim(outdir), '/static_000000_r', par%rank, '.bin'
    open(unit=31, file=trim(fname), form='unformatted', access='stream', status='replace')
    write(31) int(ne,4), int(nelem,4), int(nelemd,4), int(qsize,4), int(nlev,4), int(np,4), int(par%rank,4), int(par%nprocs,4)
    write(31) area(1)
    write(31) deriv%Dvv
    write(31) real(gp%points,8), real(gp%weights,8)
    write(31) hvcoord%hyai, hvcoord%hybi, hvcoord%hyam, hvcoord%hybm, hvcoord%ps0
    do ie = 1, nelemd
       rev = 0
       do j = 1, 8
          if (elem(ie)%desc%reverse(j)) rev(j) = 1
       enddo
       write(31) int(elem(ie)%GlobalId,4), int(elem(ie)%desc%putmapP(1:8),4), int(elem(ie)%desc%getmapP(1:8),4), int(rev,4), &
                 int(elem(ie)%vertex%face_number,4)
       write(31) ((elem(ie)%spherep(i,j)%lon, i=1,np), j=1,np)
       write(31) ((elem(ie)%spherep(i,j)%lat, i=1,np), j=1,np)
       write(31) elem(ie)%D, elem(ie)%Dinv, elem(ie)%metdet, elem(ie)%rmetdet, elem(ie)%mp, elem(ie)%spheremp, elem(ie)%rspheremp
    enddo
    write(31) int(Schedule(1)%ncycles,4), int(Schedule(1)%nSendCycles,4), int(Schedule(1)%nRecvCycles,4)
    do j = 1, Schedule(1)%nSendCycles
       write(31) int(Schedule(1)%SendCycle(j)%dest,4), int(Schedule(1)%SendCycle(j)%ptrP,4), int(Schedule(1)%SendCycle(j)%lengthP,4)
    enddo
    write(31) int(Schedule(1)%MoveCycle(1)%ptrP,4), int(Schedule(1)%MoveCycle(1)%lengthP,4)
    close(31)
  end subroutine dump_static

end program views_harness
