! column_harness.F90 -- TEST INFRASTRUCTURE (built into oracle/_ref/dropin by tests/fortran_column/Makefile; never shipped).
!
! A Fortran host that calls column_view_hip of the seam (transport_se_amd/fortran/cuda_mod_hip.F90) on device arrays of its own, laid out as
! E3SM lays its state out, and dumps what went in and what came back (tests/test_gpu_fortran_column.py reads it).  The mesh is set up with
! the reference's own public routines as views_harness.F90 does.  The host arrays are, per element,
!     dp3d(np,np,nlev,3)  T(np,np,nlev,3)  vgrad_p(np,np,nlev,3)  divdp(np,np,nlev,3)  phis(np,np)
! and the results  p_i(np,np,nlevp)  p(np,np,nlev)  phi(np,np,nlev)  omega_p(np,np,nlev);
! every call on dp3d, T, vgrad_p and divdp works on time level 2, so that neither the base offset nor the element stride of a view is
! the trivial one.  The four ops are called with c_null_ptr as the stream (suffix _s0) and on a created stream (_s1); phi and omega with
! the pressure formed on the fly and with the p of the pmid call.  The first failure stops the program with a non-zero exit.
!
! stdin (list-directed): ne qsize  /  'outdir'  /  'vcoord dir'.
! Output: static_000000_r<rank>.bin in the layout of ref_harness's dump_static, and column_000000_r<rank>.bin, a sequence of records
!     name (24 characters), ndim (int4), dims(ndim) (int4), data (real8, Fortran order)
program column_harness
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
  use fieldops_fill,      only : fo_lcg
  use cuda_mod,           only : cuda_mod_init, column_view_hip, col_pint, col_pmid, col_phi, col_omega
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
  integer, parameter :: TL2 = 2
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
  real(c_double), allocatable, target :: hdp(:,:,:,:,:), hT(:,:,:,:,:), hvg(:,:,:,:,:), hdiv(:,:,:,:,:), hphis(:,:,:), res(:)
  type(c_ptr) :: dDP, dT, dVG, dDIV, dPHIS, dPI, dP, dPHI, dOM, stream
  integer(c_size_t) :: nT, nS, nI, nO
  integer(c_long_long) :: sT(5), sS(5), sI(5), sO(5), none(5), oT
  real(c_double) :: ptop, rgas
  integer(kind=8) :: seed
  integer :: i, k

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
  call dump_static()

  ! ---- the host's arrays and views (strides in doubles: element, q, level, j, i; the E3SM-shaped inputs start at time level 2) ----
  allocate(hdp(np,np,nlev,3,nelemd), hT(np,np,nlev,3,nelemd), hvg(np,np,nlev,3,nelemd), hdiv(np,np,nlev,3,nelemd), hphis(np,np,nelemd))
  allocate(res(np*np*nlevp*nelemd))
  nT = size(hdp); nS = size(hphis); nI = int(np*np*nlevp,c_size_t)*nelemd; nO = int(np*np*nlev,c_size_t)*nelemd
  sT   = (/ 48_8*nlev, 0_8, 16_8, 4_8, 1_8 /);    oT = 16_8*nlev
  sS   = (/ 16_8, 0_8, 0_8, 4_8, 1_8 /)
  sI   = (/ 16_8*nlevp, 0_8, 16_8, 4_8, 1_8 /)
  sO   = (/ 16_8*nlev, 0_8, 16_8, 4_8, 1_8 /)
  none = 0
  ptop = hvcoord%hyai(1)*hvcoord%ps0
  rgas = 287.04d0
  call hipck(hipMalloc(dDP, nT*8), 'hipMalloc');  call hipck(hipMalloc(dT, nT*8), 'hipMalloc');   call hipck(hipMalloc(dVG, nT*8), 'hipMalloc')
  call hipck(hipMalloc(dDIV, nT*8), 'hipMalloc'); call hipck(hipMalloc(dPHIS, nS*8), 'hipMalloc'); call hipck(hipMalloc(dPI, nI*8), 'hipMalloc')
  call hipck(hipMalloc(dP, nO*8), 'hipMalloc');   call hipck(hipMalloc(dPHI, nO*8), 'hipMalloc'); call hipck(hipMalloc(dOM, nO*8), 'hipMalloc')
  call hipck(hipStreamCreate(stream), 'hipStreamCreate')

  write(fname,'(a,a,i4.4,a)') trim(outdir), '/column_000000_r', par%rank, '.bin'
  open(unit=32, file=trim(fname), form='unformatted', access='stream', status='replace')
  hdp = SENT; hT = SENT; hvg = SENT; hdiv = SENT
  do ie = 1, nelemd
     seed = 616161_8 + 7919_8*elem(ie)%GlobalId
     hphis(1,1,ie) = dble(elem(ie)%GlobalId)
     do k = 1, nlev; do j = 1, np; do i = 1, np
        hdp(i,j,k,TL2,ie)  = (hvcoord%hyai(k+1) - hvcoord%hyai(k))*hvcoord%ps0 + (hvcoord%hybi(k+1) - hvcoord%hybi(k))*1.0d5*(0.95d0 + 0.1d0*rnd(seed))
        hT(i,j,k,TL2,ie)   = 180.0d0 + 140.0d0*rnd(seed)
        hvg(i,j,k,TL2,ie)  = 2.0d0*(rnd(seed) - 0.5d0)
        hdiv(i,j,k,TL2,ie) = 1.0d-5*hdp(i,j,k,TL2,ie)*(rnd(seed) - 0.5d0)
     enddo; enddo; enddo
  enddo
  call rec('gid', hphis(1,1,:), (/ nelemd /))
  do ie = 1, nelemd; do j = 1, np; do i = 1, np
     hphis(i,j,ie) = 2.0d4*(rnd(seed) - 0.3d0)
  enddo; enddo; enddo
  call rec('in_dp', hdp(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
  call rec('in_T', hT(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
  call rec('in_vgrad_p', hvg(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
  call rec('in_divdp', hdiv(:,:,:,TL2,:), (/ np, np, nlev, nelemd /))
  call rec('in_phis', hphis, (/ np, np, nelemd /))
  res(1) = ptop; res(2) = rgas
  call rec('ptop_rgas', res, (/ 2 /))
  call h2d(dDP, hdp, nT); call h2d(dT, hT, nT); call h2d(dVG, hvg, nT); call h2d(dDIV, hdiv, nT); call h2d(dPHIS, hphis, nS)
  do m = 0, 1
     call run_column(m)
  enddo
  close(32)
  call hipck(hipStreamDestroy(stream), 'hipStreamDestroy')
  call hipck(hipFree(dDP), 'hipFree');  call hipck(hipFree(dT), 'hipFree');    call hipck(hipFree(dVG), 'hipFree')
  call hipck(hipFree(dDIV), 'hipFree'); call hipck(hipFree(dPHIS), 'hipFree'); call hipck(hipFree(dPI), 'hipFree')
  call hipck(hipFree(dP), 'hipFree');   call hipck(hipFree(dPHI), 'hipFree');  call hipck(hipFree(dOM), 'hipFree')
  ! (not haltmp: its STOP statement writes behind the last line)
  call MPI_Barrier(par%comm, ierr)
  call MPI_Finalize(ierr)
  if (par%masterproc) then
     write(*,'(a)') 'column_harness done'
     flush(6)
  endif

contains

  ! a uniform number in [0, 1) over the whole mantissa
  function rnd(sd) result(x)
    integer(kind=8), intent(inout) :: sd
    real(c_double) :: x
    x = fo_lcg(sd); x = x + fo_lcg(sd)/2147483648.0d0
  end function rnd
  subroutine fail(text)
    character(len=*), intent(in) :: text
    integer :: ierr
    write(0,'(a)') ' column_harness: FAILED: '//text
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


  ! one record: a result as it came back, (np,np,nk,nelemd); the device array is refilled with the sentinel first by `clear`
  subroutine rec_o(name, m, d, nk)
    character(len=*), intent(in) :: name
    integer, intent(in) :: m, nk
    type(c_ptr), intent(in) :: d
    character(len=3) :: sfx
    write(sfx,'(a,i1)') '_s', m
    if (m == 1) call hipck(hipStreamSynchronize(stream), 'hipStreamSynchronize')
    res = SENT
    call d2h(res, d, int(np*np*nk,c_size_t)*nelemd)
    if (count(res(1:np*np*nk*nelemd) == SENT) /= 0) call fail('a result was not written: '//name)
    call rec(name//sfx, res, (/ np, np, nk, nelemd /))
  end subroutine rec_o

  subroutine clear(d, n)
    type(c_ptr), intent(in) :: d
    integer(c_size_t), intent(in) :: n
    res = SENT
    call h2d(d, res, n)
  end subroutine clear

  subroutine run_column(m)
    integer, intent(in) :: m
    type(c_ptr) :: strm
    strm = c_null_ptr
    if (m == 1) strm = stream
    call clear(dPI, nI); call clear(dP, nO)
    call column_view_hip(col_pint, ptop, rgas, off(dDP,oT), sT, c_null_ptr, none, c_null_ptr, none, c_null_ptr, none, dPI, sI, strm)
    call rec_o('pint', m, dPI, nlevp)
    call column_view_hip(col_pmid, ptop, rgas, off(dDP,oT), sT, c_null_ptr, none, c_null_ptr, none, c_null_ptr, none, dP, sO, strm)
    call rec_o('pmid', m, dP, nlev)
    ! the geopotential and omega / p with the pressure formed on the fly, and with the p the call above left
    call clear(dPHI, nO); call clear(dOM, nO)
    call column_view_hip(col_phi, ptop, rgas, off(dDP,oT), sT, c_null_ptr, none, off(dT,oT), sT, dPHIS, sS, dPHI, sO, strm)
    call rec_o('phi', m, dPHI, nlev)
    call column_view_hip(col_omega, ptop, rgas, off(dDP,oT), sT, c_null_ptr, none, off(dVG,oT), sT, off(dDIV,oT), sT, dOM, sO, strm)
    call rec_o('omega', m, dOM, nlev)
    call clear(dPHI, nO); call clear(dOM, nO)
    call column_view_hip(col_phi, ptop, rgas, off(dDP,oT), sT, dP, sO, off(dT,oT), sT, dPHIS, sS, dPHI, sO, strm)
    call rec_o('phi_p', m, dPHI, nlev)
    call column_view_hip(col_omega, ptop, rgas, c_null_ptr, none, dP, sO, off(dVG,oT), sT, off(dDIV,oT), sT, dOM, sO, strm)
    call rec_o('omega_p', m, dOM, nlev)
  end subroutine run_column

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

end program column_harness
