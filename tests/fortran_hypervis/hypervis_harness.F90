! hypervis_harness.F90 -- TEST INFRASTRUCTURE (built into oracle/_ref/dropin by tests/fortran_hypervis/Makefile; never shipped).
!
! A Fortran host that calls hypervis_view_hip of the seam (transport_se_amd/fortran/cuda_mod_hip.F90) on a device array of its own, laid
! out as E3SM lays elem(:) out, and dumps what went in and what came back (tests/test_gpu_fortran_hypervis.py reads it).  The mesh is set
! up with the reference's own public routines as views_harness.F90 does.  Per element the host array holds three members behind one
! another, each followed by a gap of one slab:
!     T(np,np,nlev,3)  dp3d(np,np,nlev,3)  v(np,np,2,nlev,3)
! T and dp3d of time level 2 are ONE scalar view whose q stride is the distance between the members; v of time level 2 is the wind's
! view (component stride 16, level stride 32).  Two calls, each with c_null_ptr as the stream (suffix _s0) and on a created stream (_s1):
! one in place, one into the dense out arrays ten(np,np,nlev,2) and vten(np,np,2,nlev) on a fresh copy of the state.  The whole host
! array is dumped after each, gaps and the other time levels included.  The first failure stops the program with a non-zero exit.
!
! stdin (list-directed): ne qsize  /  'outdir'  /  'vcoord dir'.
! Output: static_000000_r<rank>.bin in the layout of ref_harness's dump_static, and hypervis_000000_r<rank>.bin, a sequence of records
!     name (24 characters), ndim (int4), dims(ndim) (int4), data (real8, Fortran order)
program hypervis_harness
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
  use cuda_mod,           only : cuda_mod_init, vector_setup_hip, hypervis_view_hip
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
  real(c_double), allocatable, target :: hel(:,:), res(:), mi(:,:,:,:,:)
  type(c_ptr) :: dEL, dTEN, dVTEN, stream
  integer(c_size_t) :: nEL, nTEN, nVTEN
  integer(c_long_long) :: ES, oT, oDP, oV, sS(5), sV(5), sTEN(5), sVTEN(5)
  real(c_double) :: coef(3), nu_ratio
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
  call vector_setup_hip(elem)
  call dump_static()

  ! ---- the host's array and views (strides in doubles: element, q, level, j, i; offsets of the members within an element) ----
  oT = 0_8;  oDP = oT + 48_8*nlev + 16_8;  oV = oDP + 48_8*nlev + 16_8;  ES = oV + 96_8*nlev + 16_8
  allocate(hel(ES,nelemd), res(ES*nelemd), mi(2,2,np,np,nelemd))
  nEL = int(ES,c_size_t)*nelemd; nTEN = int(np*np*nlev*2,c_size_t)*nelemd; nVTEN = nTEN
  sS    = (/ ES, oDP - oT, 16_8, 4_8, 1_8 /)
  sV    = (/ ES, 16_8, 32_8, 4_8, 1_8 /)
  sTEN  = (/ 32_8*nlev, 16_8*nlev, 16_8, 4_8, 1_8 /)
  sVTEN = (/ 32_8*nlev, 16_8, 32_8, 4_8, 1_8 /)
  coef = (/ -3.1d21, -1.7d21, -7.3d20 /)
  nu_ratio = 2.5d0
  call hipck(hipMalloc(dEL, nEL*8), 'hipMalloc'); call hipck(hipMalloc(dTEN, nTEN*8), 'hipMalloc'); call hipck(hipMalloc(dVTEN, nVTEN*8), 'hipMalloc')
  call hipck(hipStreamCreate(stream), 'hipStreamCreate')

  write(fname,'(a,a,i4.4,a)') trim(outdir), '/hypervis_000000_r', par%rank, '.bin'
  open(unit=32, file=trim(fname), form='unformatted', access='stream', status='replace')
  hel = SENT
  do ie = 1, nelemd
     seed = 717171_8 + 7919_8*elem(ie)%GlobalId
     mi(:,:,:,:,ie) = elem(ie)%metinv
     do k = 1, 3*nlev; do i = 1, np*np          ! every time level of T and dp3d
        hel(oT  + 16*(k-1) + i, ie) = 180.0d0 + 140.0d0*rnd(seed)
        hel(oDP + 16*(k-1) + i, ie) = 500.0d0 + 1000.0d0*rnd(seed)
     enddo; enddo
     do k = 1, 6*nlev; do i = 1, np*np          ! every time level and both components of v
        hel(oV + 16*(k-1) + i, ie) = 90.0d0*(rnd(seed) - 0.5d0)
     enddo; enddo
  enddo
  call rec('metinv', mi, (/ 2, 2, np, np, nelemd /))
  res(1) = dble(ES); res(2) = dble(oT); res(3) = dble(oDP); res(4) = dble(oV)
  call rec('layout', res, (/ 4 /))
  res(1:3) = coef; res(4) = nu_ratio
  call rec('coef_nu', res, (/ 4 /))
  call rec('in_state', hel, (/ int(ES), nelemd /))
  do m = 0, 1
     call run_hypervis(m)
  enddo
  close(32)
  call hipck(hipStreamDestroy(stream), 'hipStreamDestroy')
  call hipck(hipFree(dEL), 'hipFree'); call hipck(hipFree(dTEN), 'hipFree'); call hipck(hipFree(dVTEN), 'hipFree')
  ! (not haltmp: its STOP statement writes behind the last line)
  call MPI_Barrier(par%comm, ierr)
  call MPI_Finalize(ierr)
  if (par%masterproc) then
     write(*,'(a)') 'hypervis_harness done'
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
    write(0,'(a)') ' hypervis_harness: FAILED: '//text
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


  ! one record: a device array of n doubles as it came back
  subroutine rec_o(name, m, d, n, dims)
    character(len=*), intent(in) :: name
    integer, intent(in) :: m, dims(:)
    type(c_ptr), intent(in) :: d
    integer(c_size_t), intent(in) :: n
    character(len=3) :: sfx
    write(sfx,'(a,i1)') '_s', m
    res = SENT
    call d2h(res, d, n)
    call rec(name//sfx, res, dims)
  end subroutine rec_o

  subroutine clear(d, n)
    type(c_ptr), intent(in) :: d
    integer(c_size_t), intent(in) :: n
    res = SENT
    call h2d(d, res, n)
  end subroutine clear

  subroutine run_hypervis(m)
    integer, intent(in) :: m
    type(c_ptr) :: strm
    strm = c_null_ptr
    if (m == 1) strm = stream
    ! in place, on time level 2 of the three members
    call h2d(dEL, hel, nEL)
    call hypervis_view_hip(2, nlev, coef, nu_ratio, off(dEL, oT + 16_8*nlev), sS, off(dEL, oV + 32_8*nlev), sV, strm)
    if (m == 1) call hipck(hipStreamSynchronize(stream), 'hipStreamSynchronize')
    call rec_o('state', m, dEL, nEL, (/ int(ES), nelemd /))
    ! into the out arrays, on a fresh copy of the state
    call h2d(dEL, hel, nEL); call clear(dTEN, nTEN); call clear(dVTEN, nVTEN)
    call hypervis_view_hip(2, nlev, coef, nu_ratio, off(dEL, oT + 16_8*nlev), sS, off(dEL, oV + 32_8*nlev), sV, strm, dTEN, sTEN, dVTEN, sVTEN)
    if (m == 1) call hipck(hipStreamSynchronize(stream), 'hipStreamSynchronize')
    call rec_o('kept', m, dEL, nEL, (/ int(ES), nelemd /))
    call rec_o('ten', m, dTEN, nTEN, (/ np, np, nlev, 2, nelemd /))
    call rec_o('vten', m, dVTEN, nVTEN, (/ np, np, 2, nlev, nelemd /))
    if (count(res(1:nVTEN) == SENT) /= 0) call fail('vten was not written')
  end subroutine run_hypervis

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

end program hypervis_harness
