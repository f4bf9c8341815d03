! resident_harness.F90 -- TEST INFRASTRUCTURE (built into oracle/_ref/dropin by tests/fortran_resident/Makefile; never shipped).
!
! A Fortran host of the device-resident route of the seam (transport_se_amd/fortran/cuda_mod_hip.F90): the mesh is set up with the
! reference's own public routines, as prim_init1/prim_init2 do (prim_driver_mod.F90:32-371,375-696, minus namelist/IO/restart), then
!     cuda_mod_init -> dcmip_init_hip -> prim_run_subcycle_hip (one rsplit cycle per call) -> copy_state_d2h_hip
! and nothing of the tracer state is computed on the host: Qdp, dp3d, ps_v, Q and lnps come back from the device.
!
! stdin (list-directed, as oracle/ref/ref_harness.F90): ne qsize nsteps tstep nu_q testcase(1|2) dumpfreq  /  'outdir'  /  'vcoord dir'
!   dumpfreq >= 0: after every prim_run_subcycle_hip call (one rsplit cycle) the state, Q and lnps are downloaded and written:
!                  state_<nstep>_r<rank>.bin  in the format of oracle/pyoracle.py read_state (the derived fields, which the resident
!                                             route does not download, are written as the host holds them: zero)
!                  q_<nstep>_r<rank>.bin      istep, nelemd, qsize (int4); hyai, hybi, ps0; per element Q(:,:,:,1:qsize), lnps(:,:,n)
!   dumpfreq <  0: one prim_run_subcycle_hip call for all nsteps/rsplit cycles and one copy_state_d2h_hip (Q, no Qdp), no files:
!                  the rate of the route (hip_resident_report)
program resident_harness
  use kinds,              only : real_kind
  use dimensions_mod,     only : np, nlev, nlevp, ne, nelem, nelemd, nelemdmax, qsize, npart, nnodes, nmpi_per_node
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
  use cuda_mod,           only : cuda_mod_init, dcmip_init_hip, prim_run_subcycle_hip, copy_state_d2h_hip, hip_resident_report
  implicit none
#include <mpif.h>

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
  real(kind=real_kind) :: area(1), dt, nu_q_in
  logical :: rs_ddpdd, rs_recompute
  real(kind=real_kind) :: rs_rel
  integer :: ne_in, qsize_in, nsteps, tcase, dumpfreq, nelem_edge
  integer :: ie, j, ierr, nsub, isub, nq
  character(len=256) :: outdir, vdir
  character(len=512) :: fname

  par = initmp()
  if (par%masterproc) then
     read(*,*) ne_in, qsize_in, nsteps, dt, nu_q_in, tcase, dumpfreq
     read(*,*) outdir
     read(*,*) vdir
  endif
  call MPI_Bcast(ne_in,   1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(qsize_in,1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(nsteps,  1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(tcase,   1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(dumpfreq,1, MPI_INTEGER, 0, par%comm, ierr)
  call MPI_Bcast(dt,      1, MPI_DOUBLE_PRECISION, 0, par%comm, ierr)
  call MPI_Bcast(nu_q_in, 1, MPI_DOUBLE_PRECISION, 0, par%comm, ierr)
  call MPI_Bcast(outdir, 256, MPI_CHARACTER, 0, par%comm, ierr)
  call MPI_Bcast(vdir,   256, MPI_CHARACTER, 0, par%comm, ierr)

  ! ---- the namelist values of the DCMIP 1-x runs (test/dcmip1-1/dcmip1-1.nl and the run scripts) ----
  ne = ne_in;  qsize = qsize_in;  tstep = dt
  topology = "cube";  partmethod = SFCURVE;  npart = par%nprocs
  nmpi_per_node = 1;  nnodes = npart;  nthreads = 1
  nu = 0; nu_p = 0; nu_s = 0; nu_q = nu_q_in
  limiter_option = 8; hypervis_order = 2; hypervis_subcycle_q = 1
  hypervis_power = 0; hypervis_scaling = 0
  qsplit = 1; rsplit = 3; tstep_type = 1; integration = "explicit"
  cubed_sphere_map = 0
  if (tcase == 1) then
     test_case = "dcmip1-1"
  else
     test_case = "dcmip1-2"
  endif
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
     elem(ie)%derived%eta_dot_dpdn = 0; elem(ie)%derived%omega_p = 0
  enddo

  ! ---- prim_init2: time levels, vertical coordinate, derivative operator; then the seam ----
  call TimeLevel_init(tl)
  hybrid = hybrid_create(par, 0, 1)
  hvcoord = hvcoord_init(trim(vdir)//'/acme-72m.ascii', trim(vdir)//'/acme-72i.ascii', .false., par%masterproc, ierr)
  if (ierr /= 0) call haltmp('hvcoord_init failed')
  call derivinit(deriv)
  call cuda_mod_init(elem, hybrid, deriv, hvcoord)
  call dcmip_init_hip(elem, hvcoord, tcase)

  ! ---- prim_run: nsteps tracer steps = nsub calls of prim_run_subcycle ----
  nsub = nsteps / rsplit
  if (dumpfreq >= 0) then
     do isub = 1, nsub
        call prim_run_subcycle_hip(elem, hvcoord, tl, dt, 1)
        call copy_state_d2h_hip(elem, tl, .true., .true.)
        call TimeLevel_Qdp(tl, qsplit, nq)      ! (the levels prim_run_subcycle wrote: tl%n0 and this n0 after its closing update)
        call dump_state(tl%nstep, nq, tl%n0)
        call dump_q(tl%nstep, tl%n0)
     enddo
  else
     call prim_run_subcycle_hip(elem, hvcoord, tl, dt, nsub)
     call copy_state_d2h_hip(elem, tl, .false., .true.)
  endif
  if (par%masterproc) call hip_resident_report(tl%nstep)
  call haltmp('resident_harness done')

contains

  subroutine open_out(stem, istep)
    character(len=*), intent(in) :: stem
    integer, intent(in) :: istep
    write(fname,'(a,a,a,a,i6.6,a,i4.4,a)') trim(outdir), '/', trim(stem), '_', istep, '_r', par%rank, '.bin'
    open(unit=31, file=trim(fname), form='unformatted', access='stream', status='replace')
  end subroutine open_out

  ! the state as oracle/pyoracle.py read_state reads it
  subroutine dump_state(istep, nq, nt)
    integer, intent(in) :: istep, nq, nt
    integer :: ie
    call open_out('state', istep)
    write(31) int(istep,4), int(nq,4), int(nelemd,4), int(qsize,4)
    do ie = 1, nelemd
       write(31) elem(ie)%state%Qdp(:,:,:,1:qsize,nq)
       write(31) elem(ie)%derived%vn0, elem(ie)%derived%dp, elem(ie)%derived%divdp, elem(ie)%derived%divdp_proj, &
                 elem(ie)%derived%eta_dot_dpdn(:,:,1:nlev), elem(ie)%derived%omega_p, elem(ie)%state%dp3d(:,:,:,nt), &
                 elem(ie)%state%ps_v(:,:,nt)
    enddo
    close(31)
  end subroutine dump_state

  ! state%Q and state%lnps as copy_state_d2h_hip left them, with the vertical coordinate they were formed with
  subroutine dump_q(istep, nt)
    integer, intent(in) :: istep, nt
    integer :: ie
    call open_out('q', istep)
    write(31) int(istep,4), int(nelemd,4), int(qsize,4)
    write(31) hvcoord%hyai, hvcoord%hybi, hvcoord%ps0
    do ie = 1, nelemd
       write(31) elem(ie)%state%Q(:,:,:,1:qsize), elem(ie)%state%lnps(:,:,nt)
    enddo
    close(31)
  end subroutine dump_q

end program resident_harness
