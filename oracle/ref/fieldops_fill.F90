! fieldops_fill.F90 -- TEST INFRASTRUCTURE.  The inputs of the field-operator fixture (tests/golden/ref_ne2_fieldops.npz) and of every
! Fortran host that has to work on the same numbers (oracle/ref/ref_harness.F90: dump_fieldops; tests/fortran_resident/views_harness.F90).
!
! The fill of an element depends on its global number alone, so that any partition over ranks fills the same global field.  The
! generator is ref_harness's lcg; two draws make one value, so that the noise reaches the last bit of the mantissa.
module fieldops_fill
  implicit none
  private
  integer, parameter, public :: fo_nk = 3                       ! levels of the fixture
  integer(kind=8), parameter, public :: fo_seed = 918273_8      ! a seed of its own (dump_ops starts from 12345)
  public :: fo_lcg, fo_fill
contains

  function fo_lcg(seed) result(x)
    integer(kind=8), intent(inout) :: seed
    real(kind=8) :: x
    seed = mod(seed*1103515245_8 + 12345_8, 2147483648_8)
    x = dble(seed)/2147483648.0d0
  end function fo_lcg

  ! s(n,n,nk): a scalar of order 300, every value in [150, 450); v(n,n,2,nk): a wind centred on 0, every component in [-30, 30)
  subroutine fo_fill(gid, n, nk, s, v)
    integer, intent(in) :: gid, n, nk
    real(kind=8), intent(out) :: s(n,n,nk), v(n,n,2,nk)
    integer(kind=8) :: seed
    integer :: i, j, k, c
    real(kind=8) :: x
    seed = fo_seed + 7919_8*int(gid,8)
    do i = 1, 8                                  ! neighbouring seeds start close together: run them apart
       x = fo_lcg(seed)
    enddo
    do k = 1, nk; do j = 1, n; do i = 1, n
       x = fo_lcg(seed); x = x + fo_lcg(seed)/2147483648.0d0
       s(i,j,k) = 300.0d0*(0.5d0 + x)
       do c = 1, 2
          x = fo_lcg(seed); x = x + fo_lcg(seed)/2147483648.0d0
          v(i,j,c,k) = 60.0d0*(x - 0.5d0)
       enddo
    enddo; enddo; enddo
  end subroutine fo_fill

end module fieldops_fill
