!*************************************************************************************!
! host_sample.f90 -- a Fortran host of samplePoints, written for
! tests/test_gpu_sample_points.py: one call through the PUBLIC wrapper of lsf_hip
! (levelsetfortran_amd/fortran/lsf_hip.f90) with a mask and a second field.
!
! Reads sample_in.bin from the working directory (raw stream, written by the test):
!   6 INTEGER*4   nx, ny, nz, npts, order, iters
!   6 REAL*8      dx, xLo(3), iso, tol
!   REAL*8        phi(0:nx,0:ny,0:nz);  INTEGER*4 mask(0:nx,0:ny,0:nz);  REAL*8 q(0:nx,0:ny,0:nz)
!   REAL*8        pts(npts,3)
! and writes sample_out.bin the same way: val(npts), grad(npts,3), qval(npts),
! foot(npts,3), INTEGER*4 status(npts).  Build: make -C levelsetfortran_amd/fortran sample
! (-fdefault-real-8: REAL is REAL*8).  LSF_RESIDENT is read by the wrapper.
!*************************************************************************************!
PROGRAM host_sample

USE lsf_hip
IMPLICIT NONE

INTEGER :: nx,ny,nz,order,iters
INTEGER*4 :: npts
REAL :: dx,xLo(3),iso,tol
REAL,ALLOCATABLE,DIMENSION(:,:,:) :: phi,q
INTEGER,ALLOCATABLE,DIMENSION(:,:,:) :: mask
REAL,ALLOCATABLE,DIMENSION(:,:) :: pts,grad,foot
REAL,ALLOCATABLE,DIMENSION(:) :: val,qval
INTEGER*4,ALLOCATABLE,DIMENSION(:) :: status
INTEGER, PARAMETER :: un = 31

OPEN(UNIT=un,FILE='sample_in.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='OLD',ACTION='READ')
READ(un) nx,ny,nz,npts,order,iters
READ(un) dx,xLo,iso,tol
ALLOCATE(phi(0:nx,0:ny,0:nz),q(0:nx,0:ny,0:nz),mask(0:nx,0:ny,0:nz))
ALLOCATE(pts(npts,3),grad(npts,3),foot(npts,3),val(npts),qval(npts),status(npts))
READ(un) phi
READ(un) mask
READ(un) q
READ(un) pts
CLOSE(un)

! sentinels: every entry is written by the call
val = -7.
grad = -7.
qval = -7.
foot = -7.
status = -7

CALL samplePoints(phi,nx,ny,nz,dx,xLo,pts,npts,order,iso,iters,tol,val,grad,foot,status,mask=mask,q=q,qval=qval)

OPEN(UNIT=un,FILE='sample_out.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) val
WRITE(un) grad
WRITE(un) qval
WRITE(un) foot
WRITE(un) status
CLOSE(un)

END PROGRAM host_sample
