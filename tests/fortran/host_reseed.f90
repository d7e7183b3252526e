!*************************************************************************************!
! host_reseed.f90 -- a Fortran host of reseedPoints and reseedGet, written for
! tests/test_gpu_reseed_fortran.py: a reseed from scratch, then a top-up of old markers
! under a mask, through the PUBLIC wrappers of lsf_hip
! (levelsetfortran_amd/fortran/lsf_hip.f90).
!
! Reads reseed_in.bin from the working directory (raw stream, written by the test):
!   7 INTEGER*4   nx, ny, nz, npts, per_cell, order, iters
!   8 REAL*8      dx, xLo(3), rmin, rmax, band, tol
!   1 INTEGER*8   seed
!   REAL*8        phi(0:nx,0:ny,0:nz);  INTEGER*4 mask(0:nx,0:ny,0:nz)
!   REAL*8        pts(npts,3), rad(npts)
! Writes reseed_out.bin the same way: INTEGER*4 n0, pts0(n0,3), rad0(n0), INTEGER*4 src0(n0)
! (from scratch, no mask), then INTEGER*4 n1, status(npts), pts1(n1,3), rad1(n1), src1(n1)
! (the top-up of pts, rad under the mask).
! Build: make -C levelsetfortran_amd/fortran reseed (-fdefault-real-8: REAL is REAL*8).
! LSF_RESIDENT is read by the wrapper.
!*************************************************************************************!
PROGRAM host_reseed

USE lsf_hip
USE iso_c_binding, ONLY: c_int64_t
IMPLICIT NONE

INTEGER :: nx,ny,nz,per_cell,order,iters
INTEGER*4 :: npts,n0,n1,none
REAL :: dx,xLo(3),rmin,rmax,band,tol
INTEGER(c_int64_t) :: seed
REAL,ALLOCATABLE,DIMENSION(:,:,:) :: phi
INTEGER,ALLOCATABLE,DIMENSION(:,:,:) :: mask
REAL,ALLOCATABLE,DIMENSION(:,:) :: pts,pts0,pts1,nopts
REAL,ALLOCATABLE,DIMENSION(:) :: rad,rad0,rad1,norad
INTEGER*4,ALLOCATABLE,DIMENSION(:) :: status,src0,src1,nostatus
INTEGER, PARAMETER :: un = 31

OPEN(UNIT=un,FILE='reseed_in.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='OLD',ACTION='READ')
READ(un) nx,ny,nz,npts,per_cell,order,iters
READ(un) dx,xLo,rmin,rmax,band,tol
READ(un) seed
ALLOCATE(phi(0:nx,0:ny,0:nz),mask(0:nx,0:ny,0:nz),pts(npts,3),rad(npts),status(npts))
READ(un) phi
READ(un) mask
READ(un) pts
READ(un) rad
CLOSE(un)

! from scratch: no old markers, no mask
none = 0
ALLOCATE(nopts(0,3),norad(0),nostatus(0))
CALL reseedPoints(phi,nx,ny,nz,dx,xLo,nopts,norad,none,per_cell,rmin,rmax,band,order,iters,tol,seed,nostatus,n0)
ALLOCATE(pts0(n0,3),rad0(n0),src0(n0))
pts0 = -7.
rad0 = -7.
src0 = -7
CALL reseedGet(pts0,rad0,src0,n0)

! the top-up of the old markers under the mask
status = -7
CALL reseedPoints(phi,nx,ny,nz,dx,xLo,pts,rad,npts,per_cell,rmin,rmax,band,order,iters,tol,seed,status,n1,mask=mask)
ALLOCATE(pts1(n1,3),rad1(n1),src1(n1))
pts1 = -7.
rad1 = -7.
src1 = -7
CALL reseedGet(pts1,rad1,src1,n1)

OPEN(UNIT=un,FILE='reseed_out.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) n0
WRITE(un) pts0
WRITE(un) rad0
WRITE(un) src0
WRITE(un) n1
WRITE(un) status
WRITE(un) pts1
WRITE(un) rad1
WRITE(un) src1
CLOSE(un)

END PROGRAM host_reseed
