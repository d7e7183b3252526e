!*************************************************************************************!
! host_particles.f90 -- a Fortran host of advectPoints and correctField, written for
! tests/test_gpu_correct_field.py: one call of each through the PUBLIC wrappers of lsf_hip
! (levelsetfortran_amd/fortran/lsf_hip.f90) on one set of inputs, with both groups of
! fields and a mask.
!
! Reads particles_in.bin from the working directory (raw stream, written by the test):
!   7 INTEGER*4   nx, ny, nz, npts, order, scheme, nsteps
!   6 REAL*8      dx, xLo(3), dt, slack
!   REAL*8        phi, u, v, w, speed (0:nx,0:ny,0:nz each);  INTEGER*4 mask(0:nx,0:ny,0:nz)
!   REAL*8        pts(npts,3), rad(npts)
! The markers pts are corrected against phi first (correctField), then moved
! (advectPoints, through the corrected phi).  Writes particles_out.bin the same way:
! phi, INTEGER*4 cstatus(npts), change, pts(npts,3), INTEGER*4 astatus(npts), cfl.
! Build: make -C levelsetfortran_amd/fortran particles (-fdefault-real-8: REAL is REAL*8).
! LSF_RESIDENT is read by the wrapper.
!*************************************************************************************!
PROGRAM host_particles

USE lsf_hip
IMPLICIT NONE

INTEGER :: nx,ny,nz,order,scheme,nsteps
INTEGER*4 :: npts
REAL :: dx,xLo(3),dt,slack,change,cfl
REAL,ALLOCATABLE,DIMENSION(:,:,:) :: phi,u,v,w,speed
INTEGER,ALLOCATABLE,DIMENSION(:,:,:) :: mask
REAL,ALLOCATABLE,DIMENSION(:,:) :: pts
REAL,ALLOCATABLE,DIMENSION(:) :: rad
INTEGER*4,ALLOCATABLE,DIMENSION(:) :: cstatus,astatus
INTEGER, PARAMETER :: un = 31

OPEN(UNIT=un,FILE='particles_in.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='OLD',ACTION='READ')
READ(un) nx,ny,nz,npts,order,scheme,nsteps
READ(un) dx,xLo,dt,slack
ALLOCATE(phi(0:nx,0:ny,0:nz),u(0:nx,0:ny,0:nz),v(0:nx,0:ny,0:nz),w(0:nx,0:ny,0:nz),speed(0:nx,0:ny,0:nz),mask(0:nx,0:ny,0:nz))
ALLOCATE(pts(npts,3),rad(npts),cstatus(npts),astatus(npts))
READ(un) phi
READ(un) u
READ(un) v
READ(un) w
READ(un) speed
READ(un) mask
READ(un) pts
READ(un) rad
CLOSE(un)

! sentinels: every entry is written by the calls
cstatus = -7
astatus = -7
change = -7.
cfl = -7.

CALL correctField(phi,nx,ny,nz,dx,xLo,pts,rad,npts,slack,cstatus,change,mask=mask)
CALL advectPoints(pts,npts,nx,ny,nz,dx,xLo,order,scheme,dt,nsteps,astatus,cfl,u=u,v=v,w=w,phi=phi,speed=speed,mask=mask)
! under LSF_RESIDENT=2 the corrected phi lives on the device until the host asks for it
CALL syncHost(phi)

OPEN(UNIT=un,FILE='particles_out.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) phi
WRITE(un) cstatus
WRITE(un) change
WRITE(un) pts
WRITE(un) astatus
WRITE(un) cfl
CLOSE(un)

END PROGRAM host_particles
