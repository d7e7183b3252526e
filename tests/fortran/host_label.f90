!*************************************************************************************!
! host_label.f90 -- a Fortran host of labelBand, written for
! tests/test_gpu_label_band.py: the PUBLIC wrapper of lsf_hip
! (levelsetfortran_amd/fortran/lsf_hip.f90) and nothing else.
!
! Reads label_in.bin from the working directory (raw stream, written by the test):
!   4 INTEGER*4   nx, ny, nz, side
!   1 REAL*8      iso
!   REAL*8        phi(0:nx,0:ny,0:nz);   INTEGER*4  mask(0:nx,0:ny,0:nz)
!   INTEGER*4     label(0:nx,0:ny,0:nz), what the caller hands in
! calls narrowBand on a copy of phi first, so that under LSF_RESIDENT = 1 | 2 the twins of
! phi, phiNB and phiSB belong to OTHER arrays when labelBand takes them over, then
! labelBand(phi,mask,label,...), and writes label.bin (label), ncomp.bin (1 INTEGER*4),
! phi.bin and mask.bin (both as they are after the call: read, never written) the same
! way.  Build: make -C levelsetfortran_amd/fortran label (-fdefault-real-8: REAL is
! REAL*8).  LSF_RESIDENT = 0 | 1 | 2 is read by the wrappers.
!*************************************************************************************!
PROGRAM host_label

USE lsf_hip
IMPLICIT NONE

INTEGER :: nx,ny,nz,side,nComp
REAL :: iso,dx
REAL,ALLOCATABLE,DIMENSION(:,:,:) :: phi,other
INTEGER,ALLOCATABLE,DIMENSION(:,:,:) :: mask,label,otherNB,otherSB
INTEGER, PARAMETER :: un = 31

OPEN(UNIT=un,FILE='label_in.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='OLD',ACTION='READ')
READ(un) nx,ny,nz,side
READ(un) iso
ALLOCATE(phi(0:nx,0:ny,0:nz),other(0:nx,0:ny,0:nz))
ALLOCATE(mask(0:nx,0:ny,0:nz),label(0:nx,0:ny,0:nz),otherNB(0:nx,0:ny,0:nz),otherSB(0:nx,0:ny,0:nz))
READ(un) phi
READ(un) mask
READ(un) label
CLOSE(un)

dx = 3./nx
other = phi + 0.5
otherNB = 0
otherSB = 0
CALL narrowBand(nx,ny,nz,dx,other,otherNB,otherSB)
CALL labelBand(phi,mask,label,nx,ny,nz,iso,side,nComp)
CALL syncHost(other)
CALL syncHostInt(otherNB)
CALL syncHostInt(otherSB)

CALL dump_int('label.bin',label)
CALL dump_int('mask.bin',mask)
OPEN(UNIT=un,FILE='ncomp.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) nComp
CLOSE(un)
OPEN(UNIT=un,FILE='phi.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) phi
CLOSE(un)

CONTAINS

SUBROUTINE dump_int(name,a)
CHARACTER(LEN=*), INTENT(IN) :: name
INTEGER, INTENT(IN) :: a(:,:,:)
OPEN(UNIT=un,FILE=name,ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) a
CLOSE(un)
END SUBROUTINE dump_int

END PROGRAM host_label
