!*************************************************************************************!
! host_chain.f90 -- a Fortran host of the moving-geometry calls, written for
! tests/test_gpu_host_chain.py: the chain of that file through the PUBLIC wrappers of
! lsf_hip (levelsetfortran_amd/fortran/lsf_hip.f90) and nothing else.
!
!   meshDistance -> distanceFill -> narrowBand -> curvatureBand -> q = kappa ->
!   extendFieldBand -> advectFieldBand -> evolveBand -> reinitBand -> advectField ->
!   extractSurface -> stlWrite -> syncHost / syncHostInt
!
! Reads chain_in.bin from the working directory (raw stream, written by the test):
!   7 INTEGER*4   nx, ny, nz, nodes of the body, triangles of the body, steps of
!                 evolveBand, iter of reinitBand
!   8 REAL*8      dx, xLo(3), dt, width (= the band of distanceFill), h of reinitBand,
!                 the band of extendFieldBand
!   REAL*8        bodyX(nodes,3);   INTEGER*4  bodyElem(triangles,3)
!   REAL*8        u, v, w (0:nx,0:ny,0:nz)
! and writes phi.bin, phiNB.bin, phiSB.bin, kappa.bin, q.bin, surf.bin (2 INTEGER*4 counts,
! surfX, surfElem) the same way, and chain.stl.  The sentinels the arrays hold before the
! first call are those of the test.  Build: make -C levelsetfortran_amd/fortran chain
! (-fdefault-real-8: REAL is REAL*8).  LSF_RESIDENT = 0 | 1 | 2 and LSF_ARITH are read by
! the wrappers.
!*************************************************************************************!
PROGRAM host_chain

USE lsf_hip
IMPLICIT NONE

INTEGER :: nx,ny,nz,evolveSteps,reinitIter
INTEGER*4 :: nBodyNode,nBodyElem,nSurfNode,nSurfElem
REAL :: dx,xLo(3),dt,width,h,extendBand
REAL,ALLOCATABLE,DIMENSION(:,:,:) :: phi,kappa,q,u,v,w
INTEGER,ALLOCATABLE,DIMENSION(:,:,:) :: phiNB,phiSB
REAL,ALLOCATABLE,DIMENSION(:,:) :: bodyX,surfX
INTEGER*4,ALLOCATABLE,DIMENSION(:,:) :: bodyElem,surfElem
INTEGER, PARAMETER :: un = 31

OPEN(UNIT=un,FILE='chain_in.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='OLD',ACTION='READ')
READ(un) nx,ny,nz,nBodyNode,nBodyElem,evolveSteps,reinitIter
READ(un) dx,xLo,dt,width,h,extendBand
ALLOCATE(bodyX(nBodyNode,3),bodyElem(nBodyElem,3))
ALLOCATE(phi(0:nx,0:ny,0:nz),kappa(0:nx,0:ny,0:nz),q(0:nx,0:ny,0:nz))
ALLOCATE(u(0:nx,0:ny,0:nz),v(0:nx,0:ny,0:nz),w(0:nx,0:ny,0:nz))
ALLOCATE(phiNB(0:nx,0:ny,0:nz),phiSB(0:nx,0:ny,0:nz))
READ(un) bodyX
READ(un) bodyElem
READ(un) u
READ(un) v
READ(un) w
CLOSE(un)

! the sentinels of tests/test_gpu_host_chain.py
phi = 123.
phiNB = -7
phiSB = -9
kappa = -77.5
q = -55.25

CALL meshDistance(phi,nx,ny,nz,dx,xLo,bodyX,nBodyNode,bodyElem,nBodyElem,width)
CALL distanceFill(phi,nx,ny,nz,dx,width)
CALL narrowBand(nx,ny,nz,dx,phi,phiNB,phiSB)
CALL curvatureBand(phi,phiNB,kappa,nx,ny,nz,dx,1.)
q = kappa                      ! kappa has no device twin: it is home whatever LSF_RESIDENT says
CALL extendFieldBand(q,phi,phiSB,nx,ny,nz,dx,extendBand)
CALL advectFieldBand(phi,phiSB,u,v,w,nx,ny,nz,dx,dt,2)
CALL evolveBand(phi,phiSB,u,v,w,nx,ny,nz,dx,dt,evolveSteps)
CALL reinitBand(phi,phiSB,nx,ny,nz,reinitIter,dx,h)
CALL advectField(phi,u,v,w,nx,ny,nz,dx,dt,1)
CALL extractSurface(phi,nx,ny,nz,dx,xLo,0.,surfX,nSurfNode,surfElem,nSurfElem)
CALL stlWrite(surfX,nSurfNode,surfElem,'chain.stl',nSurfElem)

! the host reads phi, phiNB and phiSB itself from here on
CALL syncHost(phi)
CALL syncHostInt(phiNB)
CALL syncHostInt(phiSB)

CALL dump_real('phi.bin',phi)
CALL dump_real('kappa.bin',kappa)
CALL dump_real('q.bin',q)
CALL dump_int('phiNB.bin',phiNB)
CALL dump_int('phiSB.bin',phiSB)
OPEN(UNIT=un,FILE='surf.bin',ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) nSurfNode,nSurfElem
WRITE(un) surfX
WRITE(un) surfElem
CLOSE(un)

CONTAINS

SUBROUTINE dump_real(name,a)
CHARACTER(LEN=*), INTENT(IN) :: name
REAL, INTENT(IN) :: a(:,:,:)
OPEN(UNIT=un,FILE=name,ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) a
CLOSE(un)
END SUBROUTINE dump_real

SUBROUTINE dump_int(name,a)
CHARACTER(LEN=*), INTENT(IN) :: name
INTEGER, INTENT(IN) :: a(:,:,:)
OPEN(UNIT=un,FILE=name,ACCESS='STREAM',FORM='UNFORMATTED',STATUS='REPLACE',ACTION='WRITE')
WRITE(un) a
CLOSE(un)
END SUBROUTINE dump_int

END PROGRAM host_chain
