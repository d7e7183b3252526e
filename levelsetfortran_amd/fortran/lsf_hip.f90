!*************************************************************************************!
! lsf_hip.f90 -- iso_c_binding shim between the reference's Fortran host (set3d.f90) and
! liblsf_hip.so (include/lsf.h).
!
! It gives the host back the procedures of the hot path UNDER THEIR ORIGINAL NAMES AND
! ARGUMENT LISTS, so that the main program calls them exactly as before:
!
!   reinit(phi,gradPhi,gradPhiMag,nx,ny,nz,iter,dx,h)   replaces subs.f90:717-931
!   narrowBand(nx,ny,nz,dx,phi,phiNB,phiSB)             replaces subs.f90:178-207
!   minmaxFlow(phi,phiNB,phiSB,nx,ny,nz,iter,dx,h1)     replaces the loop set3d.f90:394-462
!   phi0Init(phi,nx,ny,nz,dx,xLo,xMin,xMax,surfX,nSurfNode,surfElem,nSurfElem)
!                                                        replaces the loop set3d.f90:218-268
!   advectNodes(phi,phiSB,nx,ny,nz,dx,xLo,surfXX,nSurfNode,iter)
!                                                        replaces set3d.f90:470-479 and :487-501
!   reinitBand(phi,mask,nx,ny,nz,iter,dx,h)             no reference counterpart: reinit on the cells
!                                                        with mask == 1 only (include/lsf.h: lsf_reinit_band)
!   meshDistance(phi,nx,ny,nz,dx,xLo,surfX,nSurfNode,surfElem,nSurfElem,width)
!                                                        no reference counterpart: exact signed distance from the
!                                                        triangles, clamped at width*dx (include/lsf.h: lsf_mesh_distance)
!   distanceFill(phi,nx,ny,nz,dx,band)                   no reference counterpart: first-order distance on every point with
!                                                        |phi| >= band*dx by fast sweeping (include/lsf.h: lsf_distance_fill)
!   extendField(q,phi,nx,ny,nz,dx,band)                  no reference counterpart: q carried off the points with |phi| < band*dx
!                                                        constant along the normals of phi (include/lsf.h: lsf_extend_field)
!   advectField(phi,u,v,w,nx,ny,nz,dx,dt,steps)          no reference counterpart: transport of phi by the velocity field
!                                                        (u,v,w), WENO5 / TVD-RK3 (include/lsf.h: lsf_advect_field)
!   advectFieldBand(phi,mask,u,v,w,nx,ny,nz,dx,dt,steps) no reference counterpart: advectField on the cells with mask == 1
!                                                        only (include/lsf.h: lsf_advect_field_band)
!   evolveBand(phi,mask,u,v,w,nx,ny,nz,dx,dt,steps)      no reference counterpart: the band time loop -- transport, two sweeps of
!                                                        the reinitialisation and the list following the surface; phi and mask
!                                                        are both updated (include/lsf.h: lsf_evolve_band)
!   evolveBandCurv(phi,mask,speed,nx,ny,nz,dx,dt,steps,b) no reference counterpart: evolveBand for the speed law F = speed - b*kappa,
!                                                        the curvature term differenced centrally inside the stages
!                                                        (include/lsf.h: lsf_evolve_band_curv)
!   curvatureBand(phi,mask,kappa,nx,ny,nz,dx,clamp)      the reference's own is commented out (subs.f90:426-448): the mean
!                                                        curvature div(grad(phi)/|grad(phi)|) on the cells with mask == 1
!                                                        only (include/lsf.h: lsf_curvature_band)
!   measureBand(phi,mask,nx,ny,nz,dx,xLo,iso,M)          no reference counterpart: area, enclosed volume, their first moments
!                                                        and the surface's, summed over the cells with mask == 1 only
!                                                        (include/lsf.h: lsf_measure_band)
!   cutCellsBand(phi,mask,nx,ny,nz,dx,iso,vof,ax,ay,az,volume)  no reference counterpart: the volume fraction inside phi < iso and
!                                                        the apertures of the lower faces of the cells with mask == 1, and
!                                                        the body's volume (include/lsf.h: lsf_cut_cells_band)
!   samplePoints(phi,nx,ny,nz,dx,xLo,pts,npts,order,     no reference counterpart: phi, its gradient and the foot point on
!                iso,iters,tol,val,grad,foot,status      phi = iso at arbitrary points, trilinear or Catmull-Rom; optionally a
!                [,mask,q,qval])                         second field q and a band mask (include/lsf.h: lsf_sample_points)
!   castRays(phi,nx,ny,nz,dx,xLo,org,dir,nrays,order,    no reference counterpart: the first hit of each ray with phi = iso,
!            iso,tmin,tmax,safety,smin,smax,skip,        marching by the field's own value and skipping what a band mask does
!            refine,max_steps,thit,hit,grad,status       not hold; optionally a second field q sampled at the hit
!            [,mask,q,qval])                             (include/lsf.h: lsf_cast_rays)
!   advectPoints(pts,npts,nx,ny,nz,dx,xLo,order,scheme,  no reference counterpart: points carried through the fields that move
!                dt,nsteps,status,cfl                    phi, x' = (u,v,w) + speed grad phi / |grad phi|, by TVD-RK3 or Euler over
!                [,u,v,w,phi,speed,mask])                the interpolant of samplePoints (include/lsf.h: lsf_advect_points)
!   correctField(phi,nx,ny,nz,dx,xLo,pts,rad,npts,       no reference counterpart: the correction of the particle level set, phi
!                slack,status,change[,mask])             rebuilt around escaped markers (include/lsf.h: lsf_correct_field)
!   reseedPoints(phi,nx,ny,nz,dx,xLo,pts,rad,npts,per_cell,rmin,rmax,band,order,iters,tol,seed,status,nout[,mask])
!   reseedGet(pts_out,rad_out,src_out,nout)              no reference counterpart: the marker population kept, dropped, re-radiused
!                                                        and topped up on the device (include/lsf.h: lsf_reseed_points)
!   labelBand(phi,mask,label,nx,ny,nz,iso,side,ncomp)    no reference counterpart: the connected components of the cells with
!                                                        mask == 1 on either side of phi = iso (include/lsf.h: lsf_label_band)
!   extendFieldBand(q,phi,mask,nx,ny,nz,dx,band)         no reference counterpart: extendField on the cells with mask == 1
!                                                        only, by Jacobi passes over the list: q carried off the list cells
!                                                        with |phi| < band*dx (include/lsf.h: lsf_extend_field_band)
!   redistanceBand(phi,mask,nx,ny,nz,dx,near)            no reference counterpart: the distance property restored on the cells
!                                                        with mask == 1 from closest points, without pseudo-time sweeps
!                                                        (include/lsf_redistance.h: lsf_redistance_band)
!   extractSurface(phi,nx,ny,nz,dx,xLo,iso,surfX,nSurfNode,surfElem,nSurfElem)
!                                                        no reference counterpart: the level set phi = iso as a triangle mesh,
!                                                        marching tetrahedra (include/lsf.h: lsf_extract_surface)
!   stlWrite(surfX,nSurfNode,surfElem,filename,nSurfElem) no reference counterpart: binary STL of a mesh (lsf_stl_write)
!   stlRead(surfX,nSurfNode,surfElem,filename,nSurfElem,surfElemTag,surfOrder,nBndComp,nBndElem,bndNormal)
!                                                        replaces subs.f90:17-121 (same list)
!
! and reproduces what the reference prints around them (subs.f90:916,923,929 and
! set3d.f90:449,456,463) and its STOP on a NaN residual (subs.f90:926, set3d.f90:458).
!
! Build with the reference's own flags (-fdefault-real-8, Makefile:4): REAL below is
! then REAL(8) = C double, INTEGER is C int.  INTEGRATION.md shows the two edits to the
! host that bring this module in; levelsetfortran_amd/fortran/Makefile applies them to
! /root/reference/set3d.f90 at build time without copying it into this repository.
!
! Run parameters.  The reference hard-codes them (set3d.f90:140,148,298,390,576) and its
! README announces a namelist ("Working on adding a namelist for inputs", README.md:11);
! this module reads one:
!
!   ./set3d_hip.exec surface.stl [inputs.nml]      (default: ./lsf.nml if it exists)
!
!   &lsf_inputs
!     dx = 0.0234375            ! grid spacing                         (set3d.f90:140)
!     dd = 10                   ! pad cells on every side              (set3d.f90:148)
!     dd_lo = 10, 234, 234      ! pad cells per axis, low / high side  (cubic grids from
!     dd_hi = 10, 235, 235      !   non-cubic bounding boxes)
!     reinit_iter = 10000       ! cap of reinit #1                     (set3d.f90:298)
!     minmax_iter = 200         ! cap of the min/max flow              (set3d.f90:390)
!     reinit2_iter = 2000       ! cap of reinit #2                     (set3d.f90:576)
!     order = 'gs'              ! 'gs' (the reference's raster order, exact) | 'jacobi'
!     arith = 'strict'          ! 'strict' (default: every operation as subs.f90 writes it, the reference's bits) |
!                               ! 'fast' (same mathematics restructured for the GPU, 2 x faster, ~1e-16 per sweep away;
!                               !   see DESIGN.md section 2 for what that becomes over thousands of sweeps)
!     devices = 0, 1, 2, 3      ! reinit runs on these GPUs (lsf_reinit_multi; a device may be listed more than once):
!                               !   order = 'jacobi': block-decomposed, one block each; order = 'gs': ONE GPU -- the process'
!                               !   current device, where the other seams keep their arrays, not the first listed --
!                               !   unless `slabs = 1`; unset: one GPU
!     slabs = 0                 ! 1: with order = 'gs', the reference's ordering over one z slab per listed device, the
!                               !   field of one GPU bit for bit (lsf_reinit_multi with LSF_ORDER_GS).  Opt-in: the path
!                               !   has not run on two real devices yet; on first use every pair of neighbouring devices
!                               !   runs lsf_peer_selftest, and a violated assumption ends the run with its name
!     transport = 'peer'        ! how the blocks exchange their 3-cell halos: 'peer' (peer copies, default) | 'rccl'
!                               !   (ncclSend / ncclRecv over xGMI; needs a distinct device per block)
!     check_every = 8           ! sweeps between two looks of the host at the RMS of a block-decomposed run (1..64;
!                               !   the stop sweep, the field and the printed residuals do not depend on it)
!     redist_iters = 8          ! redistanceBand: Newton steps of the foot iteration at most,
!     redist_tol = 1e-9         !   its tolerance |phi(foot)| <= tol*dx,
!     redist_passes = 64        !   and the cap of the Jacobi passes of its fill (include/lsf_redistance.h)
!     resident = 2              ! 0: every seam copies its arrays in and out (default of the C ABI)
!                               ! 1: skip the host-to-device copy of an array the last seam left on the device
!                               ! 2: (default here) ... and leave results on the device until the host needs them:
!                               !    phi, phiNB, phiSB cross PCIe once (lsf_mirror, include/lsf.h)
!   /
!
! Every entry is optional; environment variables of the same meaning (LSF_DX, LSF_DD,
! LSF_DD_{X,Y,Z}_{LO,HI}, LSF_REINIT_ITER, LSF_MINMAX_ITER, LSF_REINIT2_ITER, LSF_ORDER,
! LSF_ARITH, LSF_RESIDENT, LSF_DEVICES="0,1,2,3", LSF_SLABS, LSF_MULTI_TRANSPORT, LSF_MULTI_CHECK_EVERY) override the namelist.
!*************************************************************************************!
MODULE lsf_hip

USE, INTRINSIC :: iso_c_binding
IMPLICIT NONE
PRIVATE
PUBLIC :: reinit, narrowBand, minmaxFlow, phi0Init, advectNodes, lsf_env_real, lsf_env_int, lsf_pad_cells
PUBLIC :: reinitBand
PUBLIC :: meshDistance
PUBLIC :: distanceFill
PUBLIC :: extendField
PUBLIC :: advectField
PUBLIC :: advectFieldBand
PUBLIC :: evolveBand
PUBLIC :: evolveBandCurv
PUBLIC :: curvatureBand
PUBLIC :: measureBand
PUBLIC :: cutCellsBand
PUBLIC :: samplePoints
PUBLIC :: castRays
PUBLIC :: advectPoints
PUBLIC :: correctField
PUBLIC :: reseedPoints
PUBLIC :: reseedGet
PUBLIC :: labelBand
PUBLIC :: extendFieldBand
PUBLIC :: redistanceBand
PUBLIC :: extractSurface, stlWrite
PUBLIC :: writeVti, snapshotPhi, sumSqDiff, syncHost, syncHostInt, forgetHost, stlRead

INTEGER(c_int), PARAMETER :: LSF_OK = 0, LSF_ERR_NAN = 1
INTEGER(c_int), PARAMETER :: LSF_ORDER_JACOBI = 1, LSF_ARITH_STRICT = 256

! the namelist (read once; unset entries keep these sentinels)
LOGICAL, SAVE :: nml_loaded = .FALSE.
REAL, SAVE :: nml_dx = -1.
INTEGER, SAVE :: nml_dd = -1, nml_dd_lo(3) = -1, nml_dd_hi(3) = -1
INTEGER, SAVE :: nml_reinit_iter = -1, nml_minmax_iter = -1, nml_reinit2_iter = -1
CHARACTER(LEN=16), SAVE :: nml_order = ' ', nml_arith = ' ', nml_transport = ' '
INTEGER, SAVE :: nml_check_every = 8
INTEGER, SAVE :: nml_resident = -1, nml_slabs = 0
INTEGER, SAVE :: nml_redist_iters = 8, nml_redist_passes = 64
REAL, SAVE :: nml_redist_tol = 1.0e-9
INTEGER(c_int), SAVE :: nml_devices(16) = -1
LOGICAL, SAVE :: mirror_set = .FALSE.

INTERFACE
   ! int lsf_reinit(double*,int,int,int,int,double,double,double,int,int*,double*,int)
   FUNCTION lsf_reinit(phi,nx,ny,nz,iter,dx,h,tol,mode,sweeps_done,rms_trace,trace_cap) &
            BIND(C,NAME='lsf_reinit') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,iter,mode,trace_cap
      REAL(c_double), VALUE :: dx,h,tol
      INTEGER(c_int), INTENT(OUT) :: sweeps_done
      REAL(c_double), INTENT(OUT) :: rms_trace(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_reinit
   ! int lsf_reinit_band(double*,const int32_t*,int,int,int,int,double,double,double,int,int*,double*,int)
   FUNCTION lsf_reinit_band(phi,mask,nx,ny,nz,iter,dx,h,tol,mode,sweeps_done,rms_trace,trace_cap) &
            BIND(C,NAME='lsf_reinit_band') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,iter,mode,trace_cap
      REAL(c_double), VALUE :: dx,h,tol
      INTEGER(c_int), INTENT(OUT) :: sweeps_done
      REAL(c_double), INTENT(OUT) :: rms_trace(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_reinit_band
   ! int lsf_reinit_multi(double*,int,int,int,int,double,double,double,int,const int*,int,const int[3],int*,double*,int)
   FUNCTION lsf_reinit_multi(phi,nx,ny,nz,iter,dx,h,tol,mode,devices,ndev,dims,sweeps_done,rms_trace,trace_cap) &
            BIND(C,NAME='lsf_reinit_multi') RESULT(rc)
      IMPORT :: c_int, c_double, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,iter,mode,ndev,trace_cap
      REAL(c_double), VALUE :: dx,h,tol
      INTEGER(c_int), INTENT(IN) :: devices(*)
      TYPE(c_ptr), VALUE :: dims            ! NULL: the library's default decomposition
      INTEGER(c_int), INTENT(OUT) :: sweeps_done
      REAL(c_double), INTENT(OUT) :: rms_trace(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_reinit_multi
   ! int lsf_multi_defaults(int check_every, int transport)   transport: 0 peer copies, 1 RCCL
   FUNCTION lsf_multi_defaults(check_every,transport) BIND(C,NAME='lsf_multi_defaults') RESULT(rc)
      IMPORT :: c_int
      INTEGER(c_int), VALUE :: check_every,transport
      INTEGER(c_int) :: rc
   END FUNCTION lsf_multi_defaults
   FUNCTION lsf_minmax(phi,phiNB,phiSB,nx,ny,nz,iter,dx,h1,tol,mode,iters_done,rms_trace,trace_cap) &
            BIND(C,NAME='lsf_minmax') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), INTENT(INOUT) :: phiNB(*),phiSB(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,iter,mode,trace_cap
      REAL(c_double), VALUE :: dx,h1,tol
      INTEGER(c_int), INTENT(OUT) :: iters_done
      REAL(c_double), INTENT(OUT) :: rms_trace(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_minmax
   FUNCTION lsf_narrowband(phi,phiNB,phiSB,nx,ny,nz,dx) BIND(C,NAME='lsf_narrowband') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(IN) :: phi(*)
      INTEGER(c_int), INTENT(INOUT) :: phiNB(*),phiSB(*)
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), VALUE :: dx
      INTEGER(c_int) :: rc
   END FUNCTION lsf_narrowband
   FUNCTION lsf_phi0(phi,nx,ny,nz,dx,xLo,xMin,xMax,surfX,nSurfNode,surfElem,nSurfElem) &
            BIND(C,NAME='lsf_phi0') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,nSurfNode,nSurfElem
      REAL(c_double), VALUE :: dx
      REAL(c_double), INTENT(IN) :: xLo(3),xMin(3),xMax(3),surfX(*)
      INTEGER(c_int), INTENT(IN) :: surfElem(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_phi0
   ! int lsf_mesh_distance(double*,int,int,int,double,const double[3],const double*,int,const int32_t*,int,double,int,int64_t[4])
   FUNCTION lsf_mesh_distance(phi,nx,ny,nz,dx,xLo,surfX,nSurfNode,surfElem,nSurfElem,width,flags,info) &
            BIND(C,NAME='lsf_mesh_distance') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,nSurfNode,nSurfElem,flags
      REAL(c_double), VALUE :: dx,width
      REAL(c_double), INTENT(IN) :: xLo(3),surfX(*)
      INTEGER(c_int), INTENT(IN) :: surfElem(*)
      INTEGER(c_int64_t), INTENT(OUT) :: info(4)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_mesh_distance
   ! int lsf_distance_fill(double*,const int32_t*,int,int,int,double,double,int,int*,int64_t*,int,int64_t*)
   FUNCTION lsf_distance_fill(phi,mask,nx,ny,nz,dx,band,max_rounds,rounds_done,changed_trace,trace_cap,frozen_points) &
            BIND(C,NAME='lsf_distance_fill') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      TYPE(c_ptr), VALUE :: mask             ! NULL: the frozen set is |phi| < band*dx
      INTEGER(c_int), VALUE :: nx,ny,nz,max_rounds,trace_cap
      REAL(c_double), VALUE :: dx,band
      INTEGER(c_int), INTENT(OUT) :: rounds_done
      INTEGER(c_int64_t), INTENT(OUT) :: changed_trace(*),frozen_points
      INTEGER(c_int) :: rc
   END FUNCTION lsf_distance_fill
   ! int lsf_extend_field(double*,const double*,const int32_t*,int,int,int,double,double,int,int*,int64_t*,int,int64_t[3])
   FUNCTION lsf_extend_field(q,phi,mask,nx,ny,nz,dx,band,max_rounds,rounds_done,changed_trace,trace_cap,info) &
            BIND(C,NAME='lsf_extend_field') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: q(*)
      REAL(c_double), INTENT(IN) :: phi(*)
      TYPE(c_ptr), VALUE :: mask             ! NULL: the frozen set is |phi| < band*dx
      INTEGER(c_int), VALUE :: nx,ny,nz,max_rounds,trace_cap
      REAL(c_double), VALUE :: dx,band
      INTEGER(c_int), INTENT(OUT) :: rounds_done
      INTEGER(c_int64_t), INTENT(OUT) :: changed_trace(*),info(3)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_extend_field
   ! int lsf_advect_field(double*,const double*,const double*,const double*,const double*,int,int,int,double,double,int,int,int,
   !                      int*,double*,double*,int)
   FUNCTION lsf_advect_field(phi,u,v,w,speed,nx,ny,nz,dx,dt,steps,scheme,mode,steps_done,cfl,change_trace,trace_cap) &
            BIND(C,NAME='lsf_advect_field') RESULT(rc)
      IMPORT :: c_int, c_double, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      REAL(c_double), INTENT(IN) :: u(*),v(*),w(*)
      TYPE(c_ptr), VALUE :: speed            ! NULL: no motion along the normal
      INTEGER(c_int), VALUE :: nx,ny,nz,steps,scheme,mode,trace_cap
      REAL(c_double), VALUE :: dx,dt
      INTEGER(c_int), INTENT(OUT) :: steps_done
      REAL(c_double), INTENT(OUT) :: cfl
      REAL(c_double), INTENT(OUT) :: change_trace(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_advect_field
   ! int lsf_advect_field_band(double*,const int32_t*,const double*,const double*,const double*,const double*,int,int,int,double,double,
   !                           int,int,int,int*,double*,double*,int,int64_t[3],double*)
   FUNCTION lsf_advect_field_band(phi,mask,u,v,w,speed,nx,ny,nz,dx,dt,steps,scheme,mode,steps_done,cfl,change_trace,trace_cap, &
                                  info,margin) BIND(C,NAME='lsf_advect_field_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      REAL(c_double), INTENT(IN) :: u(*),v(*),w(*)
      TYPE(c_ptr), VALUE :: speed            ! NULL: no motion along the normal
      INTEGER(c_int), VALUE :: nx,ny,nz,steps,scheme,mode,trace_cap
      REAL(c_double), VALUE :: dx,dt
      INTEGER(c_int), INTENT(OUT) :: steps_done
      REAL(c_double), INTENT(OUT) :: cfl
      REAL(c_double), INTENT(OUT) :: change_trace(*)
      INTEGER(c_int64_t), INTENT(OUT) :: info(3)
      REAL(c_double), INTENT(OUT) :: margin
      INTEGER(c_int) :: rc
   END FUNCTION lsf_advect_field_band
   ! int lsf_evolve_band(double*,int32_t*,const double*,const double*,const double*,const double*,int,int,int,double,double,int,int,int,
   !                     double,int,int,double,int,int*,double*,double*,int,int64_t[6],double*)
   FUNCTION lsf_evolve_band(phi,mask,u,v,w,speed,nx,ny,nz,dx,dt,steps,scheme,mode,core,ring,reinit_sweeps,h,check_every, &
                            steps_done,cfl,change_trace,trace_cap,info,margin) BIND(C,NAME='lsf_evolve_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), INTENT(INOUT) :: mask(*)
      REAL(c_double), INTENT(IN) :: u(*),v(*),w(*)
      TYPE(c_ptr), VALUE :: speed            ! NULL: no motion along the normal
      INTEGER(c_int), VALUE :: nx,ny,nz,steps,scheme,mode,ring,reinit_sweeps,check_every,trace_cap
      REAL(c_double), VALUE :: dx,dt,core,h
      INTEGER(c_int), INTENT(OUT) :: steps_done
      REAL(c_double), INTENT(OUT) :: cfl
      REAL(c_double), INTENT(OUT) :: change_trace(*)
      INTEGER(c_int64_t), INTENT(OUT) :: info(6)
      REAL(c_double), INTENT(OUT) :: margin
      INTEGER(c_int) :: rc
   END FUNCTION lsf_evolve_band
   ! int lsf_evolve_band_curv(double*,int32_t*,const double*,const double*,const double*,const double*,int,int,int,double,double,int,int,
   !                          int,double,int,int,double,int,double,double,int*,double*,double*,double*,int,int64_t[6],double*)
   FUNCTION lsf_evolve_band_curv(phi,mask,u,v,w,speed,nx,ny,nz,dx,dt,steps,scheme,mode,core,ring,reinit_sweeps,h,check_every, &
                                 bcurv,clamp,steps_done,cfl,diffusion,change_trace,trace_cap,info,margin) &
            BIND(C,NAME='lsf_evolve_band_curv') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), INTENT(INOUT) :: mask(*)
      TYPE(c_ptr), VALUE :: u,v,w            ! NULL: no velocity
      REAL(c_double), INTENT(IN) :: speed(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,steps,scheme,mode,ring,reinit_sweeps,check_every,trace_cap
      REAL(c_double), VALUE :: dx,dt,core,h,bcurv,clamp
      INTEGER(c_int), INTENT(OUT) :: steps_done
      REAL(c_double), INTENT(OUT) :: cfl,diffusion
      REAL(c_double), INTENT(OUT) :: change_trace(*)
      INTEGER(c_int64_t), INTENT(OUT) :: info(6)
      REAL(c_double), INTENT(OUT) :: margin
      INTEGER(c_int) :: rc
   END FUNCTION lsf_evolve_band_curv
   ! int lsf_curvature_band(const double*,const int32_t*,double*,double*,double*,int,int,int,double,double,int64_t[4],double*)
   FUNCTION lsf_curvature_band(phi,mask,kappa,gauss,gmag,nx,ny,nz,dx,clamp,info,kappa_max) &
            BIND(C,NAME='lsf_curvature_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      REAL(c_double), INTENT(INOUT) :: kappa(*)
      TYPE(c_ptr), VALUE :: gauss,gmag       ! NULL: not wanted
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), VALUE :: dx,clamp
      INTEGER(c_int64_t), INTENT(OUT) :: info(4)
      REAL(c_double), INTENT(OUT) :: kappa_max
      INTEGER(c_int) :: rc
   END FUNCTION lsf_curvature_band
   ! int lsf_measure_band(const double*,const int32_t*,const double*,double*,int,int,int,double,const double[3],double,double[9],
   !                      int64_t[5])
   FUNCTION lsf_measure_band(phi,mask,q,cell_area,nx,ny,nz,dx,xLo,iso,M,info) &
            BIND(C,NAME='lsf_measure_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*),xLo(3)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      TYPE(c_ptr), VALUE :: q,cell_area      ! NULL: no field to integrate, no per-cell areas wanted
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), VALUE :: dx,iso
      REAL(c_double), INTENT(OUT) :: M(9)
      INTEGER(c_int64_t), INTENT(OUT) :: info(5)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_measure_band
   ! int lsf_cut_cells_band(const double*,const int32_t*,int,int,int,double,double,double*,double*,double*,double*,double*,double*,
   !                        double*,double*,double*,int64_t[5])
   FUNCTION lsf_cut_cells_band(phi,mask,nx,ny,nz,dx,iso,vof,ax,ay,az,bx,by,bz,volume,vof_min,info) &
            BIND(C,NAME='lsf_cut_cells_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), VALUE :: dx,iso
      REAL(c_double), INTENT(INOUT) :: vof(*),ax(*),ay(*),az(*)
      TYPE(c_ptr), VALUE :: bx,by,bz         ! NULL: no area vector wanted
      REAL(c_double), INTENT(OUT) :: volume,vof_min
      INTEGER(c_int64_t), INTENT(OUT) :: info(5)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_cut_cells_band
   ! int lsf_label_band(const double*,const int32_t*,int32_t*,int,int,int,double,int,int,int64_t*,int,int64_t*,int64_t[8])
   FUNCTION lsf_label_band(phi,mask,label,nx,ny,nz,iso,side,max_passes,comp,comp_cap,ncomp,info) &
            BIND(C,NAME='lsf_label_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      INTEGER(c_int), INTENT(INOUT) :: label(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,side,max_passes,comp_cap
      REAL(c_double), VALUE :: iso
      TYPE(c_ptr), VALUE :: comp             ! NULL with comp_cap = 0: no table wanted
      INTEGER(c_int64_t), INTENT(OUT) :: ncomp
      INTEGER(c_int64_t), INTENT(OUT) :: info(8)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_label_band
   ! int lsf_redistance_band(double*,const int32_t*,int,int,int,double,double,int,double,int,int*,int64_t*,int,double*,int64_t[9])
   FUNCTION lsf_redistance_band(phi,mask,nx,ny,nz,dx,near,iters,tol,max_passes,passes_done,changed_trace,trace_cap,change,info) &
            BIND(C,NAME='lsf_redistance_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t
      REAL(c_double), INTENT(INOUT) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,iters,max_passes,trace_cap
      REAL(c_double), VALUE :: dx,near,tol
      INTEGER(c_int), INTENT(OUT) :: passes_done
      INTEGER(c_int64_t), INTENT(OUT) :: changed_trace(*)
      REAL(c_double), INTENT(OUT) :: change
      INTEGER(c_int64_t), INTENT(OUT) :: info(9)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_redistance_band
   ! int lsf_sample_points(const double*,const int32_t*,const double*,int,int,int,double,const double[3],const double*,int,int,
   !                       double,int,double,double*,double*,double*,double*,int32_t*,int64_t[6])
   FUNCTION lsf_sample_points(phi,mask,q,nx,ny,nz,dx,xLo,pts,npts,order,iso,iters,tol,val,grad,qval,foot,status,info) &
            BIND(C,NAME='lsf_sample_points') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*),xLo(3),pts(*)
      TYPE(c_ptr), VALUE :: mask,q           ! NULL: no band, no second field
      INTEGER(c_int), VALUE :: nx,ny,nz,npts,order,iters
      REAL(c_double), VALUE :: dx,iso,tol
      REAL(c_double), INTENT(OUT) :: val(*),grad(*)
      TYPE(c_ptr), VALUE :: qval,foot        ! NULL: not wanted (qval needs q, foot needs iters >= 1)
      INTEGER(c_int), INTENT(OUT) :: status(*)
      INTEGER(c_int64_t), INTENT(OUT) :: info(6)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_sample_points
   ! int lsf_cast_rays(const double*,const int32_t*,const double*,int,int,int,double,const double[3],const double*,const double*,int,int,
   !                   double,double,double,double,double,double,double,int,int,double*,double*,double*,double*,int32_t*,int64_t[9])
   FUNCTION lsf_cast_rays(phi,mask,q,nx,ny,nz,dx,xLo,org,dir,nrays,order,iso,tmin,tmax,safety,smin,smax,skip,refine,max_steps, &
                          thit,hit,grad,qval,status,info) BIND(C,NAME='lsf_cast_rays') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*),xLo(3),org(*),dir(*)
      TYPE(c_ptr), VALUE :: mask,q           ! NULL: no band, no second field
      INTEGER(c_int), VALUE :: nx,ny,nz,nrays,order,refine,max_steps
      REAL(c_double), VALUE :: dx,iso,tmin,tmax,safety,smin,smax,skip
      REAL(c_double), INTENT(OUT) :: thit(*),hit(*),grad(*)
      TYPE(c_ptr), VALUE :: qval             ! NULL: not wanted (qval needs q)
      INTEGER(c_int), INTENT(OUT) :: status(*)
      INTEGER(c_int64_t), INTENT(OUT) :: info(9)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_cast_rays
   ! int lsf_advect_points(const double*,const double*,const double*,const double*,const double*,const int32_t*,int,int,int,double,
   !                       const double[3],double*,int,int,int,double,int,int32_t*,double*,int64_t[6])
   FUNCTION lsf_advect_points(u,v,w,phi,speed,mask,nx,ny,nz,dx,xLo,pts,npts,order,scheme,dt,nsteps,status,cfl,info) &
            BIND(C,NAME='lsf_advect_points') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      TYPE(c_ptr), VALUE :: u,v,w,phi,speed,mask   ! NULL: that group, or the band, is absent
      INTEGER(c_int), VALUE :: nx,ny,nz,npts,order,scheme,nsteps
      REAL(c_double), VALUE :: dx,dt
      REAL(c_double), INTENT(IN) :: xLo(3)
      REAL(c_double), INTENT(INOUT) :: pts(*)
      INTEGER(c_int), INTENT(OUT) :: status(*)
      REAL(c_double), INTENT(OUT) :: cfl
      INTEGER(c_int64_t), INTENT(OUT) :: info(6)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_advect_points
   ! int lsf_correct_field(double*,const int32_t*,int,int,int,double,const double[3],const double*,const double*,int,double,int32_t*,
   !                       double*,int64_t[7])
   FUNCTION lsf_correct_field(phi,mask,nx,ny,nz,dx,xLo,pts,rad,npts,slack,status,change,info) &
            BIND(C,NAME='lsf_correct_field') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: phi(*)
      TYPE(c_ptr), VALUE :: mask             ! NULL: the whole grid
      INTEGER(c_int), VALUE :: nx,ny,nz,npts
      REAL(c_double), VALUE :: dx,slack
      REAL(c_double), INTENT(IN) :: xLo(3),pts(*),rad(*)
      INTEGER(c_int), INTENT(OUT) :: status(*)
      REAL(c_double), INTENT(OUT) :: change
      INTEGER(c_int64_t), INTENT(OUT) :: info(7)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_correct_field
   ! int lsf_reseed_points(const double*,const int32_t*,int,int,int,double,const double[3],const double*,const double*,int,int,double,
   !                       double,double,int,int,double,uint64_t,int32_t*,int*,int64_t[14])
   FUNCTION lsf_reseed_points(phi,mask,nx,ny,nz,dx,xLo,pts,rad,npts,per_cell,rmin,rmax,band,order,iters,tol,seed,status,nout,info) &
            BIND(C,NAME='lsf_reseed_points') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(IN) :: phi(*)
      TYPE(c_ptr), VALUE :: mask             ! NULL: the whole grid
      INTEGER(c_int), VALUE :: nx,ny,nz,npts,per_cell,order,iters
      REAL(c_double), VALUE :: dx,rmin,rmax,band,tol
      REAL(c_double), INTENT(IN) :: xLo(3),pts(*),rad(*)
      INTEGER(c_int64_t), VALUE :: seed      ! the bits of a uint64_t, taken as they are
      INTEGER(c_int), INTENT(OUT) :: status(*)
      INTEGER(c_int), INTENT(OUT) :: nout
      INTEGER(c_int64_t), INTENT(OUT) :: info(14)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_reseed_points
   FUNCTION lsf_reseed_get(pts_out,rad_out,src_out) BIND(C,NAME='lsf_reseed_get') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(OUT) :: pts_out(*),rad_out(*)
      INTEGER(c_int), INTENT(OUT) :: src_out(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_reseed_get
   ! int lsf_extend_field_band(double*,const double*,const int32_t*,const int32_t*,int,int,int,double,double,int,int*,int64_t*,int,
   !                           int64_t[4])
   FUNCTION lsf_extend_field_band(q,phi,mask,known,nx,ny,nz,dx,band,max_passes,passes_done,changed_trace,trace_cap,info) &
            BIND(C,NAME='lsf_extend_field_band') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t, c_ptr
      REAL(c_double), INTENT(INOUT) :: q(*)
      REAL(c_double), INTENT(IN) :: phi(*)
      INTEGER(c_int), INTENT(IN) :: mask(*)
      TYPE(c_ptr), VALUE :: known            ! NULL: the frozen cells are the list cells with |phi| < band*dx
      INTEGER(c_int), VALUE :: nx,ny,nz,max_passes,trace_cap
      REAL(c_double), VALUE :: dx,band
      INTEGER(c_int), INTENT(OUT) :: passes_done
      INTEGER(c_int64_t), INTENT(OUT) :: changed_trace(*),info(4)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_extend_field_band
   FUNCTION lsf_advect_nodes(phi,phiSB,nx,ny,nz,dx,xLo,surfXX,nSurfNode,iters) &
            BIND(C,NAME='lsf_advect_nodes') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(IN) :: phi(*),xLo(3)
      INTEGER(c_int), INTENT(IN) :: phiSB(*)
      INTEGER(c_int), VALUE :: nx,ny,nz,nSurfNode,iters
      REAL(c_double), VALUE :: dx
      REAL(c_double), INTENT(INOUT) :: surfXX(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_advect_nodes
   FUNCTION lsf_mirror(flags) BIND(C,NAME='lsf_mirror') RESULT(rc)
      IMPORT :: c_int
      INTEGER(c_int), VALUE :: flags
      INTEGER(c_int) :: rc
   END FUNCTION lsf_mirror
   FUNCTION lsf_mirror_sync(host) BIND(C,NAME='lsf_mirror_sync') RESULT(rc)
      IMPORT :: c_int, c_ptr
      TYPE(c_ptr), VALUE :: host
      INTEGER(c_int) :: rc
   END FUNCTION lsf_mirror_sync
   FUNCTION lsf_mirror_forget(host) BIND(C,NAME='lsf_mirror_forget') RESULT(rc)
      IMPORT :: c_int, c_ptr
      TYPE(c_ptr), VALUE :: host
      INTEGER(c_int) :: rc
   END FUNCTION lsf_mirror_forget
   FUNCTION lsf_snapshot(phi,phiO,nx,ny,nz) BIND(C,NAME='lsf_snapshot') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(IN) :: phi(*)
      REAL(c_double), INTENT(INOUT) :: phiO(*)
      INTEGER(c_int), VALUE :: nx,ny,nz
      INTEGER(c_int) :: rc
   END FUNCTION lsf_snapshot
   FUNCTION lsf_sumsq_diff(phi,phiO,nx,ny,nz,s) BIND(C,NAME='lsf_sumsq_diff') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(IN) :: phi(*),phiO(*)
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), INTENT(OUT) :: s
      INTEGER(c_int) :: rc
   END FUNCTION lsf_sumsq_diff
   FUNCTION lsf_write_vti(path,phi,nx,ny,nz,dx,xLo) BIND(C,NAME='lsf_write_vti') RESULT(rc)
      IMPORT :: c_int, c_double, c_char
      CHARACTER(KIND=c_char), INTENT(IN) :: path(*)
      REAL(c_double), INTENT(IN) :: phi(*),xLo(3)
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), VALUE :: dx
      INTEGER(c_int) :: rc
   END FUNCTION lsf_write_vti
   ! int lsf_extract_surface(const double*,int,int,int,double,const double[3],double,int*,int*,int64_t[4])
   FUNCTION lsf_extract_surface(phi,nx,ny,nz,dx,xLo,iso,nSurfNode,nSurfElem,info) BIND(C,NAME='lsf_extract_surface') RESULT(rc)
      IMPORT :: c_int, c_double, c_int64_t
      REAL(c_double), INTENT(IN) :: phi(*),xLo(3)
      INTEGER(c_int), VALUE :: nx,ny,nz
      REAL(c_double), VALUE :: dx,iso
      INTEGER(c_int), INTENT(OUT) :: nSurfNode,nSurfElem
      INTEGER(c_int64_t), INTENT(OUT) :: info(4)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_extract_surface
   FUNCTION lsf_extract_get(surfX,surfElem) BIND(C,NAME='lsf_extract_get') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(OUT) :: surfX(*)
      INTEGER(c_int), INTENT(OUT) :: surfElem(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_extract_get
   FUNCTION lsf_stl_write(path,surfX,nSurfNode,surfElem,nSurfElem) BIND(C,NAME='lsf_stl_write') RESULT(rc)
      IMPORT :: c_int, c_double, c_char
      CHARACTER(KIND=c_char), INTENT(IN) :: path(*)
      REAL(c_double), INTENT(IN) :: surfX(*)
      INTEGER(c_int), INTENT(IN) :: surfElem(*)
      INTEGER(c_int), VALUE :: nSurfNode,nSurfElem
      INTEGER(c_int) :: rc
   END FUNCTION lsf_stl_write
   FUNCTION lsf_stl_read(path,nSurfElem,nSurfNode) BIND(C,NAME='lsf_stl_read') RESULT(rc)
      IMPORT :: c_int, c_char
      CHARACTER(KIND=c_char), INTENT(IN) :: path(*)
      INTEGER(c_int), INTENT(OUT) :: nSurfElem,nSurfNode
      INTEGER(c_int) :: rc
   END FUNCTION lsf_stl_read
   FUNCTION lsf_stl_get(surfX,surfElem) BIND(C,NAME='lsf_stl_get') RESULT(rc)
      IMPORT :: c_int, c_double
      REAL(c_double), INTENT(OUT) :: surfX(*)
      INTEGER(c_int), INTENT(OUT) :: surfElem(*)
      INTEGER(c_int) :: rc
   END FUNCTION lsf_stl_get
   FUNCTION lsf_last_error() BIND(C,NAME='lsf_last_error') RESULT(p)
      IMPORT :: c_ptr
      TYPE(c_ptr) :: p
   END FUNCTION lsf_last_error
   FUNCTION c_strlen(s) BIND(C,NAME='strlen') RESULT(n)
      IMPORT :: c_ptr, c_size_t
      TYPE(c_ptr), VALUE :: s
      INTEGER(c_size_t) :: n
   END FUNCTION c_strlen
END INTERFACE

CONTAINS

!*************************************************************************************!
! mode word of include/lsf.h from the environment
!*************************************************************************************!
FUNCTION lsf_mode() RESULT(mode)
INTEGER(c_int) :: mode
CHARACTER(LEN=32) :: v
INTEGER :: st
CALL lsf_load_inputs()
CALL lsf_set_mirror()
mode = 0
v = nml_order
CALL get_environment_variable('LSF_ORDER',v,STATUS=st)
IF (st /= 0) v = nml_order
IF (LEN_TRIM(v) > 0 .AND. TRIM(v) /= 'gs' .AND. TRIM(v) /= 'jacobi') THEN
   PRINT*, " liblsf_hip: order must be 'gs' or 'jacobi', not ",TRIM(v)
   STOP 1
END IF
IF (TRIM(v) == 'jacobi') mode = mode + LSF_ORDER_JACOBI
CALL get_environment_variable('LSF_ARITH',v,STATUS=st)
IF (st /= 0) v = nml_arith
! the reference's own arithmetic unless the run asks for the fast one: a drop-in returns the reference's numbers
IF (LEN_TRIM(v) > 0 .AND. TRIM(v) /= 'strict' .AND. TRIM(v) /= 'fast') THEN
   PRINT*, " liblsf_hip: arith must be 'strict' or 'fast', not ",TRIM(v)
   STOP 1
END IF
IF (TRIM(v) /= 'fast') mode = mode + LSF_ARITH_STRICT
END FUNCTION lsf_mode

!*************************************************************************************!
! &lsf_inputs: from the file named by the second command-line argument, else ./lsf.nml
!*************************************************************************************!
SUBROUTINE lsf_load_inputs()
REAL :: dx,redist_tol
INTEGER :: dd,dd_lo(3),dd_hi(3),reinit_iter,minmax_iter,reinit2_iter,ios,u,resident,devices(16),check_every,slabs
INTEGER :: redist_iters,redist_passes
CHARACTER(LEN=16) :: order,arith,transport
CHARACTER(LEN=1024) :: path
LOGICAL :: there
NAMELIST /lsf_inputs/ dx,dd,dd_lo,dd_hi,reinit_iter,minmax_iter,reinit2_iter,order,arith,resident,devices,transport,check_every,slabs, &
                      redist_iters,redist_tol,redist_passes
IF (nml_loaded) RETURN
nml_loaded = .TRUE.
path = ' '
IF (command_argument_count() >= 2) CALL get_command_argument(2,path)
IF (LEN_TRIM(path) == 0) path = 'lsf.nml'
INQUIRE(FILE=TRIM(path),EXIST=there)
IF (.NOT. there) THEN
   IF (command_argument_count() >= 2) THEN
      PRINT*, " liblsf_hip: namelist file not found: ",TRIM(path)
      STOP 1
   END IF
   RETURN
END IF
dx = nml_dx; dd = nml_dd; dd_lo = nml_dd_lo; dd_hi = nml_dd_hi
reinit_iter = nml_reinit_iter; minmax_iter = nml_minmax_iter; reinit2_iter = nml_reinit2_iter
order = nml_order; arith = nml_arith; resident = nml_resident; devices = nml_devices
transport = nml_transport; check_every = nml_check_every; slabs = nml_slabs
redist_iters = nml_redist_iters; redist_tol = nml_redist_tol; redist_passes = nml_redist_passes
u = 47
OPEN(UNIT=u,FILE=TRIM(path),STATUS='old',ACTION='read',IOSTAT=ios)
IF (ios == 0) READ(u,NML=lsf_inputs,IOSTAT=ios)
IF (ios /= 0) THEN
   PRINT*, " liblsf_hip: cannot read &lsf_inputs from ",TRIM(path)
   STOP 1
END IF
CLOSE(u)
nml_dx = dx; nml_dd = dd; nml_dd_lo = dd_lo; nml_dd_hi = dd_hi
nml_reinit_iter = reinit_iter; nml_minmax_iter = minmax_iter; nml_reinit2_iter = reinit2_iter
nml_order = order; nml_arith = arith; nml_resident = resident; nml_devices = devices
nml_transport = transport; nml_check_every = check_every; nml_slabs = slabs
nml_redist_iters = redist_iters; nml_redist_tol = redist_tol; nml_redist_passes = redist_passes
PRINT*, " Run parameters read from ",TRIM(path)
END SUBROUTINE lsf_load_inputs

! GPUs for the block-decomposed reinit: LSF_DEVICES="0,1,..." or the namelist's `devices`; nd = leading entries >= 0
SUBROUTINE lsf_device_list(devs,nd)
INTEGER(c_int), INTENT(OUT) :: devs(16),nd
CHARACTER(LEN=256) :: v
INTEGER :: st,ios
CALL lsf_load_inputs()
devs = nml_devices
CALL get_environment_variable('LSF_DEVICES',v,STATUS=st)
IF (st == 0 .AND. LEN_TRIM(v) > 0) THEN
   devs = -1
   v = v(1:LEN_TRIM(v))//' /'                        ! the slash ends the list: entries not given stay -1
   READ(v,*,IOSTAT=ios) devs
   IF (ios /= 0) THEN
      PRINT*, " liblsf_hip: cannot read LSF_DEVICES=",TRIM(v)
      STOP 1
   END IF
END IF
nd = 0
DO WHILE (nd < 16)
   IF (devs(nd+1) < 0) EXIT
   nd = nd+1
END DO
END SUBROUTINE lsf_device_list

SUBROUTINE lsf_fail(where,rc)
CHARACTER(LEN=*), INTENT(IN) :: where
INTEGER(c_int), INTENT(IN) :: rc
TYPE(c_ptr) :: p
CHARACTER(KIND=c_char), POINTER :: s(:)
INTEGER :: n,i
CHARACTER(LEN=512) :: msg
msg = ''
p = lsf_last_error()
IF (c_associated(p)) THEN
   n = MIN(INT(c_strlen(p)),512)
   CALL c_f_pointer(p,s,(/n/))
   DO i = 1,n
      msg(i:i) = s(i)
   END DO
END IF
PRINT*, " liblsf_hip: ",where," failed with code ",rc,": ",TRIM(msg)
STOP 1
END SUBROUTINE lsf_fail

!*************************************************************************************!
! Reinitialize the signed distance function  (same dummy arguments as subs.f90:717-725)
!*************************************************************************************!
SUBROUTINE reinit(phi,gradPhi,gradPhiMag,nx,ny,nz,iter,dx,h)

INTEGER,INTENT(IN) :: nx,ny,nz,iter
REAL,INTENT(IN) :: dx,h
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi,gradPhiMag
REAL,DIMENSION(0:nx,0:ny,0:nz,3),INTENT(INOUT) :: gradPhi
REAL,ALLOCATABLE :: trace(:)
INTEGER(c_int) :: rc,done,mode,devs(16),nd
INTEGER :: n,use_slabs

! gradPhi and gradPhiMag are dead outputs of the reference's reinit: the host zeroes them
! right after the first call (set3d.f90:372-375) and never reads them after the second.
! They are left untouched.

ALLOCATE(trace(iter+1))
mode = lsf_mode()
CALL lsf_device_list(devs,nd)
use_slabs = nml_slabs
CALL lsf_env_int('LSF_SLABS',use_slabs)
IF (nd >= 2 .AND. IAND(mode,LSF_ORDER_JACOBI) /= 0) THEN
   ! one block per listed GPU, halos peer to peer, same result as one GPU (include/lsf.h: lsf_reinit_multi)
   PRINT*, " Reinit block-decomposed over ",nd," devices "
   IF (LEN_TRIM(nml_transport) > 0 .AND. TRIM(nml_transport) /= 'peer' .AND. TRIM(nml_transport) /= 'rccl') THEN
      PRINT*, " liblsf_hip: transport must be 'peer' or 'rccl', not ",TRIM(nml_transport)
      STOP 1
   END IF
   rc = lsf_multi_defaults(nml_check_every,MERGE(1,0,TRIM(nml_transport) == 'rccl'))
   IF (rc /= LSF_OK) CALL lsf_fail('lsf_multi_defaults',rc)
   rc = lsf_reinit_multi(phi,nx,ny,nz,iter,dx,h,1.E-5,mode,devs,nd,C_NULL_PTR,done,trace,iter+1)
   IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_reinit_multi',rc)
ELSE IF (nd >= 2 .AND. use_slabs /= 0) THEN
   ! the reference's own ordering, one slab of z per listed GPU: the field of one GPU, bit for bit (include/lsf.h).
   ! Opt-in (slabs = 1 / LSF_SLABS=1): without it a device list with order = 'gs' runs on one GPU, as it always did.
   PRINT*, " Reinit in the reference's ordering over ",nd," z slabs "
   rc = lsf_reinit_multi(phi,nx,ny,nz,iter,dx,h,1.E-5,mode,devs,nd,C_NULL_PTR,done,trace,iter+1)
   IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_reinit_multi',rc)
ELSE
   IF (nd >= 2) PRINT*, " Reinit in the reference's ordering on one device (slabs = 1 shards it over the listed devices) "
   rc = lsf_reinit(phi,nx,ny,nz,iter,dx,h,1.E-5,mode,done,trace,iter+1)
   IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_reinit',rc)
END IF

! what the reference prints, sweep by sweep (subs.f90:915-926)
DO n = 0,done-1
   IF (trace(n+1) < 1.E-5) THEN
      PRINT*, " Distance function time integration has reached steady state "
      EXIT
   END IF
   PRINT*, " Iteration: ",n," ", " RMS Error: ",trace(n+1)
   IF (isnan(trace(n+1))) STOP
END DO
PRINT*
DEALLOCATE(trace)

END SUBROUTINE reinit

!*************************************************************************************!
! Reinitialize on the cells of a mask only (include/lsf.h: lsf_reinit_band; no reference
! counterpart).  mask: e.g. phiSB of narrowBand; the interior cells where it is 1 are
! updated, every other point keeps its value.  Always the Jacobi ordering (a raster order
! has no meaning on a list of cells); the arithmetic is the run's (arith / LSF_ARITH).
! The residual printed is the RMS change over the listed cells.
!*************************************************************************************!
SUBROUTINE reinitBand(phi,mask,nx,ny,nz,iter,dx,h)

INTEGER,INTENT(IN) :: nx,ny,nz,iter
REAL,INTENT(IN) :: dx,h
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
REAL,ALLOCATABLE :: trace(:)
INTEGER(c_int) :: rc,done,mode
INTEGER :: n

ALLOCATE(trace(iter+1))
mode = lsf_mode()
mode = IOR(IAND(mode,LSF_ARITH_STRICT),LSF_ORDER_JACOBI)
rc = lsf_reinit_band(phi,mask,nx,ny,nz,iter,dx,h,1.E-5,mode,done,trace,iter+1)
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_reinit_band',rc)

! the lines of reinit, sweep by sweep (subs.f90:915-926)
DO n = 0,done-1
   IF (trace(n+1) < 1.E-5) THEN
      PRINT*, " Distance function time integration has reached steady state "
      EXIT
   END IF
   PRINT*, " Iteration: ",n," ", " RMS Error: ",trace(n+1)
   IF (isnan(trace(n+1))) STOP
END DO
PRINT*
DEALLOCATE(trace)

END SUBROUTINE reinitBand

!*************************************************************************************!
! Determine Narrow Band  (same dummy arguments as subs.f90:178-184)
!*************************************************************************************!
SUBROUTINE narrowBand(nx,ny,nz,dx,phi,phiNB,phiSB)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phiNB,phiSB
INTEGER(c_int) :: rc

CALL lsf_set_mirror()
rc = lsf_narrowband(phi,phiNB,phiSB,nx,ny,nz,dx)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_narrowband',rc)

END SUBROUTINE narrowBand

!*************************************************************************************!
! Min/Max Flow: the loop of set3d.f90:394-462 as one call
!*************************************************************************************!
SUBROUTINE minmaxFlow(phi,phiNB,phiSB,nx,ny,nz,iter,dx,h1)

INTEGER,INTENT(IN) :: nx,ny,nz,iter
REAL,INTENT(IN) :: dx,h1
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phiNB,phiSB
REAL,ALLOCATABLE :: trace(:)
INTEGER(c_int) :: rc,done
INTEGER :: n

ALLOCATE(trace(MAX(iter,1)))
rc = lsf_minmax(phi,phiNB,phiSB,nx,ny,nz,iter,dx,h1,1.E-7,lsf_mode(),done,trace,MAX(iter,1))
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_minmax',rc)

! what the reference prints (set3d.f90:448-458)
DO n = 1,done
   IF (trace(n) < 1.E-7) THEN
      PRINT*, " Min/max time integration has reached steady state "
      EXIT
   END IF
   PRINT*, " Iteration: ",n," ", " RMS Error: ",trace(n)
   IF (isnan(trace(n))) STOP
END DO
PRINT*
DEALLOCATE(trace)

END SUBROUTINE minmaxFlow

!*************************************************************************************!
! Inside/outside initialisation: the search loop of set3d.f90:218-268 as one call
! (SURVEY.md section 8f rank 1).  phi must hold 1. on entry like at set3d.f90:161.
!*************************************************************************************!
SUBROUTINE phi0Init(phi,nx,ny,nz,dx,xLo,xMin,xMax,surfX,nSurfNode,surfElem,nSurfElem)

INTEGER,INTENT(IN) :: nx,ny,nz
INTEGER*4,INTENT(IN) :: nSurfNode,nSurfElem
REAL,INTENT(IN) :: dx,xLo(3),xMin(3),xMax(3)
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
REAL,INTENT(IN) :: surfX(nSurfNode,3)
INTEGER*4,INTENT(IN) :: surfElem(nSurfElem,3)
INTEGER(c_int) :: rc

CALL lsf_set_mirror()
rc = lsf_phi0(phi,nx,ny,nz,dx,xLo,xMin,xMax,surfX,nSurfNode,surfElem,nSurfElem)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_phi0',rc)

END SUBROUTINE phi0Init

!*************************************************************************************!
! Exact signed distance from the triangle mesh (include/lsf.h: lsf_mesh_distance; no
! reference counterpart).  phi is an output: the distance to the nearest triangle,
! negative inside, within width cells of the surface and +-width*dx elsewhere.  surfX and
! surfElem as stlRead returns them.  A mesh with defective edges fails through lsf_fail.
!*************************************************************************************!
SUBROUTINE meshDistance(phi,nx,ny,nz,dx,xLo,surfX,nSurfNode,surfElem,nSurfElem,width)

INTEGER,INTENT(IN) :: nx,ny,nz
INTEGER*4,INTENT(IN) :: nSurfNode,nSurfElem
REAL,INTENT(IN) :: dx,xLo(3),width
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
REAL,INTENT(IN) :: surfX(nSurfNode,3)
INTEGER*4,INTENT(IN) :: surfElem(nSurfElem,3)
INTEGER(c_int64_t) :: info(4)
INTEGER(c_int) :: rc

CALL lsf_set_mirror()
rc = lsf_mesh_distance(phi,nx,ny,nz,dx,xLo,surfX,nSurfNode,surfElem,nSurfElem,width,0_c_int,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_mesh_distance',rc)

END SUBROUTINE meshDistance

!*************************************************************************************!
! First-order distance outside a frozen band by fast sweeping (include/lsf.h:
! lsf_distance_fill; no reference counterpart).  The points with |phi| < band*dx on entry
! (the tube of meshDistance(width = band)) are never written; every other point keeps its
! sign and receives the distance grown outwards from them, at most 64 rounds of 8 raster
! sweeps.  Prints the rounds run and the visits the last one lowered (0: converged).
!*************************************************************************************!
SUBROUTINE distanceFill(phi,nx,ny,nz,dx,band)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,band
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER(c_int), PARAMETER :: max_rounds = 64
INTEGER(c_int64_t) :: trace(max_rounds),frozen
INTEGER(c_int) :: rc,done

CALL lsf_set_mirror()
rc = lsf_distance_fill(phi,c_null_ptr,nx,ny,nz,dx,band,max_rounds,done,trace,max_rounds,frozen)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_distance_fill',rc)
PRINT*, " Distance fill: ",done," rounds, ",frozen," frozen points, last round lowered ",trace(done)
PRINT*

END SUBROUTINE distanceFill

!*************************************************************************************!
! A quantity carried off the surface constant along the normals of phi (include/lsf.h:
! lsf_extend_field; no reference counterpart).  The points with |phi| < band*dx hold the
! caller's q and are never written; every other point receives the value that reaches it
! along the normal, at most 64 rounds of 8 raster sweeps.  phi is not written.  Points a
! plateau of |phi| keeps out of reach stay NaN and are counted.  Prints the rounds run,
! the visits the last one changed (0: converged) and the unreached points.
!*************************************************************************************!
SUBROUTINE extendField(q,phi,nx,ny,nz,dx,band)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,band
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: q
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER(c_int), PARAMETER :: max_rounds = 64
INTEGER(c_int64_t) :: trace(max_rounds),info(3)
INTEGER(c_int) :: rc,done

CALL lsf_set_mirror()
rc = lsf_extend_field(q,phi,c_null_ptr,nx,ny,nz,dx,band,max_rounds,done,trace,max_rounds,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_extend_field',rc)
PRINT*, " Extend field: ",done," rounds, ",info(1)," frozen points, last round changed ",trace(done),", unreached ",info(3)
PRINT*

END SUBROUTINE extendField

!*************************************************************************************!
! extendField on the cells with mask == 1 only (include/lsf.h: lsf_extend_field_band; no
! reference counterpart): the list cells with |phi| < band*dx hold the caller's q and are
! never written; every other list cell receives the value that reaches it along the normal
! through list cells, at most 256 Jacobi passes over the list.  q is neither read nor
! written outside the list; phi and mask are not written.  List cells no value reaches
! stay NaN and are counted.  Prints the passes run, the visits the last one changed
! (0: converged) and the unreached cells.
!*************************************************************************************!
SUBROUTINE extendFieldBand(q,phi,mask,nx,ny,nz,dx,band)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,band
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: q
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
INTEGER(c_int), PARAMETER :: max_passes = 256
INTEGER(c_int64_t) :: trace(max_passes),info(4)
INTEGER(c_int) :: rc,done

CALL lsf_set_mirror()
rc = lsf_extend_field_band(q,phi,mask,c_null_ptr,nx,ny,nz,dx,band,max_passes,done,trace,max_passes,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_extend_field_band',rc)
PRINT*, " Extend field on the band: ",info(1)," list cells, ",info(2)," frozen, ",done," passes, last pass changed ",trace(done), &
        ", unreached ",info(4)
PRINT*

END SUBROUTINE extendFieldBand

!*************************************************************************************!
! The distance property restored on the cells with mask == 1 from closest points
! (include/lsf_redistance.h: lsf_redistance_band; no reference counterpart): a list cell
! whose foot on the interpolant's zero level set is found closer than near*dx takes that
! distance with the sign it had; the other list cells are filled from those by Jacobi
! passes of distanceFill's visit over the list.  Nothing outside the list is read or
! written, no cell changes sign, and list cells that no frozen cell reaches keep their
! value and are counted.  iters, tol and the cap of the passes come from &lsf_inputs
! (redist_iters = 8, redist_tol = 1e-9, redist_passes = 64).  Prints the counts, the
! passes run, the visits the last one lowered (0: converged) and the largest change.
!*************************************************************************************!
SUBROUTINE redistanceBand(phi,mask,nx,ny,nz,dx,near)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,near
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
INTEGER(c_int64_t), ALLOCATABLE :: trace(:)
INTEGER(c_int64_t) :: info(9)
INTEGER(c_int) :: rc,done
REAL(c_double) :: change

CALL lsf_load_inputs()
CALL lsf_set_mirror()
ALLOCATE(trace(MAX(nml_redist_passes,1)))
rc = lsf_redistance_band(phi,mask,nx,ny,nz,dx,near,nml_redist_iters,nml_redist_tol,nml_redist_passes,done,trace, &
                         MAX(nml_redist_passes,1),change,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_redistance_band',rc)
PRINT*, " Redistance on the band: list cells, frozen, filled, unreached ",info(1),info(2),info(3),info(4)
PRINT*, " Redistance on the band: feet off the band, outside, flat, not converged, beyond near ",info(5),info(6),info(7),info(8),info(9)
PRINT*, " Redistance on the band: ",done," passes, last pass lowered ",trace(done),", largest change ",change
PRINT*
DEALLOCATE(trace)

END SUBROUTINE redistanceBand

!*************************************************************************************!
! Transport of the level set by a velocity field, phi_t + u.grad(phi) = 0 (include/lsf.h:
! lsf_advect_field; no reference counterpart): `steps` steps of size dt, WENO5 one-sided
! derivatives, TVD-RK3, the reference's own arithmetic (LSF_ARITH_STRICT), the
! extrapolation boundary condition after every stage.  u, v, w have phi's shape and are
! read only.  The CFL number is printed, not judged: keep dt*max(|u|+|v|+|w|)/dx below 1.
! A NaN stops the run like the reference's reinit (subs.f90:926).
!*************************************************************************************!
SUBROUTINE advectField(phi,u,v,w,nx,ny,nz,dx,dt,steps)

INTEGER,INTENT(IN) :: nx,ny,nz,steps
REAL,INTENT(IN) :: dx,dt
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: u,v,w
INTEGER(c_int), PARAMETER :: LSF_ADVECT_RK3 = 0
REAL,ALLOCATABLE :: trace(:)
REAL :: cfl
INTEGER(c_int) :: rc,done,mode

ALLOCATE(trace(MAX(steps,1)))
trace = 0.
cfl = 0.
done = 0
CALL lsf_set_mirror()
mode = IOR(LSF_ARITH_STRICT,LSF_ORDER_JACOBI)
rc = lsf_advect_field(phi,u,v,w,c_null_ptr,nx,ny,nz,dx,dt,steps,LSF_ADVECT_RK3,mode,done,cfl,trace,MAX(steps,1))
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_advect_field',rc)
PRINT*, " Level-set transport: ",done," steps, CFL ",cfl,", last change ",trace(MAX(done,1))
PRINT*
IF (rc == LSF_ERR_NAN) STOP
DEALLOCATE(trace)

END SUBROUTINE advectField

!*************************************************************************************!
! advectField on the cells of a mask only (include/lsf.h: lsf_advect_field_band; no
! reference counterpart): the interior points with mask == 1 (e.g. phiSB of narrowBand)
! take `steps` steps of size dt, WENO5 / TVD-RK3 in the reference's own arithmetic
! (LSF_ARITH_STRICT); every other point keeps its value and no boundary condition is
! applied.  u, v, w are read at those cells only.  Prints the steps, the CFL number over
! the list, the last change, the list and edge cells, the edge cells whose sign changed
! (> 0: the surface reached the edge of the mask -- rebuild it) and the smallest |phi|
! over the edge cells in units of dx.  A NaN stops the run like advectField.
!*************************************************************************************!
SUBROUTINE advectFieldBand(phi,mask,u,v,w,nx,ny,nz,dx,dt,steps)

INTEGER,INTENT(IN) :: nx,ny,nz,steps
REAL,INTENT(IN) :: dx,dt
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: u,v,w
INTEGER(c_int), PARAMETER :: LSF_ADVECT_RK3 = 0
REAL,ALLOCATABLE :: trace(:)
REAL :: cfl,margin
INTEGER(c_int64_t) :: info(3)
INTEGER(c_int) :: rc,done,mode

ALLOCATE(trace(MAX(steps,1)))
trace = 0.
cfl = 0.
margin = 0.
info = 0
done = 0
CALL lsf_set_mirror()
mode = IOR(LSF_ARITH_STRICT,LSF_ORDER_JACOBI)
rc = lsf_advect_field_band(phi,mask,u,v,w,c_null_ptr,nx,ny,nz,dx,dt,steps,LSF_ADVECT_RK3,mode,done,cfl,trace,MAX(steps,1), &
                           info,margin)
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_advect_field_band',rc)
PRINT*, " Level-set transport on the band: ",done," steps, CFL ",cfl,", last change ",trace(MAX(done,1))
IF (rc == LSF_OK) PRINT*, "   list cells ",info(1),", edge cells ",info(2),", edge sign flips ",info(3),", margin/dx ",margin/dx
PRINT*
IF (rc == LSF_ERR_NAN) STOP
DEALLOCATE(trace)

END SUBROUTINE advectFieldBand

!*************************************************************************************!
! The band time loop (include/lsf.h: lsf_evolve_band; no reference counterpart): `steps`
! steps of size dt, each the transport of advectFieldBand followed by two sweeps of the
! reinitialisation (pseudo-time step 0.5 dx) on ONE list of cells that stays on the device
! and is rebuilt when the surface comes within 3 dx of its open edge (core 3, ring 3, a
! check after every step).  phi AND mask are updated: on return mask is 1 on the cells of
! the current list and 0 elsewhere.  u, v, w must be finite at all points.  Prints the
! steps, the CFL number, the last change, the list and open-edge cells, the sign flips of
! the last check (> 0: the surface reached the edge and the run ended early), the
! rebuilds, the cells that entered, the near-wall cells and the margin in units of dx.
! A NaN stops the run like advectField.
!*************************************************************************************!
SUBROUTINE evolveBand(phi,mask,u,v,w,nx,ny,nz,dx,dt,steps)

INTEGER,INTENT(IN) :: nx,ny,nz,steps
REAL,INTENT(IN) :: dx,dt
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: u,v,w
INTEGER(c_int), PARAMETER :: LSF_ADVECT_RK3 = 0
REAL,ALLOCATABLE :: trace(:)
REAL :: cfl,margin
INTEGER(c_int64_t) :: info(6)
INTEGER(c_int) :: rc,done,mode

ALLOCATE(trace(MAX(steps,1)))
trace = 0.
cfl = 0.
margin = 0.
info = 0
done = 0
CALL lsf_set_mirror()
mode = IOR(LSF_ARITH_STRICT,LSF_ORDER_JACOBI)
rc = lsf_evolve_band(phi,mask,u,v,w,c_null_ptr,nx,ny,nz,dx,dt,steps,LSF_ADVECT_RK3,mode,3.0_c_double,3,2,0.5_c_double*dx,1, &
                     done,cfl,trace,MAX(steps,1),info,margin)
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_evolve_band',rc)
PRINT*, " Band time loop: ",done," of ",steps," steps, CFL ",cfl,", last change ",trace(MAX(done,1))
IF (rc == LSF_OK) PRINT*, "   list cells ",info(1),", open-edge cells ",info(2),", sign flips ",info(3),", rebuilds ",info(4), &
                          ", entered ",info(5),", near a wall ",info(6),", margin/dx ",margin/dx
PRINT*
IF (rc == LSF_ERR_NAN) STOP
DEALLOCATE(trace)

END SUBROUTINE evolveBand

!*************************************************************************************!
! The band time loop with a curvature term (include/lsf.h: lsf_evolve_band_curv; no
! reference counterpart): evolveBand for phi_t + speed |grad(phi)| = b kappa |grad(phi)|,
! the speed law F = speed - b*kappa with the curvature term differenced centrally from
! every stage's own field.  No velocity, |kappa| limited to 1/dx (clamp 1), everything else
! evolveBand's defaults: RK3, two sweeps with pseudo-time step 0.5 dx, core 3, ring 3, a
! check after every step.  phi AND mask are updated; speed must be finite at all points.
! Prints evolveBand's lines with the number b dt/dx^2 of the explicit term after the CFL
! number.  A NaN stops the run like advectField.
!*************************************************************************************!
SUBROUTINE evolveBandCurv(phi,mask,speed,nx,ny,nz,dx,dt,steps,b)

INTEGER,INTENT(IN) :: nx,ny,nz,steps
REAL,INTENT(IN) :: dx,dt,b
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: speed
INTEGER(c_int), PARAMETER :: LSF_ADVECT_RK3 = 0
REAL,ALLOCATABLE :: trace(:)
REAL :: cfl,diffusion,margin
INTEGER(c_int64_t) :: info(6)
INTEGER(c_int) :: rc,done,mode

ALLOCATE(trace(MAX(steps,1)))
trace = 0.
cfl = 0.
diffusion = 0.
margin = 0.
info = 0
done = 0
CALL lsf_set_mirror()
mode = IOR(LSF_ARITH_STRICT,LSF_ORDER_JACOBI)
rc = lsf_evolve_band_curv(phi,mask,c_null_ptr,c_null_ptr,c_null_ptr,speed,nx,ny,nz,dx,dt,steps,LSF_ADVECT_RK3,mode,3.0_c_double,3,2, &
                          0.5_c_double*dx,1,b,1.0_c_double,done,cfl,diffusion,trace,MAX(steps,1),info,margin)
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_evolve_band_curv',rc)
PRINT*, " Band time loop: ",done," of ",steps," steps, CFL ",cfl,", b dt/dx^2 ",diffusion,", last change ",trace(MAX(done,1))
IF (rc == LSF_OK) PRINT*, "   list cells ",info(1),", open-edge cells ",info(2),", sign flips ",info(3),", rebuilds ",info(4), &
                          ", entered ",info(5),", near a wall ",info(6),", margin/dx ",margin/dx
PRINT*
IF (rc == LSF_ERR_NAN) STOP
DEALLOCATE(trace)

END SUBROUTINE evolveBandCurv

!*************************************************************************************!
! Mean curvature of the level sets on the cells of a mask only (include/lsf.h:
! lsf_curvature_band; the reference's own "true curvature" is commented out,
! subs.f90:426-448): kappa = div(grad(phi)/|grad(phi)|) = k1 + k2 from second-order central
! differences at the interior points with mask == 1 (e.g. phiNB of narrowBand); a sphere
! with phi < 0 inside has kappa = +2/r.  kappa is written at those cells only: every
! other point keeps what it held.  phi and mask are read only.  clamp > 0 limits |kappa|
! to clamp/dx (1. is the usual choice: a grid resolves no more), 0. means no clamp.
! Prints the list cells, the flat cells (kappa = 0 there), the clamped cells and the
! largest |kappa| in units of 1/dx.  A non-finite kappa stops the run like advectField.
!*************************************************************************************!
SUBROUTINE curvatureBand(phi,mask,kappa,nx,ny,nz,dx,clamp)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,clamp
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: kappa
REAL :: kmax
INTEGER(c_int64_t) :: info(4)
INTEGER(c_int) :: rc

kmax = 0.
info = 0
CALL lsf_set_mirror()
rc = lsf_curvature_band(phi,mask,kappa,c_null_ptr,c_null_ptr,nx,ny,nz,dx,clamp,info,kmax)
IF (rc /= LSF_OK .AND. rc /= LSF_ERR_NAN) CALL lsf_fail('lsf_curvature_band',rc)
IF (rc == LSF_OK) PRINT*, " Curvature on the band: list cells ",info(1),", flat cells ",info(2),", clamped cells ",info(3), &
                          ", largest |kappa|*dx ",kmax*dx
IF (rc == LSF_ERR_NAN) PRINT*, " Curvature on the band: a list cell holds a non-finite kappa"
PRINT*
IF (rc == LSF_ERR_NAN) STOP

END SUBROUTINE curvatureBand

!*************************************************************************************!
! How much surface there is and how much body it encloses, on the cells of a mask only
! (include/lsf.h: lsf_measure_band; no reference counterpart): the level set phi = iso is
! measured in the cells whose lower corner is an interior point with mask == 1 (e.g.
! phiNB of narrowBand), triangle by triangle as extractSurface would emit them, and no
! mesh is made.  M(1) area, M(2) enclosed volume, M(3:5) its first moments (the centroid
! is M(3:5)/M(2)), M(6:8) the first moments of the surface, M(9) 0.  phi and mask are read
! only.  Prints the area, the volume, the cells and the triangles, and says when the
! surface leaves the list (volume and centroid then describe an open piece).
!*************************************************************************************!
SUBROUTINE measureBand(phi,mask,nx,ny,nz,dx,xLo,iso,M)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,xLo(3),iso
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
REAL,INTENT(OUT) :: M(9)
INTEGER(c_int64_t) :: info(5)
INTEGER(c_int) :: rc

M = 0.
info = 0
CALL lsf_set_mirror()
rc = lsf_measure_band(phi,mask,c_null_ptr,c_null_ptr,nx,ny,nz,dx,xLo,iso,M,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_measure_band',rc)
PRINT*, " Measures on the band: area ",M(1),", volume ",M(2),", crossed cells ",info(2)," of ",info(1),", triangles ",info(3)
IF (info(4) > 0) PRINT*, " Measures on the band: ",info(4)," crossed cells at the edge of the list: an open piece"
PRINT*

END SUBROUTINE measureBand

!*************************************************************************************!
! How much of each cell lies inside the body and how much of each face is open, on the
! cells of a mask only (include/lsf.h: lsf_cut_cells_band; no reference counterpart):
! what a cut-cell (embedded-boundary) solver takes from a level set.  At every interior
! point with mask == 1 vof receives the fraction of the cell whose lower corner the point
! is that lies in phi < iso, and ax, ay, az the open fractions of that cell's LOWER faces
! (the upper ones are the neighbours' lower ones); nothing is written anywhere else.
! volume is the sum of the fractions times dx**3: with a mask of phi < 2.1*dx the body's
! volume.  phi and mask are read only.  Prints the volume, the cells and the smallest
! cut-cell fraction.
!*************************************************************************************!
SUBROUTINE cutCellsBand(phi,mask,nx,ny,nz,dx,iso,vof,ax,ay,az,volume)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,iso
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: vof,ax,ay,az
REAL,INTENT(OUT) :: volume
REAL :: vof_min
INTEGER(c_int64_t) :: info(5)
INTEGER(c_int) :: rc

volume = 0.
vof_min = 0.
info = 0
CALL lsf_set_mirror()
rc = lsf_cut_cells_band(phi,mask,nx,ny,nz,dx,iso,vof,ax,ay,az,c_null_ptr,c_null_ptr,c_null_ptr,volume,vof_min,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_cut_cells_band',rc)
PRINT*, " Cut cells on the band: volume ",volume,", cut cells ",info(2),", full cells ",info(3)," of ",info(1), &
        ", smallest cut-cell fraction ",vof_min
IF (info(4) > 0) PRINT*, " Cut cells on the band: ",info(4)," cut cells at the edge of the list: an aperture is missing"
PRINT*

END SUBROUTINE cutCellsBand

!*************************************************************************************!
! How many bodies there are and which cell belongs to which, on the cells of a mask only
! (include/lsf.h: lsf_label_band; no reference counterpart): the 6-connected components of
! the interior points with mask == 1 (e.g. phiSB of narrowBand, or the mask evolveBand
! returns) on one side of phi = iso.  side = 0: the cells with phi - iso < 0, 1: all other
! cells (phi == iso included), 2: both classes, never mixed in one component.  label
! (INTEGER, phi's shape) receives at every such cell the 0-based point index
! i + (nx+1)*(j + (ny+1)*k) of the smallest point of its component, -1 at a list cell of
! the class left out; every other point keeps what it held.  phi and mask are read only.
! ncomp receives the number of components.  Prints the list cells, the labelled cells,
! the components of each class and the passes, and says when the passes ran out before
! the labels were certified (they are then a refinement of the components).
!*************************************************************************************!
SUBROUTINE labelBand(phi,mask,label,nx,ny,nz,iso,side,ncomp)

INTEGER,INTENT(IN) :: nx,ny,nz,side
REAL,INTENT(IN) :: iso
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: mask
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: label
INTEGER,INTENT(OUT) :: ncomp
INTEGER(c_int64_t) :: info(8),nc
INTEGER(c_int) :: rc

info = 0
nc = 0
CALL lsf_set_mirror()
rc = lsf_label_band(phi,mask,label,nx,ny,nz,iso,side,64,c_null_ptr,0,nc,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_label_band',rc)
ncomp = INT(nc)
PRINT*, " Components on the band: list cells ",info(1),", labelled ",info(2),", inside ",info(3),", outside ",info(4), &
        ", passes ",info(5)
IF (info(6) > 0) PRINT*, " Components on the band: ",info(6)," links were still found by the last pass: a refinement"
PRINT*

END SUBROUTINE labelBand

!*************************************************************************************!
! The field at arbitrary points (include/lsf.h: lsf_sample_points; no reference
! counterpart): val = phi and grad = its gradient at the npts points pts(npts,3) -- the
! layout of surfX, so the nodes of extractSurface plug in -- interpolated trilinearly
! (order = 0) or by Catmull-Rom cubics (order = 1, linear in the cells next to the walls).
! iters >= 1: foot(npts,3) receives the foot of each point on phi = iso (both sides), by
! at most iters steps along the interpolant's gradient, converged when
! |phi - iso| <= tol*dx; iters = 0 leaves foot alone.  status(t): 0 OK, 1 outside the
! grid, 2 off the band, 3 flat, 4 not converged; a refused point holds NaN.  mask: only
! stencils of interior points with mask == 1 are sampled.  q, qval: a second field and
! its values at the points.  phi, mask, q and pts are read only.  Prints the counts.
!*************************************************************************************!
SUBROUTINE samplePoints(phi,nx,ny,nz,dx,xLo,pts,npts,order,iso,iters,tol,val,grad,foot,status,mask,q,qval)

INTEGER,INTENT(IN) :: nx,ny,nz,order,iters
INTEGER*4,INTENT(IN) :: npts
REAL,INTENT(IN) :: dx,xLo(3),iso,tol
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
REAL,INTENT(IN) :: pts(npts,3)
REAL,INTENT(OUT) :: val(npts),grad(npts,3)
REAL,INTENT(INOUT),TARGET :: foot(npts,3)
INTEGER*4,INTENT(OUT) :: status(npts)
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: q
REAL,INTENT(OUT),OPTIONAL,TARGET :: qval(npts)
TYPE(c_ptr) :: pm,pq,pqv,pf
INTEGER(c_int64_t) :: info(6)
INTEGER(c_int) :: rc

pm = c_null_ptr
pq = c_null_ptr
pqv = c_null_ptr
pf = c_null_ptr
IF (PRESENT(mask)) pm = C_LOC(mask)
IF (PRESENT(q)) pq = C_LOC(q)
IF (PRESENT(qval)) pqv = C_LOC(qval)
IF (iters >= 1) pf = C_LOC(foot)
info = 0
CALL lsf_set_mirror()
rc = lsf_sample_points(phi,pm,pq,nx,ny,nz,dx,xLo,pts,npts,order,iso,iters,tol,val,grad,pqv,pf,status,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_sample_points',rc)
PRINT*, " Samples: points ",npts,", ok ",info(1),", outside ",info(2)
PRINT*, " Samples: off the band ",info(3),", linear fallbacks ",info(4)
IF (iters >= 1) PRINT*, " Samples: flat ",info(5),", not converged ",info(6)
PRINT*

END SUBROUTINE samplePoints

!*************************************************************************************!
! The first hit of a ray with the level set (include/lsf.h: lsf_cast_rays; no reference
! counterpart): ray r starts at org(r,:) and runs along dir(r,:), any length -- the
! layout of surfX, so the nodes of extractSurface and grad of samplePoints plug in.  It
! is followed from the length tmin to tmax in steps of safety*|phi - iso|, kept between
! smin and smax cells, over the interpolant of samplePoints (order = 0 trilinear, 1
! Catmull-Rom); the first sign change is bisected refine times.  thit(r): the length to
! the hit; hit(r,:), grad(r,:): the point and the gradient there.  status(r): 0 hit,
! 1 miss, 2 the ray does not meet the grid, 3 not a ray, 4 lost (the surface was crossed
! where the list has no cells), 5 more than max_steps steps; a ray that is not hit holds
! NaN.  mask: only stencils of interior points with mask == 1 are sampled, the rest is
! crossed in strides of skip cells.  q, qval: a second field and its values at the hits.
! phi, mask, q, org and dir are read only.  Prints the counts.
!*************************************************************************************!
SUBROUTINE castRays(phi,nx,ny,nz,dx,xLo,org,dir,nrays,order,iso,tmin,tmax,safety,smin,smax,skip,refine,max_steps, &
                    thit,hit,grad,status,mask,q,qval)

INTEGER,INTENT(IN) :: nx,ny,nz,order,refine,max_steps
INTEGER*4,INTENT(IN) :: nrays
REAL,INTENT(IN) :: dx,xLo(3),iso,tmin,tmax,safety,smin,smax,skip
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
REAL,INTENT(IN) :: org(nrays,3),dir(nrays,3)
REAL,INTENT(OUT) :: thit(nrays),hit(nrays,3),grad(nrays,3)
INTEGER*4,INTENT(OUT) :: status(nrays)
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: mask
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: q
REAL,INTENT(OUT),OPTIONAL,TARGET :: qval(nrays)
TYPE(c_ptr) :: pm,pq,pqv
INTEGER(c_int64_t) :: info(9)
INTEGER(c_int) :: rc

pm = c_null_ptr
pq = c_null_ptr
pqv = c_null_ptr
IF (PRESENT(mask)) pm = C_LOC(mask)
IF (PRESENT(q)) pq = C_LOC(q)
IF (PRESENT(qval)) pqv = C_LOC(qval)
info = 0
CALL lsf_set_mirror()
rc = lsf_cast_rays(phi,pm,pq,nx,ny,nz,dx,xLo,org,dir,nrays,order,iso,tmin,tmax,safety,smin,smax,skip,refine,max_steps, &
                   thit,hit,grad,pqv,status,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_cast_rays',rc)
PRINT*, " Rays: rays ",nrays,", hit ",info(1),", miss ",info(2),", no grid ",info(3)
PRINT*, " Rays: bad ",info(4),", lost ",info(5),", out of steps ",info(6)
PRINT*, " Rays: samples ",info(7),", strides ",info(8),", began inside ",info(9)
PRINT*

END SUBROUTINE castRays

!*************************************************************************************!
! Points carried through the fields that move phi (include/lsf.h: lsf_advect_points; no
! reference counterpart -- advectNodes below is the reference's own surface-node scheme):
! pts(npts,3), the layout of surfX, moves in place along
!    x' = (u,v,w)(x) + speed(x) * grad phi(x) / |grad phi(x)|
! by nsteps steps of size dt (dt < 0 traces backwards) of TVD-RK3 (scheme = 0) or Euler
! (scheme = 1), over the interpolant of samplePoints (order = 0 trilinear, 1 Catmull-Rom).
! u, v, w come together or not at all; speed and phi come together; at least one group.
! status(t): 0 OK, 1 outside the grid, 2 off the band, 3 flat; a point that stops keeps the
! position of its last completed step.  cfl: the largest |dt*k|/dx over the completed
! steps.  The fields are read only.  Prints the counts.
!*************************************************************************************!
SUBROUTINE advectPoints(pts,npts,nx,ny,nz,dx,xLo,order,scheme,dt,nsteps,status,cfl,u,v,w,phi,speed,mask)

INTEGER,INTENT(IN) :: nx,ny,nz,order,scheme,nsteps
INTEGER*4,INTENT(IN) :: npts
REAL,INTENT(IN) :: dx,xLo(3),dt
REAL,INTENT(INOUT) :: pts(npts,3)
INTEGER*4,INTENT(OUT) :: status(npts)
REAL,INTENT(OUT) :: cfl
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: u,v,w,phi,speed
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: mask
TYPE(c_ptr) :: pu,pv,pw,pp,ps,pm
INTEGER(c_int64_t) :: info(6)
INTEGER(c_int) :: rc

pu = c_null_ptr
pv = c_null_ptr
pw = c_null_ptr
pp = c_null_ptr
ps = c_null_ptr
pm = c_null_ptr
IF (PRESENT(u)) pu = C_LOC(u)
IF (PRESENT(v)) pv = C_LOC(v)
IF (PRESENT(w)) pw = C_LOC(w)
IF (PRESENT(phi)) pp = C_LOC(phi)
IF (PRESENT(speed)) ps = C_LOC(speed)
IF (PRESENT(mask)) pm = C_LOC(mask)
info = 0
cfl = 0.
CALL lsf_set_mirror()
rc = lsf_advect_points(pu,pv,pw,pp,ps,pm,nx,ny,nz,dx,xLo,pts,npts,order,scheme,dt,nsteps,status,cfl,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_advect_points',rc)
PRINT*, " Points: points ",npts,", ok ",info(1),", outside ",info(2)
PRINT*, " Points: off the band ",info(3),", flat ",info(4)
PRINT*, " Points: steps made ",info(5),", linear fallbacks ",info(6),", CFL ",cfl
PRINT*

END SUBROUTINE advectPoints

!*************************************************************************************!
! The correction of the particle level set (include/lsf.h: lsf_correct_field; no reference
! counterpart): phi, in place, is rebuilt around every marker that has escaped.  pts(npts,3)
! are the markers, rad(npts) their radii with the side in the sign (> 0: the marker belongs
! where phi > 0).  A marker with phi on the wrong side by more than slack times its radius
! offers s*(r - distance) to the 8 corners of its cell; the largest offer of the positive
! markers and the smallest of the negative ones are merged by magnitude.  status(t):
! 0 in place, 1 escaped, 2 outside the grid, 3 off the band, 4 non-finite phi, 5 bad radius.
! change: the largest |new - old|.  mask: only cells with mask == 1 are corrected.  The
! result does not depend on the order of the markers.  Prints the counts.
!*************************************************************************************!
SUBROUTINE correctField(phi,nx,ny,nz,dx,xLo,pts,rad,npts,slack,status,change,mask)

INTEGER,INTENT(IN) :: nx,ny,nz
INTEGER*4,INTENT(IN) :: npts
REAL,INTENT(IN) :: dx,xLo(3),slack
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(INOUT) :: phi
REAL,INTENT(IN) :: pts(npts,3),rad(npts)
INTEGER*4,INTENT(OUT) :: status(npts)
REAL,INTENT(OUT) :: change
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: mask
TYPE(c_ptr) :: pm
INTEGER(c_int64_t) :: info(7)
INTEGER(c_int) :: rc

pm = c_null_ptr
IF (PRESENT(mask)) pm = C_LOC(mask)
info = 0
change = 0.
CALL lsf_set_mirror()
rc = lsf_correct_field(phi,pm,nx,ny,nz,dx,xLo,pts,rad,npts,slack,status,change,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_correct_field',rc)
PRINT*, " Correction: markers ",npts,", in place ",info(1),", escaped ",info(2)
PRINT*, " Correction: outside ",info(3),", off the band ",info(4)
PRINT*, " Correction: non-finite ",info(5),", bad radius ",info(6)
PRINT*, " Correction: points changed ",info(7),", largest change ",change
PRINT*

END SUBROUTINE correctField

!*************************************************************************************!
! The maintenance of the marker population (include/lsf.h: lsf_reseed_points; no reference
! counterpart): the old markers pts(npts,3), rad(npts) that are still usable are kept with
! their radius refreshed, every cell next to the surface with fewer than per_cell of them
! is topped up with new markers attracted to a random level on their own side, and the
! compacted set is kept on the device: nout is its size, reseedGet copies it out.
! npts = 0 seeds from scratch.  status(t) of the INPUT markers: 0 kept, 1 outside the grid,
! 2 off the band, 3 non-finite phi, 4 bad radius, 5 farther than band*dx from the surface.
! order: 0 linear, 1 cubic.  seed: INTEGER(c_int64_t), its bits taken as they are; vary it
! from reseed to reseed.  phi is read only.  Prints the counts.
!*************************************************************************************!
SUBROUTINE reseedPoints(phi,nx,ny,nz,dx,xLo,pts,rad,npts,per_cell,rmin,rmax,band,order,iters,tol,seed,status,nout,mask)

INTEGER,INTENT(IN) :: nx,ny,nz,per_cell,order,iters
INTEGER*4,INTENT(IN) :: npts
REAL,INTENT(IN) :: dx,xLo(3),rmin,rmax,band,tol
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
REAL,INTENT(IN) :: pts(npts,3),rad(npts)
INTEGER(c_int64_t),INTENT(IN) :: seed
INTEGER*4,INTENT(OUT) :: status(npts)
INTEGER*4,INTENT(OUT) :: nout
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN),OPTIONAL,TARGET :: mask
TYPE(c_ptr) :: pm
INTEGER(c_int64_t) :: info(14)
INTEGER(c_int) :: rc

pm = c_null_ptr
IF (PRESENT(mask)) pm = C_LOC(mask)
info = 0
nout = 0
CALL lsf_set_mirror()
rc = lsf_reseed_points(phi,pm,nx,ny,nz,dx,xLo,pts,rad,npts,per_cell,rmin,rmax,band,order,iters,tol,seed,status,nout,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_reseed_points',rc)
PRINT*, " Reseed: markers in ",npts,", kept ",info(1),", outside ",info(2),", off the band ",info(3)
PRINT*, " Reseed: non-finite ",info(4),", bad radius ",info(5),", far ",info(6)
PRINT*, " Reseed: eligible cells ",info(7),", candidates ",info(8),", accepted ",info(9)
PRINT*, " Reseed: over-full cells ",info(12),", largest count ",info(13),", markers out ",nout
PRINT*

END SUBROUTINE reseedPoints

!*************************************************************************************!
! The marker set kept by reseedPoints -> pts_out(nout,3), rad_out(nout), src_out(nout)
! (the 1-based input position of a kept marker, 0 for a new one); the kept set is released.
!*************************************************************************************!
SUBROUTINE reseedGet(pts_out,rad_out,src_out,nout)

INTEGER*4,INTENT(IN) :: nout
REAL,INTENT(OUT) :: pts_out(nout,3),rad_out(nout)
INTEGER*4,INTENT(OUT) :: src_out(nout)
INTEGER(c_int) :: rc

rc = lsf_reseed_get(pts_out,rad_out,src_out)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_reseed_get',rc)

END SUBROUTINE reseedGet

!*************************************************************************************!
! Order-8 gradients on the stencil band + node advection: set3d.f90:470-501 as one call
! (SURVEY.md section 8f rank 3).  surfXX holds the surface nodes on entry (set3d.f90:485).
!*************************************************************************************!
SUBROUTINE advectNodes(phi,phiSB,nx,ny,nz,dx,xLo,surfXX,nSurfNode,iter)

INTEGER,INTENT(IN) :: nx,ny,nz,iter
INTEGER*4,INTENT(IN) :: nSurfNode
REAL,INTENT(IN) :: dx,xLo(3)
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
INTEGER,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phiSB
REAL,INTENT(INOUT) :: surfXX(nSurfNode,3)
INTEGER(c_int) :: rc

CALL lsf_set_mirror()
rc = lsf_advect_nodes(phi,phiSB,nx,ny,nz,dx,xLo,surfXX,nSurfNode,iter)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_advect_nodes',rc)

END SUBROUTINE advectNodes

!*************************************************************************************!
! Run-time overrides of the host's hard-coded parameters (set3d.f90:140,148,298,390,576)
! needed by every BASELINE configuration except the as-shipped one.
!*************************************************************************************!
SUBROUTINE lsf_env_real(name,val)
CHARACTER(LEN=*), INTENT(IN) :: name
REAL, INTENT(INOUT) :: val
CHARACTER(LEN=64) :: v
INTEGER :: st,ios
REAL :: t
CALL lsf_load_inputs()
IF (name == 'LSF_DX' .AND. nml_dx > 0.) THEN
   val = nml_dx
   PRINT*, " dx = ",val," (namelist)"
END IF
CALL get_environment_variable(name,v,STATUS=st)
IF (st /= 0) RETURN
READ(v,*,IOSTAT=ios) t
IF (ios == 0) THEN
   val = t
   PRINT*, " ",name," = ",val," (environment override)"
END IF
END SUBROUTINE lsf_env_real

SUBROUTINE lsf_env_int(name,val)
CHARACTER(LEN=*), INTENT(IN) :: name
INTEGER, INTENT(INOUT) :: val
CHARACTER(LEN=64) :: v
INTEGER :: st,ios,t
CALL lsf_load_inputs()
t = -1
IF (name == 'LSF_DD') t = nml_dd
IF (name == 'LSF_REINIT_ITER') t = nml_reinit_iter
IF (name == 'LSF_MINMAX_ITER') t = nml_minmax_iter
IF (name == 'LSF_REINIT2_ITER') t = nml_reinit2_iter
IF (t >= 0) THEN
   val = t
   PRINT*, " ",name(5:)," = ",val," (namelist)"
END IF
CALL get_environment_variable(name,v,STATUS=st)
IF (st /= 0) RETURN
READ(v,*,IOSTAT=ios) t
IF (ios == 0) THEN
   val = t
   PRINT*, " ",name," = ",val," (environment override)"
END IF
END SUBROUTINE lsf_env_int

!*************************************************************************************!
! Pad cells per axis and side (host edit E4b; set3d.f90:148-157 pads every side by dd).
! BASELINE configuration 3 asks for a cubic 512^3 grid around a 12 x 1 x 1 bounding box.
!*************************************************************************************!
SUBROUTINE lsf_pad_cells(dd,ddLo,ddHi)
INTEGER, INTENT(IN) :: dd
INTEGER, INTENT(OUT) :: ddLo(3),ddHi(3)
CHARACTER(LEN=1), PARAMETER :: ax(3) = (/'X','Y','Z'/)
INTEGER :: a
CALL lsf_load_inputs()
ddLo = dd
ddHi = dd
DO a = 1,3
   IF (nml_dd_lo(a) >= 0) ddLo(a) = nml_dd_lo(a)
   IF (nml_dd_hi(a) >= 0) ddHi(a) = nml_dd_hi(a)
   CALL lsf_env_int('LSF_DD_'//ax(a)//'_LO',ddLo(a))
   CALL lsf_env_int('LSF_DD_'//ax(a)//'_HI',ddHi(a))
END DO
END SUBROUTINE lsf_pad_cells

!*************************************************************************************!
! Device-resident chain (include/lsf.h: lsf_mirror).  The host program hands the same
! arrays from seam to seam and never changes them in between; with resident = 2 the
! library keeps them on the device and the four places where the host itself reads phi
! between the seams go through the library as well (host edits E8, E9):
!   snapshotPhi   phiO = phi                        set3d.f90:311
!   sumSqDiff     the asymptotic-error loop         set3d.f90:510-516
!   writeVti      the two VTK writers               set3d.f90:336-351, :554-569
!   syncHost      brings a host array up to date (after the last seam)
!*************************************************************************************!
SUBROUTINE lsf_set_mirror()
INTEGER :: resident,st,ios,t
INTEGER(c_int) :: rc
CHARACTER(LEN=64) :: v
IF (mirror_set) RETURN
mirror_set = .TRUE.
CALL lsf_load_inputs()
resident = 2
IF (nml_resident >= 0) resident = nml_resident
CALL get_environment_variable('LSF_RESIDENT',v,STATUS=st)
IF (st == 0) THEN
   READ(v,*,IOSTAT=ios) t
   IF (ios == 0) resident = t
END IF
rc = 0
IF (resident == 1) rc = lsf_mirror(1_c_int)
IF (resident >= 2) rc = lsf_mirror(3_c_int)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_mirror',rc)
END SUBROUTINE lsf_set_mirror

SUBROUTINE snapshotPhi(phi,phiO,nx,ny,nz)
INTEGER, INTENT(IN) :: nx,ny,nz
REAL, INTENT(IN) :: phi(0:nx,0:ny,0:nz)
REAL, INTENT(INOUT) :: phiO(0:nx,0:ny,0:nz)
INTEGER(c_int) :: rc
CALL lsf_set_mirror()
rc = lsf_snapshot(phi,phiO,nx,ny,nz)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_snapshot',rc)
END SUBROUTINE snapshotPhi

SUBROUTINE sumSqDiff(phi,phiO,nx,ny,nz,s)
INTEGER, INTENT(IN) :: nx,ny,nz
REAL, INTENT(IN) :: phi(0:nx,0:ny,0:nz),phiO(0:nx,0:ny,0:nz)
REAL, INTENT(INOUT) :: s
REAL(c_double) :: t
INTEGER(c_int) :: rc
CALL lsf_set_mirror()
rc = lsf_sumsq_diff(phi,phiO,nx,ny,nz,t)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_sumsq_diff',rc)
s = s + t
END SUBROUTINE sumSqDiff

SUBROUTINE writeVti(name,phi,nx,ny,nz,dx,xLo)
CHARACTER(LEN=*), INTENT(IN) :: name
INTEGER, INTENT(IN) :: nx,ny,nz
REAL, INTENT(IN) :: phi(0:nx,0:ny,0:nz),dx,xLo(3)
INTEGER(c_int) :: rc
CHARACTER(KIND=c_char) :: cname(LEN_TRIM(name)+1)
INTEGER :: i
CALL lsf_set_mirror()
DO i = 1,LEN_TRIM(name)
   cname(i) = name(i:i)
END DO
cname(LEN_TRIM(name)+1) = c_null_char
rc = lsf_write_vti(cname,phi,nx,ny,nz,dx,xLo)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_write_vti',rc)
END SUBROUTINE writeVti

SUBROUTINE syncHost(a)
REAL, INTENT(INOUT), TARGET :: a(*)
INTEGER(c_int) :: rc
rc = lsf_mirror_sync(c_loc(a))
IF (rc /= LSF_OK) CALL lsf_fail('lsf_mirror_sync',rc)
END SUBROUTINE syncHost

! the array is about to be freed (or its device copy is of no further use): drop its twin without a copy
SUBROUTINE forgetHost(a)
REAL, INTENT(INOUT), TARGET :: a(*)
INTEGER(c_int) :: rc
rc = lsf_mirror_forget(c_loc(a))
IF (rc /= LSF_OK) CALL lsf_fail('lsf_mirror_forget',rc)
END SUBROUTINE forgetHost

SUBROUTINE syncHostInt(a)
INTEGER, INTENT(INOUT), TARGET :: a(*)
INTEGER(c_int) :: rc
rc = lsf_mirror_sync(c_loc(a))
IF (rc /= LSF_OK) CALL lsf_fail('lsf_mirror_sync',rc)
END SUBROUTINE syncHostInt

!*************************************************************************************!
! The level set phi = iso as a triangle mesh (include/lsf.h: lsf_extract_surface; no
! reference counterpart): marching tetrahedra on the six Kuhn tetrahedra of every cell,
! made on the device.  surfX(nSurfNode,3) and surfElem(nSurfElem,3) are allocated here, as
! stlRead allocates them, in the format meshDistance and phi0Init take; normals point
! towards phi >= iso.  An empty level set gives nSurfNode = nSurfElem = 0 and arrays of
! zero rows.  phi is read only.
!*************************************************************************************!
SUBROUTINE extractSurface(phi,nx,ny,nz,dx,xLo,iso,surfX,nSurfNode,surfElem,nSurfElem)

INTEGER,INTENT(IN) :: nx,ny,nz
REAL,INTENT(IN) :: dx,xLo(3),iso
REAL,DIMENSION(0:nx,0:ny,0:nz),INTENT(IN) :: phi
REAL,ALLOCATABLE,DIMENSION(:,:),INTENT(OUT) :: surfX
INTEGER*4,ALLOCATABLE,DIMENSION(:,:),INTENT(OUT) :: surfElem
INTEGER*4,INTENT(OUT) :: nSurfNode,nSurfElem
INTEGER(c_int64_t) :: info(4)
INTEGER(c_int) :: rc

CALL lsf_set_mirror()
rc = lsf_extract_surface(phi,nx,ny,nz,dx,xLo,iso,nSurfNode,nSurfElem,info)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_extract_surface',rc)
ALLOCATE(surfX(nSurfNode,3))
ALLOCATE(surfElem(nSurfElem,3))
rc = lsf_extract_get(surfX,surfElem)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_extract_get',rc)
PRINT*, " Surface extraction: ",nSurfNode," nodes, ",nSurfElem," triangles, ",info(3)," cells crossed"
PRINT*

END SUBROUTINE extractSurface

!*************************************************************************************!
! Binary STL of a mesh (include/lsf.h: lsf_stl_write): what stlRead reads back.
!*************************************************************************************!
SUBROUTINE stlWrite(surfX,nSurfNode,surfElem,filename,nSurfElem)

INTEGER*4,INTENT(IN) :: nSurfNode,nSurfElem
REAL,INTENT(IN) :: surfX(nSurfNode,3)
INTEGER*4,INTENT(IN) :: surfElem(nSurfElem,3)
CHARACTER(LEN=*), INTENT(IN) :: filename
INTEGER(c_int) :: rc
CHARACTER(KIND=c_char) :: cname(LEN_TRIM(filename)+1)
INTEGER :: i

DO i = 1,LEN_TRIM(filename)
   cname(i) = filename(i:i)
END DO
cname(LEN_TRIM(filename)+1) = c_null_char
rc = lsf_stl_write(cname,surfX,nSurfNode,surfElem,nSurfElem)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_stl_write',rc)

END SUBROUTINE stlWrite

!*************************************************************************************!
! Read STL and Allocate  (same dummy arguments as subs.f90:17; host edit E11)
! The reference merges repeated vertices with a linear search per vertex (quadratic);
! lsf_stl_read returns the same nodes and connectivity from a hash (include/lsf.h).
!*************************************************************************************!
SUBROUTINE stlRead(surfX,nSurfNode,surfElem,filename,nSurfElem,surfElemTag,surfOrder,nBndComp,nBndElem,bndNormal)
CHARACTER, INTENT(IN) :: filename*80
INTEGER*4 nSurfNode,nSurfElem
INTEGER*4,ALLOCATABLE,DIMENSION(:,:),INTENT(OUT) :: surfElem
REAL,ALLOCATABLE,DIMENSION(:,:),INTENT(OUT) :: surfX
INTEGER,ALLOCATABLE,DIMENSION(:),INTENT(OUT) :: surfElemTag,surfOrder
REAL,ALLOCATABLE,DIMENSION(:,:),INTENT(OUT) :: bndNormal
INTEGER,INTENT(OUT) :: nBndComp,nBndElem
INTEGER(c_int) :: rc
CHARACTER(KIND=c_char) :: cname(LEN_TRIM(filename)+1)
INTEGER :: i

PRINT*
PRINT*, " Reading in .stl Mesh "
PRINT*

DO i = 1,LEN_TRIM(filename)
   cname(i) = filename(i:i)
END DO
cname(LEN_TRIM(filename)+1) = c_null_char
rc = lsf_stl_read(cname,nSurfElem,nSurfNode)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_stl_read',rc)
ALLOCATE(surfElem(nSurfElem,3))
ALLOCATE(surfX(nSurfNode,3))
rc = lsf_stl_get(surfX,surfElem)
IF (rc /= LSF_OK) CALL lsf_fail('lsf_stl_get',rc)

! subs.f90:108-118 (the reference allocates bndNormal before it sets nBndComp; one component is what it means)
nBndComp = 1
nBndElem = 0
ALLOCATE(surfOrder(nSurfElem))
ALLOCATE(surfElemTag(nSurfElem))
ALLOCATE(bndNormal(nBndComp,3))
surfOrder = 1
surfElemTag = 0
bndNormal = 0.

END SUBROUTINE stlRead

END MODULE lsf_hip
