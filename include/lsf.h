/*
 * lsf.h -- C ABI of liblsf_hip.so: the MI355X (gfx950) implementation of the hot path of
 * musheen/LevelSetFortran -- WENO5 Hamilton-Jacobi reinitialisation and min/max-flow smoothing
 * on a uniform 3-D grid.
 *
 * The reference has no FFI: its seam is the Fortran module procedure `reinit`
 * (subs.f90:717-725, called at set3d.f90:308 and :582) and the min/max loop written inline in the
 * main program (set3d.f90:394-462).  Each entry point below names the reference interface it
 * replaces.  levelsetfortran_amd/fortran/lsf_hip.f90 is the iso_c_binding shim that gives
 * the reference host those procedures back under their original names.
 *
 * Conventions
 *  - Plain C types only.  `int` is the reference's INTEGER*4, `double` its REAL under
 *    -fdefault-real-8 (Makefile:4).
 *  - Every field is Fortran-ordered exactly like `REAL phi(0:nx,0:ny,0:nz)` (subs.f90:721):
 *    extents (nx+1, ny+1, nz+1), `i` unit stride, element (i,j,k) at i + (nx+1)*(j + (ny+1)*k).
 *  - Functions without a `_device` suffix take HOST pointers owned by the caller; the library
 *    copies in on entry and out on exit and is quiescent on return.  `_device` functions take
 *    DEVICE pointers (HBM-resident fields, e.g. torch tensors) and a hipStream_t passed as void*
 *    (NULL = the null stream); they enqueue work and, unless stated otherwise, return after the
 *    stream has been synchronised.
 *  - All functions return LSF_OK (0) or an LSF_ERR_* code; lsf_last_error() describes the last
 *    failure on the calling thread.  There is no CPU fallback: without a usable gfx950 device the
 *    compute entry points return LSF_ERR_NO_DEVICE.
 */
#ifndef LSF_H
#define LSF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSF_VERSION 106 /* 0.1.6: lsf_copy_bandwidth (measurement aid); the argument block of the exact-ordering kernels no longer carries experiment fields */

/* ---- return codes ---------------------------------------------------------------------- */
#define LSF_OK 0
#define LSF_ERR_NAN 1       /* RMS became NaN: the reference STOPs (subs.f90:926, set3d.f90:458) */
#define LSF_ERR_INVALID 2   /* bad argument                                                      */
#define LSF_ERR_HIP 3       /* HIP runtime failure                                               */
#define LSF_ERR_NO_DEVICE 4 /* no HIP device / not gfx950                                        */

/* ---- mode word: ordering | arithmetic ---------------------------------------------------- */
/* ordering (low byte) */
#define LSF_ORDER_GS 0     /* the reference's in-place Gauss-Seidel raster sweeps, reproduced      \
                              exactly by a tiled hyperplane wavefront     */
#define LSF_ORDER_JACOBI 1 /* double-buffered sweep: shards across GPUs, NOT reference-equal       */
#define LSF_ORDER_MASK 0xff
/* arithmetic (bit 8) */
#define LSF_ARITH_FAST 0x000   /* restructured fp64 arithmetic (FMA, shared terms, one reciprocal   \
                                  per WENO side): ~1e-16 per sweep from LSF_ARITH_STRICT, within   \
                                  1e-12 RMS of it for a thousand sweeps; over thousands of sweeps  \
                                  the scheme itself amplifies any rounding difference at kinks of  \
                                  the surface (isolated cells up to 1e-5 apart)  */
#define LSF_ARITH_STRICT 0x100 /* every operation as written in subs.f90, no contraction:           \
                                  bit-identical to the reference for LSF_ORDER_GS (the default of  \
                                  the Fortran shim); 1.8 x the time of LSF_ARITH_FAST              */
/* Operand range of the bit-identity promise of LSF_ARITH_STRICT.  The divisions by dx (subs.f90:509-530) and the weight
 * divisions (:536-546) are carried out by the hardware's division sequence WITHOUT its rescaling frame, which is the IEEE
 * quotient as long as numerator, divisor and quotient are normal numbers away from the ends of the exponent range: pinned
 * for fields and grid spacings scaled from 1e-140 to 1e140 (tests/test_gpu_parity.py, ..._at_the_ends_of_the_exponent_range)
 * and by 1.7e10 random quotients (profiles/micro/divcheck.hip); the weight divisions fall back to the framed division when
 * eps + IS >= 1e120.  Outside that range -- a difference of phi values divided by dx whose quotient is subnormal or
 * overflows, an infinite phi -- the last bit, or inf against NaN, may differ from the reference; such a field is already
 * outside anything a distance function holds (|phi| <= a few domain lengths, dx >= 1e-100 of it). */

/* ---- library / device ------------------------------------------------------------------- */
int lsf_version(void);
const char *lsf_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int lsf_device_count(void);
/* select the device used by the calling thread's subsequent calls (default 0) */
int lsf_set_device(int device);
/* release every cached device buffer of the current device */
int lsf_release_workspace(void);
/* Measurement aid (bench.py): with profiling enabled the next lsf_reinit*_ call brackets, per sweep,
 * the sweep kernel(s), the boundary-condition kernel and the RMS/stop kernel with HIP events on the
 * stream they are launched on.  lsf_profile_get returns the sums over the sweeps of that call (ms),
 * the number of sweep-kernel launches and the number of sweeps timed. */
/* diagnostic: 1 when the 16-byte loads / stores of the exact-ordering tiles (one raw buffer descriptor of 2^31 - 1 bytes per
 * tile image of rows_z + 6 planes) can address every point of a tile on an (nx, ny) grid; the kernels test the same expression. */
int lsf_skew_wide_fits(int nx, int ny, int rows_z);
int lsf_profile(int enable);
/* Measurement aid (bench.py "roofline.peak_measured", SURVEY.md section 8d: the roofline "also against a measured device-copy
 * bandwidth"): copies `bytes` bytes (>= 1 MiB, a multiple of 16) between two fresh device buffers reps + 1 times with a
 * streaming kernel (16 bytes per lane and access) and returns the rate of the fastest timed pass in GB/s, counting the bytes
 * read AND the bytes written.  No reference counterpart. */
int lsf_copy_bandwidth(size_t bytes, int reps, double *gbps);
int lsf_profile_get(double *sweep_kernel_ms, double *bc_ms, double *finish_ms,
                    long long *sweep_kernel_launches, int *sweeps);
/* name of the sweep kernel the last profiled call launched (the exact ordering picks its tile shape by
 * grid size); "" before the first profiled call.  The string is static. */
const char *lsf_profile_kernel(void);

/* ---- seam 1: reinit ----------------------------------------------------------------------
 * Replaces SUBROUTINE reinit(phi,gradPhi,gradPhiMag,nx,ny,nz,iter,dx,h), subs.f90:717-931.
 * Runs at most iter+1 sweeps (the reference loop is DO n=0,iter, subs.f90:735) of
 * {one raster sweep of the WENO5/Godunov update (subs.f90:743-852, weno :489-711, phiSign
 * :152-172); extrapolation boundary condition (:859-897); RMS change over all points (:902-914)}
 * and stops after the first sweep whose RMS is < tol (the reference uses 1e-5, :915).
 * gradPhi / gradPhiMag are dead outputs of the reference and are not part
 * of this interface.
 *   sweeps_done  (out, may be NULL) number of sweeps executed
 *   rms_trace    (out, may be NULL) RMS of sweep s (0-based) in rms_trace[s], s < trace_cap; the
 *                Fortran shim prints the reference's " Iteration: n  RMS Error: e" lines from it
 * Returns LSF_ERR_NAN if an RMS is NaN (phi then holds the state after that sweep).
 */
int lsf_reinit(double *phi, int nx, int ny, int nz, int iter, double dx, double h, double tol,
               int mode, int *sweeps_done, double *rms_trace, int trace_cap);

/* Same on an HBM-resident field.  d_phi is updated in place.  first_raster (0..7) is the number
 * of raster directions already consumed (0 = start with scan 1, like the reference); d_phiS may be
 * NULL (then phiS = phi on entry, subs.f90:731) or a device copy of the sign field to use. */
int lsf_reinit_device(double *d_phi, const double *d_phiS, int nx, int ny, int nz, int iter, double dx,
                      double h, double tol, int mode, int first_raster, int *sweeps_done,
                      double *rms_trace, int trace_cap, void *stream);

/* ---- narrow-band (tube) reinitialisation: reinit on the cells of a caller's mask only -------------
 * No reference counterpart: the reference's reinit visits every interior cell, although the stages behind it (min/max flow,
 * order-8 gradients, node advection) read phi only where phiNB / phiSB are 1.
 *   LIST     the interior points (1..n-1 in each axis) with mask == 1 on entry, fixed for the whole call.  Any other mask
 *            value means "not in the band"; a 1 on a wall point is ignored.  The mask is read once and never written.
 *   phiS     phi on entry (subs.f90:731), or d_phiS when given (device seam); only its list cells are read.
 *   a sweep  every list cell becomes phi + h * sgn * (1 - gM) (subs.f90:747-750; weno :489-711; phiSign :152-172) with all 19
 *            stencil values taken from the field as it was at the start of the sweep (the Jacobi ordering).  Cells 4..n-5 take
 *            WENO5, the others first-order differences, as in lsf_reinit.  Points outside LIST are NEVER written, wall points
 *            included: the extrapolation boundary condition (subs.f90:859-897) is NOT applied.
 *   RMS      sqrt(sum over list cells (new - old)^2 / nL), nL = length of LIST, summed in a fixed order (reproducible from run
 *            to run).  NOT comparable with lsf_reinit's RMS, which divides by nx*ny*nz.
 *   sweeps   at most iter+1; stops after the first sweep whose RMS is < tol (tol <= 0: never early).  A NaN RMS returns
 *            LSF_ERR_NAN and phi holds the state after that sweep.  sweeps_done / rms_trace / trace_cap as in lsf_reinit.
 *   empty    LIST empty: LSF_OK, sweeps_done = 0, nothing written.
 *   mode     LSF_ORDER_JACOBI | LSF_ARITH_FAST or | LSF_ARITH_STRICT.  LSF_ORDER_GS is LSF_ERR_INVALID: a raster order has
 *            no meaning on a list.  With LSF_ARITH_STRICT a sweep is, bit for bit, a full-grid Jacobi sweep whose result is
 *            kept at the list cells only.
 *   limits   a NULL mask, iter < 0, bad dims or more than 2^31 - 1 points are LSF_ERR_INVALID (list entries are 32-bit point
 *            indices, like the min/max band's).
 * Guidance: make the update mask WIDER than the band whose values are trusted.  List cells within three cells of the list's
 * edge read frozen neighbours.  On the cube40 fixture after min/max flow, against a full-grid Jacobi run: with phiSB
 * (|phi| < 8.1 dx) as the mask the cells with |phi| < 4.1 dx differ by 0 after 1 sweep, 1.8e-10 after 10, 1.2e-7 after 50 and
 * 8.8e-7 after 100; with phiNB (|phi| < 4.1 dx) itself as the mask by 2.9e-4 after 10 sweeps.
 * Work: beyond one pass over the mask and one copy of the field per call, nothing is proportional to the grid; a sweep visits
 * the list cells only.  No speed is claimed here (the measurement is profiles/micro/reinit_band_time.py), and there is no
 * automatic dispatch to the full-grid kernels of lsf_reinit. */
int lsf_reinit_band(double *phi, const int32_t *mask, int nx, int ny, int nz, int iter, double dx, double h,
                    double tol, int mode, int *sweeps_done, double *rms_trace, int trace_cap);
int lsf_reinit_band_device(double *d_phi, const double *d_phiS, const int32_t *d_mask, int nx, int ny, int nz,
                           int iter, double dx, double h, double tol, int mode, int *sweeps_done,
                           double *rms_trace, int trace_cap, void *stream);

/* ---- seam 2: min/max flow ---------------------------------------------------------------
 * Replaces the loop DO n = 1,iter ... END DO at set3d.f90:394-462 (secondDeriv subs.f90:370-407,
 * minMax subs.f90:413-483, narrowBand subs.f90:178-207), hoisted into one call.
 * phiNB / phiSB: in = the masks made at set3d.f90:360; out = the masks the host holds after the
 * loop (the band is refreshed only on the non-exit path, set3d.f90:448-460).
 * Stops after the first iteration whose RMS is < tol (reference 1e-7, set3d.f90:448).
 */
int lsf_minmax(double *phi, int32_t *phiNB, int32_t *phiSB, int nx, int ny, int nz, int iter,
               double dx, double h1, double tol, int mode, int *iters_done, double *rms_trace,
               int trace_cap);

int lsf_minmax_device(double *d_phi, int32_t *d_phiNB, int32_t *d_phiSB, int nx, int ny, int nz,
                      int iter, double dx, double h1, double tol, int mode, int *iters_done,
                      double *rms_trace, int trace_cap, void *stream);

/* ---- narrowBand --------------------------------------------------------------------------
 * Replaces SUBROUTINE narrowBand(nx,ny,nz,dx,phi,phiNB,phiSB), subs.f90:178-207. */
int lsf_narrowband(const double *phi, int32_t *phiNB, int32_t *phiSB, int nx, int ny, int nz,
                   double dx);
int lsf_narrowband_device(const double *d_phi, int32_t *d_phiNB, int32_t *d_phiSB, int nx, int ny,
                          int nz, double dx, void *stream);

/* ---- phi0: inside/outside initialisation (the step before the hot path) -------------------
 * Replaces the centroid table + search loop of the main program, set3d.f90:196-268 (SURVEY.md section 8f
 * rank 1): for every grid point within 3 cells of the surface bounding box, the nearest triangle centroid
 * (first minimum), the sign of the triple product of its vertex vectors, smeared by phiSign(pS,dx,1);
 * 1.0 elsewhere (set3d.f90:161).  surfX is the host's REAL surfX(nSurfNode,3), surfElem its
 * INTEGER*4 surfElem(nSurfElem,3) (1-based), both Fortran-ordered HOST arrays; xLo/minX/maxX as computed at
 * set3d.f90:94-157.  Bit-identical to the reference. */
int lsf_phi0(double *phi, int nx, int ny, int nz, double dx, const double xLo[3], const double minX[3],
             const double maxX[3], const double *surfX, int nSurfNode, const int32_t *surfElem,
             int nSurfElem);
int lsf_phi0_device(double *d_phi, int nx, int ny, int nz, double dx, const double xLo[3],
                    const double minX[3], const double maxX[3], const double *surfX, int nSurfNode,
                    const int32_t *surfElem, int nSurfElem, void *stream);

/* ---- exact signed distance from the triangle mesh, clamped to a tube -------------------------------
 * No reference counterpart: lsf_phi0 above restates the reference's inside/outside test (nearest CENTROID, a smeared +-1), which
 * carries no sub-cell position of the surface.  This is the distance to the triangles themselves.  surfX(nSurfNode,3) and
 * surfElem(nSurfElem,3) are 1-based Fortran-ordered HOST arrays exactly as lsf_phi0 takes them; the grid point (i,j,k) is
 * xLo + (i,j,k)*dx (set3d.f90:168-170).  info may be NULL.
 *   far      width * dx, computed once on the host.
 *   TUBE     the grid points, wall points included, whose distance to the nearest non-degenerate triangle is <= far.  A tube
 *            point receives the exact Euclidean point-to-triangle distance d (closest point over the face, edge and vertex
 *            regions, fp64), negative where the offset from the closest point has a negative dot product with the angle-weighted
 *            pseudonormal of the closest FEATURE: the face normal, the sum of the two unit face normals of an edge, the sum of
 *            the unit face normals weighted by their angles at a vertex.  A zero dot product counts as positive.
 *   ties     between triangles the smaller distance wins; at equal distance bits the positive sign wins.  The field is
 *            bit-identical from run to run and between the two seams.
 *   far      every other point receives +-far: the sign of the last tube point met when walking its (i,j) column from k = 0, and
 *   points   before the first tube point the exterior sign, + if the mesh's signed volume is >= 0, else -.  Correct because two
 *            neighbouring grid points on opposite sides of the surface are both within dx of it, hence both in the tube: this
 *            is why width >= 1.5 is required.  THE ONE ASSUMPTION: the k = 0 plane lies outside the body or inside the tube.
 *            The reference's grid pads 10 cells around the surface (set3d.f90:148-157), so there it always does.
 *   flags    LSF_MESH_UNSIGNED: no pseudonormals, no requirements on the mesh; tube points get d, all others +far.
 *   mesh     prepared on the host once per call.  A triangle with a zero-length normal is DEGENERATE: skipped, part of no
 *            pseudonormal.  An edge pseudonormal is computed once per edge, the lower triangle index first in the sum, and
 *            copied to both triangles; vertex sums run in triangle order.  An edge is DEFECTIVE unless exactly two
 *            non-degenerate triangles share it and traverse it in opposite directions.
 *   info     [0] tube points  [1] degenerate triangles skipped  [2] defective edges  [3] non-degenerate triangles whose padded
 *            box misses the grid.  Written on LSF_OK only.
 *   errors   LSF_ERR_INVALID, all detected before anything is written: width not finite or < 1.5, dx <= 0, bad dims, a NULL
 *            pointer, nSurfElem < 1, an index outside 1..nSurfNode, a non-finite coordinate, an unknown flag, and a SIGNED call
 *            on a mesh with defective edges (the message names their number; the unsigned call accepts such a mesh).  No device:
 *            LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   seams    lsf_mesh_distance treats the twin of phi exactly as lsf_phi0 does under lsf_mirror (phi is an output).
 * lsf_mesh_check is host code only and needs no device (like lsf_stl_read): info[1] and info[2] as above, info[0] = info[3] = 0,
 * and the signed volume sum(v0 . (v1 x v2)) / 6.
 * Guidance: the field is a CLAMPED distance, |phi| <= far.  lsf_reinit, lsf_narrowband, lsf_minmax and lsf_reinit_band take it as
 * it is (narrowBand's 4.1 dx / 8.1 dx bands want width > 8.1 to be read off the field directly; lsf_reinit grows the distance
 * outwards from any width).  Work: a triangle costs the points of its padded bounding box, (2*width)^3 for a small one, so a wider
 * tube is paid for per triangle; beyond one fill and one pass over the field nothing is proportional to the grid. */
#define LSF_MESH_UNSIGNED 1 /* flags */
#define LSF_MESH_INFO_LEN 4
int lsf_mesh_check(const double *surfX, int nSurfNode, const int32_t *surfElem, int nSurfElem,
                   int64_t info[LSF_MESH_INFO_LEN], double *signed_volume);
int lsf_mesh_distance(double *phi, int nx, int ny, int nz, double dx, const double xLo[3], const double *surfX,
                      int nSurfNode, const int32_t *surfElem, int nSurfElem, double width, int flags,
                      int64_t info[LSF_MESH_INFO_LEN]);
int lsf_mesh_distance_device(double *d_phi, int nx, int ny, int nz, double dx, const double xLo[3], const double *surfX,
                             int nSurfNode, const int32_t *surfElem, int nSurfElem, double width, int flags,
                             int64_t info[LSF_MESH_INFO_LEN], void *stream);

/* ---- distance fill: first-order fast sweeping outwards from a frozen band --------------------------
 * No reference counterpart.  Solves |grad phi| = 1 on every point that is not FROZEN, with the frozen points as boundary data, by
 * rounds of 8 in-place raster sweeps of the first-order Godunov update: what turns the clamped field of lsf_mesh_distance, or a
 * field that is trusted on a mask only, into a distance on the whole grid without the pseudo-time sweeps of lsf_reinit.  The field
 * layout is that of every other entry point.  rounds_done, changed_trace and frozen_points may be NULL.
 *   FROZEN   mask == NULL: the points, wall points included, with |phi| < far on entry; far = band * dx, computed once on the host.
 *            For a field of lsf_mesh_distance(width = w), band = w selects its tube.  With a mask: the points with mask == 1, and
 *            band is ignored.  The mask is read once and never written.  Frozen points are never written.
 *   sign     every other point keeps the sign it has on entry (phi < 0 is negative; anything else, -0.0 included, is positive);
 *            its magnitude is replaced.
 *   round    8 in-place raster sweeps over all points 0..n of each axis (walls are solved, not extrapolated), in the direction
 *            order of the reference's reinit (subs.f90:740-855): (+,+,+) (+,+,-) (+,-,-) (-,-,-) (-,+,-) (-,-,+) (-,+,+) (+,-,+).
 *            Non-frozen points start at +inf.
 *   visit    of a non-frozen point, u being the magnitudes as they are at that moment of the sweep:
 *              x = min(u(i-1), u(i+1)), likewise y and z; a neighbour outside the grid counts as +inf;
 *              a = min(min(x,y),z); c = max(max(x,y),z); b = max(min(x,y), min(max(x,y),z));
 *              a = +inf: nothing happens.  Otherwise t = a + dx;
 *              if t > b:     d = a - b; t = ((a + b) + sqrt(2*(dx*dx) - d*d)) * 0.5;
 *              if that t > c: t = (((a + b) + c) + sqrt(max(3*(dx*dx) - (((a-b)*(a-b) + (a-c)*(a-c)) + (b-c)*(b-c)), 0))) / 3;
 *              new = min(old, t).
 *            Evaluated exactly as written, left to right, without contraction; sqrt and / are the IEEE ones.
 *   trace    changed_trace[r], r < trace_cap: the number of visits of round r with new < old (an integer: no arrival order in it).
 *   stop     after the first round whose count is 0 (that round is counted) or after max_rounds; rounds_done = rounds run.
 *            Reaching max_rounds is LSF_OK: the caller reads the last trace entry.  After round 1 every point is finite.
 *   result   field, rounds_done and trace are those of the serial loops above, bit for bit, on both seams, on any stream, from
 *            run to run -- after every round, not only at the fixed point (tests/distance_fill_ref.py is that serial statement).
 *   errors   LSF_ERR_INVALID, all detected before phi is written, the offending count in lsf_last_error() where there is one:
 *            a NULL phi; nx, ny or nz < 1 or more than 2^31 - 1 points; dx not finite or <= 0; mask == NULL with band not finite
 *            or <= 0; max_rounds < 1; no frozen point; a non-finite value on a frozen point; two axis neighbours of opposite
 *            sign that are not both frozen (the frozen set must separate the signs).  No device: LSF_ERR_NO_DEVICE -- there is no
 *            CPU fallback.
 *   seams    lsf_distance_fill treats phi as in/out and the mask as an input under lsf_mirror exactly as lsf_reinit_band does.
 *            lsf_distance_fill_device returns after the stream is synchronised (the host reads one count per round).
 * Guidance: the scheme is FIRST ORDER away from the frozen set: against the closed forms of the test inputs the largest error far
 * from the surface is 0.98 - 1.65 dx (box and sphere, bands of 3.5 and 1.5 cells), growing with the distance travelled; the values
 * inside the band are the caller's, untouched.  That is enough for lsf_narrowband / lsf_minmax / lsf_write_vti when the band covers
 * what they read to full accuracy (band >= 8.1 for narrowBand's stencil band).  lsf_reinit afterwards is optional and shorter: on
 * the cube40 fixture at 62^3 the CPU oracle stops after 367 sweeps from the filled field, 565 from the clamped one (no other count
 * is promised).  Convergence took 2 - 4 rounds on the test inputs; a shape with many concave turns needs more.
 * Workspace beyond the caller's field: one bit per point -- a 32-bit word per 32 points of a row, rows padded to a whole word, i.e.
 * 4 * ceil((nx+1)/32) * (ny+1) * (nz+1) bytes -- plus 32 bytes of counters; no second copy of the field.  (Below one byte per point
 * for nx >= 3.)  Work: a round is 8 * (tiles_x + tiles_y + tiles_z - 2) dependent launches of 32 x 8 x 8-point tiles.
 * Not timed on hardware. */
int lsf_distance_fill(double *phi, const int32_t *mask, int nx, int ny, int nz, double dx, double band, int max_rounds,
                      int *rounds_done, int64_t *changed_trace, int trace_cap, int64_t *frozen_points);
int lsf_distance_fill_device(double *d_phi, const int32_t *d_mask, int nx, int ny, int nz, double dx, double band,
                             int max_rounds, int *rounds_done, int64_t *changed_trace, int trace_cap,
                             int64_t *frozen_points, void *stream);

/* ---- extension off the surface: a quantity carried constant along the normals of phi ----------
 * No reference counterpart.  Solves grad(q) . grad(phi) = 0 on every point that is not FROZEN, with q on the frozen points as boundary
 * data, by rounds of 8 in-place raster sweeps of the first-order upwind update in |phi| (extension velocities of Adalsteinsson and
 * Sethian in the fast-sweeping form of Zhao): what gives lsf_advect_field its `speed` or u, v, w AT EVERY GRID POINT from values known
 * on or next to the surface only, and a speed that is constant along the normals keeps phi a distance while it moves.  q, phi and
 * mask have the layout of every other entry point.  rounds_done, changed_trace and info may be NULL.
 *   FROZEN   the rule of lsf_distance_fill.  mask == NULL: the points, wall points included, with |phi| < far; far = band * dx,
 *            computed once on the host.  With a mask: the points with mask == 1, and band is ignored.  Frozen points hold the
 *            caller's q and are never written.  phi and mask are inputs only: read, never written.
 *   start    every other point is UNKNOWN: whatever q holds there on entry is ignored (a NaN there is legal).  Unknown is
 *            represented in the field by NaN.
 *   round    8 in-place raster sweeps over all points 0..n of each axis, in the direction order of lsf_distance_fill:
 *            (+,+,+) (+,+,-) (+,-,-) (-,-,-) (-,+,-) (-,-,+) (-,+,+) (+,-,+).
 *   visit    of a non-frozen point p, with f = |phi| (a neighbour outside the grid has f = +inf) and q as it is at that moment of
 *            the sweep.  For each axis A: n_A is the one of the two neighbours with the smaller f, the one at the lower index on
 *            a tie;  w_A = f(p) - f(n_A);  the axis is USED when w_A > 0 and q(n_A) is not NaN;
 *              t_A = w_A * q(n_A) and s_A = w_A when used, both 0.0 otherwise;
 *              den = (s_x + s_y) + s_z;  den == 0: nothing happens.  Otherwise new = ((t_x + t_y) + t_z) / den;
 *              if !(new == old) -- true for an unknown old -- new is stored and the visit is counted.
 *            Evaluated exactly as written, left to right, without contraction; / is the IEEE division.
 *   trace    changed_trace[r], r < trace_cap: the number of counted visits of round r (an integer: no arrival order in it).
 *   stop     after the first round whose count is 0 (that round is counted) or after max_rounds; rounds_done = rounds run.
 *            Reaching max_rounds is LSF_OK.  A point depends only on neighbours of strictly smaller |phi|, so the dependency
 *            graph has no cycle and the fixed point is reached EXACTLY: the rounds stop by themselves, with a count of 0.
 *   info     [0] frozen points  [1] non-frozen points that hold a value on return  [2] UNREACHED points, still NaN on return.
 *            Written on LSF_OK only.  Unreached points are left NaN, loudly, and reported -- never filled with a guess: a point
 *            none of whose neighbours has a smaller |phi| than its own has nothing to take a value from, so a PLATEAU of |phi|
 *            can never be reached.  Such a plateau is the +-far of a clamped lsf_mesh_distance field or the 1.0 of lsf_phi0: run
 *            lsf_distance_fill or lsf_reinit first.
 *   result   field, rounds_done, trace and info are those of the serial loops above, bit for bit, on both seams, on any stream,
 *            from run to run -- after every round, not only at the fixed point (tests/extend_ref.py is that serial statement).
 *   range    the bit promise is stated for finite q on the frozen points and finite phi whose products w * q do not overflow
 *            (every new value is then a weighted mean of finite values); nothing is promised beyond it.
 *   errors   LSF_ERR_INVALID, all detected before q is written, the offending count in lsf_last_error() where there is one: a NULL
 *            q or phi; nx, ny or nz < 1 or more than 2^31 - 1 points; dx not finite or <= 0; mask == NULL with band not finite or
 *            <= 0; max_rounds < 1; no frozen point; a non-finite q on a frozen point (count); a non-finite phi anywhere (count).
 *            Unlike lsf_distance_fill the frozen set need NOT separate the signs: |phi| orders the points on both sides.  No
 *            device: LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   seams    lsf_extend_field takes phi, an input only, through its twin under lsf_mirror exactly as lsf_extract_surface takes its
 *            phi, and the mask as lsf_distance_fill takes its mask.  q has NO twin and lsf_mirror does not apply to it: it is staged
 *            in a workspace slot of its own, copied in on every call and copied back on LSF_OK only, LSF_MIRROR_LAZY or not.
 *            lsf_extend_field_device returns after the stream is synchronised (the host reads one count per round).
 * Guidance: the scheme is FIRST ORDER; every value is a convex combination of frozen values, so the result stays inside their
 * [min, max].  A caller with u, v, w calls three times.  Convergence took 2 - 4 rounds on the test inputs (6 on two spheres at 512^3).
 * Workspace beyond the caller's arrays: the bit per point of lsf_distance_fill plus 48 bytes of counters; the host seam adds one
 * field for q.  Work: a round is 8 * (tiles_x + tiles_y + tiles_z - 2) dependent launches of 32 x 8 x 8-point tiles, as in
 * lsf_distance_fill, each tile loading two fields.  Out of scope: several quantities in one call, higher order, fp32, multi-GPU,
 * q taken from mesh-node data.
 * Timed once beside lsf_distance_fill on the same field (profiles/extend_field_time.txt, from profiles/micro/extend_field_time.py):
 * 19.2 ms per round at 256^3 against 14.4, 110 ms at 512^3 against 36.  No speed is claimed beyond that record. */
#define LSF_EXTEND_INFO_LEN 3
int lsf_extend_field(double *q, const double *phi, const int32_t *mask, int nx, int ny, int nz, double dx, double band,
                     int max_rounds, int *rounds_done, int64_t *changed_trace, int trace_cap, int64_t info[LSF_EXTEND_INFO_LEN]);
int lsf_extend_field_device(double *d_q, const double *d_phi, const int32_t *d_mask, int nx, int ny, int nz, double dx,
                            double band, int max_rounds, int *rounds_done, int64_t *changed_trace, int trace_cap,
                            int64_t info[LSF_EXTEND_INFO_LEN], void *stream);

/* ---- level-set transport: WENO5 / TVD-RK3 advection by a velocity field and along the normal ----------
 * No reference counterpart ("Currently has no capability to do moving geometry", the reference's README).  Advances
 *     phi_t + u . grad(phi) + F |grad(phi)| = 0
 * by `steps` explicit steps of size dt on the whole grid; lsf_reinit / lsf_reinit_band repair the distance property afterwards.
 * The field layout is that of every other entry point.  steps_done, cfl and change_trace may be NULL.
 *   fields   u, v, w (the velocity) and speed (F, the speed along the outward normal grad(phi)/|grad(phi)|: F > 0 grows the
 *            region phi < 0) have phi's layout: values AT the grid points.  u, v, w are given together or all NULL; speed may be
 *            NULL; at least one of the two groups is given.  All four are inputs: read, never written, and frozen for the whole
 *            call -- a caller with a time-dependent velocity calls once per step on the device seam.
 *   mode     LSF_ORDER_JACOBI | LSF_ARITH_STRICT or | LSF_ARITH_FAST.  LSF_ORDER_GS is LSF_ERR_INVALID (every stage reads the
 *            field as it was when the stage began), as in lsf_reinit_band.
 *   D-, D+   every interior cell (1..n-1 on each axis) takes its one-sided derivatives dmA, dpA on each axis A from the
 *            reference's weno (subs.f90:489-711) WITHOUT the p5 = 0 of its y axis (subs.f90:576 belongs to the reference's
 *            reinit, not to this operator): WENO5 on all three axes when 4 <= i <= nx-5 and likewise j and k (the reference's
 *            joint rule), first-order differences (c - m)/dx, (p - c)/dx on all three axes otherwise.
 *   STRICT   evaluated as written, left to right, without contraction; / and sqrt are the IEEE ones:
 *              pos(a) = a > 0 ? a : 0;  neg(a) = a < 0 ? a : 0
 *              T  = ((pos(u)*dmx + neg(u)*dpx) + (pos(v)*dmy + neg(v)*dpy)) + (pos(w)*dmz + neg(w)*dpz)    (absent without u, v, w)
 *              gA = m*m, m = max(max(dmA*sg, dpA*-sg), 0), sg = speed > 0 ? 1 : -1     (the Godunov term of subs.f90:684-692,
 *                   switched on the sign of the speed instead of the sign of phi)
 *              N  = speed * sqrt((gX + gY) + gZ)                                                           (absent without speed)
 *              R  = T, N or T + N;    t = phi - dt*R
 *   FAST     the same operator in the restructured arithmetic of LSF_ARITH_FAST (differences scaled by dx, one reciprocal per
 *            WENO side, FMA): ~1e-16 per stage from STRICT.
 *   stages   S(a) = t computed from the field a at every interior cell:
 *              LSF_ADVECT_EULER  phi <- S(phi)
 *              LSF_ADVECT_RK3    a = S(phi);  b = 0.75*phi + 0.25*S(a);  phi <- (1./3.)*phi + (2./3.)*S(b)     (Shu-Osher)
 *            After every stage the wall points of the stage's output take the extrapolation boundary condition of
 *            subs.f90:859-897 (as after a sweep of lsf_reinit).
 *   trace    change_trace[s], s < trace_cap: the largest |new - old| over the interior cells of step s (0-based), NaN if any of them
 *            is NaN -- no order of summation in it: bit-identical between the seams, on any stream, from run to run.  A NaN ends the
 *            call with LSF_ERR_NAN after that step; steps_done counts it and phi holds the state after it.
 *   cfl      (dt * max over ALL points of (|u| + |v| + |w| + |speed|)) / dx, absent fields left out, computed once per call.  It is
 *            REPORTED, never judged: the caller keeps it below 1 (RK3 with WENO5 is stable there; tests run at 0.5).  Written on
 *            LSF_OK and on LSF_ERR_NAN.
 *   steps=0  LSF_OK, steps_done = 0, phi untouched, cfl still reported.
 *   result   with LSF_ARITH_STRICT field, trace and cfl are those of the statement above bit for bit (tests/advect_ref.py is that
 *            statement in numpy), on both seams.  One call of n steps equals n calls of one step: no state between calls.
 *   errors   LSF_ERR_INVALID, all detected before phi is written, with the count in lsf_last_error() where there is one: a NULL
 *            phi; u, v, w not given together; neither velocity nor speed; nx, ny or nz < 2, a k-plane above 2 GB or more than
 *            2^31 - 1 points (the dimensions lsf_reinit_band refuses); dx or dt not finite or <= 0; steps < 0; an unknown scheme;
 *            LSF_ORDER_GS or an unknown ordering; a non-finite value in u, v, w or speed (counted by the same pass that finds the
 *            maximum for cfl).  No device: LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   seams    lsf_advect_field treats phi as in/out under lsf_mirror exactly as lsf_reinit_band does, and u, v, w, speed as that
 *            call treats its mask: inputs only, never copied back; taken from the host, or under LSF_MIRROR_TRUST / LAZY from their
 *            device twin where they have a current one.
 *            lsf_advect_field_device returns after the stream is synchronised (the host reads the step counter).
 * Workspace beyond the caller's fields: two fields for LSF_ADVECT_RK3 (stage 3 writes the caller's field in place: it reads the old
 * phi at its own point only), one for LSF_ADVECT_EULER; the host seam adds one field per input given.  The result always ends in
 * the caller's field.  Work: one launch per stage over the interior + the boundary condition, one small launch per step for the
 * trace.  The same operator on the cells of a mask: lsf_advect_field_band below.  Out of scope: fp32,
 * multi-GPU, a CFL-chosen dt.
 * Not timed on hardware yet: no speed is claimed (the measurement is profiles/micro/advect_field_time.py). */
#define LSF_ADVECT_RK3 0 /* scheme */
#define LSF_ADVECT_EULER 1
int lsf_advect_field(double *phi, const double *u, const double *v, const double *w, const double *speed, int nx, int ny,
                     int nz, double dx, double dt, int steps, int scheme, int mode, int *steps_done, double *cfl,
                     double *change_trace, int trace_cap);
int lsf_advect_field_device(double *d_phi, const double *d_u, const double *d_v, const double *d_w, const double *d_speed,
                            int nx, int ny, int nz, double dx, double dt, int steps, int scheme, int mode, int *steps_done,
                            double *cfl, double *change_trace, int trace_cap, void *stream);

/* ---- level-set transport on the cells of a caller's mask only: lsf_advect_field on a list ----------
 * No reference counterpart.  In a time loop "advect, repair the distance on the tube (lsf_reinit_band), rebuild the tube
 * (lsf_narrowband)" lsf_advect_field pays (n+1)^3 per stage; this call applies the same operator to the cells of a mask and
 * reports when the mask was too narrow.  steps_done, cfl, change_trace, info and margin may be NULL.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1 on entry, fixed for the whole
 *            call.  Any other mask value means "not in the list"; a 1 on a wall point is ignored.  The mask is read once and
 *            never written.
 *   operator D-, D+, T, N, R and t = phi - dt*R are exactly those of lsf_advect_field: STRICT and FAST, the joint WENO rule (cells
 *            4..n-5 on all three axes, first-order differences on all three otherwise), no y quirk.  All stencil values are taken
 *            from the stage's input field, whether the stencil point is in the list or not.
 *   stages   S(a) = t computed from the field a:
 *              LSF_ADVECT_EULER  list cells of phi <- S(phi)
 *              LSF_ADVECT_RK3    a = phi with its list cells replaced by S(phi);
 *                                b = phi with its list cells replaced by 0.75*phi + 0.25*S(a);
 *                                list cells of phi <- (1./3.)*phi + (2./3.)*S(b)
 *            Points outside LIST are NEVER written, wall points included: the extrapolation boundary condition is NOT applied, as
 *            in lsf_reinit_band.
 *   inputs   u, v, w, speed have phi's layout and are given as in lsf_advect_field (u, v, w together or all NULL, speed optional,
 *            at least one group).  They are read AT LIST CELLS ONLY: whatever they hold elsewhere is ignored and a NaN there is
 *            legal -- what lsf_extend_field leaves on unreached points.  Never written.
 *   cfl      (dt * max over LIST cells of (|u| + |v| + |w| + |speed|)) / dx, added left to right, absent fields left out.
 *            Reported, never judged.
 *   trace    change_trace[s], s < trace_cap: the largest |new - old| over the list cells of step s, NaN if any of them is NaN; the
 *            bit-pattern maximum of lsf_advect_field.  A NaN ends the call with LSF_ERR_NAN after that step; steps_done counts
 *            it and phi holds the state after it.
 *   EDGE     a list cell is an edge cell when at least one of its six axis neighbours is not in LIST (a wall point never is).
 *   info     [0] list cells; [1] edge cells; [2] edge cells whose (phi < 0) on return differs from (phi < 0) on entry: the surface
 *            reached the edge of the list and the result next to it is not to be trusted.
 *   margin   the smallest |phi| over the edge cells on return (the minimum of bit patterns: no order in it).  The caller compares
 *            it with a few dx before the next call and rebuilds the mask (lsf_narrowband) when it shrinks.
 *            info and margin are written on LSF_OK only; on LSF_OK no list cell is NaN, so both are well defined.
 *   steps=0  LSF_OK, phi untouched; cfl, info and margin are still reported: info[2] = 0, margin that of the field as it came.
 *   empty    LIST empty: LSF_OK, steps_done = 0, nothing written, cfl = 0, info = {0,0,0}, margin = +inf.
 *   mode     LSF_ORDER_JACOBI | LSF_ARITH_STRICT or | LSF_ARITH_FAST.  LSF_ORDER_GS is LSF_ERR_INVALID.
 *   result   with LSF_ARITH_STRICT field, trace, cfl, info and margin are those of the serial statement tests/advect_band_ref.py
 *            bit for bit, on both seams, on any stream, from run to run.  One call of n steps equals n calls of one step for phi,
 *            trace and cfl; info[2] is relative to each call's own entry.
 *   errors   those of lsf_advect_field; a NULL mask; a non-finite u, v, w or speed AT A LIST CELL, with the count in
 *            lsf_last_error().  All detected before phi is written.  No device: LSF_ERR_NO_DEVICE.
 *   seams    phi and the mask are treated as lsf_reinit_band treats them under lsf_mirror; u, v, w, speed as lsf_advect_field
 *            treats them.  lsf_advect_field_band_device returns after the stream is synchronised.
 * Guidance: one stage carries information three cells along an axis.  A list cell farther than 9 cells per RK3 step (3 per Euler
 * step) from every non-list point -- city-block distance, walls count as non-list -- holds exactly the value lsf_advect_field
 * would give it; cells nearer than that read frozen neighbours.  Make the mask WIDER than the band whose values are trusted and
 * keep steps * cfl well below the width.  Serial statement, a sphere translated at CFL 0.49 on 49^3 points (the translate case of
 * tests/advect_ref.py), largest difference from the full-grid run over the cells with |exact| < 2 dx: with the mask
 * |phi| < 8.1 dx 0 after 1 step, 1.5e-7 (2.3e-6 dx) after 4 and 5.6e-6 (8.9e-5 dx) after 8 (margin 6.9, 6.0 and 4.7 dx); with
 * |phi| < 4.1 dx 1.6e-5 (2.6e-4 dx) after 1 step, 2.1e-4 (3.4e-3 dx) after 4 and 0.16 (2.6 dx) after 8, when the surface has left
 * the list (margin 2.9, 1.9 and 0.65 dx; no edge cell has changed sign yet: watch the margin, not only info[2]).
 * Work: beyond the list build and one copy of the field per workspace field (two for RK3, one for Euler), nothing is proportional
 * to the grid; a stage visits the list cells only.  Measured on one MI355X (profiles/advect_band_time.txt, made by
 * profiles/micro/advect_band_time.py: a sphere, the mask |phi| < 8.1 dx, RK3, STRICT, ms per step against lsf_advect_field on the
 * same field): 0.08 against 1.47 at 256^3 (2.2 % of the grid in the list) and 0.24 against 12.1 at 512^3 (1.1 %) inside a call of
 * 20 steps; a call of ONE step, which pays the list build and the copies each time, 0.49 against 1.59 and 1.59 against 13.0.
 * No automatic rebuilding of the list, no dispatch to lsf_advect_field. */
#define LSF_ADVECT_BAND_INFO_LEN 3
int lsf_advect_field_band(double *phi, const int32_t *mask, const double *u, const double *v, const double *w,
                          const double *speed, int nx, int ny, int nz, double dx, double dt, int steps, int scheme, int mode,
                          int *steps_done, double *cfl, double *change_trace, int trace_cap,
                          int64_t info[LSF_ADVECT_BAND_INFO_LEN], double *margin);
int lsf_advect_field_band_device(double *d_phi, const int32_t *d_mask, const double *d_u, const double *d_v, const double *d_w,
                                 const double *d_speed, int nx, int ny, int nz, double dx, double dt, int steps, int scheme,
                                 int mode, int *steps_done, double *cfl, double *change_trace, int trace_cap,
                                 int64_t info[LSF_ADVECT_BAND_INFO_LEN], double *margin, void *stream);

/* ---- the band time loop: transport, repair of the distance and the cell list moving with the surface ----------
 * No reference counterpart.  lsf_advect_field_band and lsf_reinit_band each build the list from the mask and copy the field on every
 * call, and a list made from |phi| < w dx cannot follow the surface: points outside it are never written, so ahead of the surface
 * they keep the distance of time 0.  This call keeps ONE list on the device for all its steps, runs the stages of the one and the
 * sweeps of the other on it, watches the edge of the list and rebuilds the list when the surface comes near it (the local level
 * set method of Peng, Merriman, Osher, Zhao and Kang, J. Comput. Phys. 155, 1999: dilate the trusted core, give entering cells a
 * placeholder that the reinitialisation corrects).  steps_done, cfl, change_trace, info and margin may be NULL.
 *   LIST     on entry the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  From the first
 *            rebuild on, LIST is the last rebuilt list.
 *   step s   in this order:
 *            1. one step of lsf_advect_field_band's stages on LIST: operator, schemes, STRICT and FAST unchanged; no boundary
 *               condition, nothing outside LIST is written.  change_trace[s] as there.  A NaN ends the call with LSF_ERR_NAN after
 *               this transport: the sweeps of the step are not run, steps_done counts the step, info and margin are not written.
 *            2. reinit_sweeps (>= 0) sweeps of lsf_reinit_band's sweep on LIST with pseudo-time step h; phiS is the field after 1
 *               at the list cells.  No RMS, no early stop.
 *            3. the CHECK, if (s+1) % check_every == 0 or s == steps-1.
 *   CHECK    An OPEN EDGE cell is a list cell with at least one of its six axis neighbours an INTERIOR point outside LIST.  A wall
 *            neighbour does not open an edge: the list cannot grow there (without this rule a surface near a wall rebuilds in every
 *            step).  flips = the number of open-edge cells whose (phi < 0) differs from that at the last build of the list (entry,
 *            or the last rebuild); margin = the smallest |phi| over the open-edge cells, the minimum of bit patterns, +inf when
 *            there are none.  flips > 0: the call ends with LSF_OK, steps_done = s+1 (< steps possible), info[2] = flips, no
 *            rebuild -- the loud ending: the surface reached the edge between two checks.  Else, margin < core*dx: REBUILD.
 *   REBUILD  CORE = the list cells with |phi| < core*dx.  NEW = the interior points within Chebyshev distance `ring` of a CORE
 *            cell.  Entering cells (NEW \ LIST) take phi < 0 ? -far : +far with far = (core + (double)ring) * dx, computed once on
 *            the host (-0.0 and every positive value give +far); leaving cells keep the value they hold.  LIST becomes NEW and the
 *            sign reference becomes the field as it is now.  A rebuild after the last step is done like any other, so with no flips
 *            one call of n steps equals two calls of n/2 for phi, mask and trace whenever check_every divides n/2.
 *   inputs   u, v, w, speed are given as in lsf_advect_field.  The list moves, so they must be finite at ALL points: checked once
 *            per call, before anything is written, by the pass lsf_advect_field uses, and cfl is that call's, over all points.
 *            They are frozen for the call: a caller with a time-dependent speed calls once per few steps.
 *   outputs  on LSF_OK and LSF_ERR_NAN phi is the state after the last step run and mask is 1 on the cells of the current LIST and 0
 *            on every other point (the mask is in/out).  On LSF_ERR_INVALID both are untouched.
 *   info     on LSF_OK only: [0] list cells, [1] open-edge cells, [2] flips of the last check, [3] rebuilds, [4] entering cells
 *            summed over the rebuilds, [5] list cells adjacent to a wall with |phi| < core*dx ([0], [1] and [5] of the list on
 *            return).  [5] > 0: the surface is near a wall, where this call applies no boundary condition and the result next to it
 *            is the caller's risk.  margin (LSF_OK only) is taken over the open-edge cells of the list on return.
 *   errors   LSF_ERR_INVALID, all detected before anything is written: those of lsf_advect_field_band; core not finite or <= 0; ring
 *            outside 1..8; reinit_sweeps < 0; h not finite or <= 0 when reinit_sweeps > 0; check_every < 1; non-finite inputs, with
 *            their count in lsf_last_error().  No device: LSF_ERR_NO_DEVICE.
 *   empty    LIST empty on entry: LSF_OK, steps_done = 0, phi untouched, the mask all 0, cfl = 0, info zero, margin = +inf.
 *   steps=0  LSF_OK, phi untouched, the mask normalised to 0/1, cfl reported, one check without rebuild for info and margin.
 *   mode     LSF_ORDER_JACOBI | LSF_ARITH_STRICT or | LSF_ARITH_FAST.
 *   result   with LSF_ARITH_STRICT phi, mask, trace, cfl, info and margin are those of the serial statement
 *            tests/evolve_band_ref.py bit for bit, on both seams, on any stream, from run to run: all reductions are bit-pattern
 *            minima / maxima or integer counts, so the order of the list reaches no result.
 *   seams    phi and mask are in/out under lsf_mirror, as phi is for lsf_reinit_band (the mask through the twin of phiNB when it
 *            IS that array, of phiSB otherwise); u, v, w, speed as lsf_advect_field treats them.  lsf_evolve_band_device returns
 *            after the stream is synchronised.
 * Guidance: the field must be a distance for |phi| < far; a clamped one (what lsf_mesh_distance(width) gives) is fine.  Keep
 * check_every * cfl well below core: the surface may move that many cells between two looks at the edge.  Use ring >= 3, so a core
 * cell's WENO stencil stays in the list.  The placeholders are corrected by the sweeps and by nothing else.  Serial statement, the
 * distance to a sphere of radius 0.5 clamped to +-6 dx on 49^3 points, mask |phi| < 6 dx, u = (1,0,0) at CFL 0.5, 36 steps (the
 * surface moves 18 cells, three times the list's half-width), core = 3, ring = 3, h = 0.5 dx: with 2 sweeps per step 6 rebuilds,
 * no flips, every cell with |exact| < 2 dx in the final list and the largest error there 0.029 dx (lsf_advect_field alone, every
 * cell and no reinitialisation: 0.014 dx); with reinit_sweeps = 0 the same run ends 3.3 dx off.
 * Work: between rebuilds nothing is proportional to the grid: the stage buffers are copied from phi once per call, a step enqueues
 * its stages and sweeps on the resident list, and the host reads one 64-byte record per check.  A rebuild clears and collects a
 * 4-byte scratch mask (the list build of lsf_reinit_band) and makes no pass over a field.  Workspace: the stage buffers of
 * lsf_advect_field_band and one 4-byte mask.  Measured on one MI355X (profiles/evolve_band_time.txt, made by
 * profiles/micro/evolve_band_time.py: the sphere and mask of lsf_advect_field_band's measurement, RK3, STRICT, 2 sweeps, 20 steps,
 * ms per step against the same steps done with one lsf_advect_field_band step and one lsf_reinit_band(iter = 1) per step): 0.15
 * against 0.78 at 256^3 and 0.40 against 2.51 at 512^3, no rebuild in those runs; with core = 6, where one rebuild falls inside
 * the 20 steps and the list grows by a third, 0.16 and 0.46.  Out of scope: a boundary condition at the walls or a surface that
 * leaves through one, inputs that are NaN off the list, a CFL-chosen dt, a time-dependent velocity inside one call, fp32,
 * multi-GPU, a rebuild without the pass over the mask. */
#define LSF_EVOLVE_INFO_LEN 6
int lsf_evolve_band(double *phi, int32_t *mask, const double *u, const double *v, const double *w, const double *speed, int nx,
                    int ny, int nz, double dx, double dt, int steps, int scheme, int mode, double core, int ring,
                    int reinit_sweeps, double h, int check_every, int *steps_done, double *cfl, double *change_trace,
                    int trace_cap, int64_t info[LSF_EVOLVE_INFO_LEN], double *margin);
int lsf_evolve_band_device(double *d_phi, int32_t *d_mask, const double *d_u, const double *d_v, const double *d_w,
                           const double *d_speed, int nx, int ny, int nz, double dx, double dt, int steps, int scheme, int mode,
                           double core, int ring, int reinit_sweeps, double h, int check_every, int *steps_done, double *cfl,
                           double *change_trace, int trace_cap, int64_t info[LSF_EVOLVE_INFO_LEN], double *margin, void *stream);

/* ---- mean and Gaussian curvature of the level sets on the cells of a caller's mask ----------
 * The reference computed its "true curvature" once and commented it out (subs.f90:426-448; setSurfCurv interpolates a `curv`
 * that nothing fills any more); the ingredients are its second-order secondDeriv (subs.f90:382-398).  This call gives the shape
 * of the surface where a speed law F = a - b*kappa needs it: kappa = div(grad(phi)/|grad(phi)|) = k1 + k2, the Gaussian curvature
 * k1 * k2 and |grad(phi)|, at the list cells only.  gauss, gmag, info and kappa_max may be NULL; kappa is required.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  Any other mask value means
 *            "not in the list"; a 1 on a wall point is ignored.  The mask is read once and never written.  Every stencil point
 *            of an interior cell -- +-1 on each axis and the 12 edge diagonals -- lies inside the field: one rule for every list
 *            cell, no WENO rule, no first-order cells.
 *   outputs  phi and mask are inputs only.  Each output that is given is written AT LIST CELLS and nowhere else: what it holds at
 *            every other point stays bit for bit, NaNs included -- a kappa written on the cells of a mask plugs straight into the
 *            `speed` of lsf_advect_field_band on the same mask (which reads it at list cells only) and, on a thin frozen band, into
 *            the q of lsf_extend_field.
 *   values   evaluated exactly as written, left to right, without contraction; / and sqrt are the IEEE ones; c is the value at
 *            the cell and s(a,b,c) the neighbour at that offset; 2.*dx, dx*dx and 4.*(dx*dx) are computed once:
 *              px  = (s(1,0,0) - s(-1,0,0)) / (2.*dx)                                          likewise py, pz
 *              pxx = ((s(1,0,0) - 2.*c) + s(-1,0,0)) / (dx*dx)                                 likewise pyy, pzz
 *              pxy = (((s(1,1,0) - s(1,-1,0)) - s(-1,1,0)) + s(-1,-1,0)) / (4.*(dx*dx))        likewise pxz (x,z), pyz (y,z)
 *              g2  = (px*px + py*py) + pz*pz;  g = sqrt(g2)                                    -> gmag
 *              num = ((px*px)*(pyy+pzz) + (py*py)*(pxx+pzz)) + (pz*pz)*(pxx+pyy)
 *              mix = ((px*py)*pxy + (px*pz)*pxz) + (py*pz)*pyz
 *              H   = (num - 2.*mix) / (g2*g)                                                   -> kappa
 *              A   = ((px*px)*(pyy*pzz - pyz*pyz) + (py*py)*(pxx*pzz - pxz*pxz)) + (pz*pz)*(pxx*pyy - pxy*pxy)
 *              B   = ((px*py)*(pxz*pyz - pxy*pzz) + (py*pz)*(pxy*pxz - pyz*pxx)) + (px*pz)*(pxy*pyz - pxz*pyy)
 *              K   = (A + 2.*B) / (g2*g2)                                                      -> gauss
 *            Signs: a sphere of radius r with phi < 0 inside has kappa = +2/r and gauss = 1/r^2.
 *   DEGENERATE  a cell with g2 < 1e-24 (a flat spot, e.g. the inside of a plateau): H = K = 0.0, gmag gets its g.  A NaN g2 is
 *            not degenerate and gives NaN.
 *   CLAMP    clamp == 0: none.  Otherwise lim = clamp / dx, computed once on the host, and
 *              if (H > lim) H = lim;  if (H < -lim) H = -lim;      K likewise with lim*lim
 *            -- comparisons, so a NaN stays NaN.  A cell is CLAMPED when a written value differs from the unclamped one (K counts
 *            only where gauss is given).  gmag is never clamped.  A grid cannot resolve |kappa| > 1/dx, so clamp = 1 is the
 *            usual choice: on the distance to a sphere with every interior point listed the largest unclamped |kappa|*dx is
 *            10.8, at the cells next to the centre.
 *   info     [0] list cells; [1] degenerate cells; [2] clamped cells; [3] 0, reserved.
 *   kappa_max  the largest |kappa| AS STORED over the list cells: the maximum of bit patterns, so no order of reduction shows
 *            in it.  info and kappa_max are written on LSF_OK only.
 *   NaN      a non-finite stored value at a list cell -- kappa, or gauss or gmag where given -- gives LSF_ERR_NAN with the number
 *            of such cells in lsf_last_error().  The outputs then hold what was computed; info and kappa_max are not written.
 *   empty    LIST empty: LSF_OK, nothing written, info all 0, kappa_max = 0.0.
 *   errors   LSF_ERR_INVALID, all detected before anything is written: a NULL phi, mask or kappa; an output that overlaps phi
 *            or another output; the dimensions lsf_reinit_band refuses (nx, ny or nz < 2, a k-plane above 2 GB, more than
 *            2^31 - 1 points); dx not finite or <= 0; clamp not finite or < 0.  No device: LSF_ERR_NO_DEVICE -- there is no CPU
 *            fallback.
 *   result   the outputs, info and kappa_max are those of the serial statement tests/curvature_ref.py bit for bit, on both
 *            seams, on any stream, from run to run.  There is one arithmetic and no mode word.
 *   seams    lsf_curvature_band takes phi, an input only, through its twin under lsf_mirror exactly as lsf_extract_surface takes
 *            its phi, and the mask as lsf_reinit_band takes its mask.  The outputs have NO twin: each one given is staged as
 *            lsf_extend_field stages q, copied in on every call and copied back on LSF_OK and on LSF_ERR_NAN.
 *            lsf_curvature_band_device returns after the stream is synchronised (the host finishes the per-block counts).
 * Guidance: the scheme is SECOND ORDER on a smooth phi (serial statement, distance to a sphere of radius R = 0.6, cells with
 * |phi| < 2.1 dx against the level set through the cell, 2/r and 1/r^2: largest error of kappa 5.0e-2 of the surface's 2/R on 25^3
 * points and 5.3e-3 on 49^3, of gauss 1.7e-1 of 1/R^2 and 1.3e-2).  phi need not be a distance, but the kinks of one (the medial axis, the clamp of
 * lsf_mesh_distance(width)) give large values: that is what the clamp and info[2] are for.  kappa handed to lsf_advect_field_band
 * as speed = a - b*kappa is UPWINDED by that call's Godunov term, which is fine for a small b; the centrally differenced parabolic
 * term b*kappa*|grad(phi)| inside the transport stages is lsf_evolve_band_curv below, built from this call's H and g.
 * Work: the list build of lsf_reinit_band and ONE launch over the list, one lane per cell, 19 gathered loads and up to three
 * stores; the host reads 32 bytes per 256 list cells.  Workspace: that of the list; the host seam adds one field per output given.
 * Also out of scope: principal directions, fp32, multi-GPU, a dense call without a mask.
 * Timed once on one MI355X beside ONE Euler step of lsf_advect_field_band on the same sphere and mask |phi| < 8.1 dx
 * (profiles/curvature_band_time.txt, from profiles/micro/curvature_band_time.py; device seam, ms per call, list build included):
 * 0.25 against 0.39 at 256^3 (2.2 % of the grid in the list) and 0.51 against 1.00 at 512^3 (1.1 %), with one output or all three.
 * No speed is claimed beyond that record. */
#define LSF_CURV_INFO_LEN 4
int lsf_curvature_band(const double *phi, const int32_t *mask, double *kappa, double *gauss, double *gmag, int nx, int ny, int nz,
                       double dx, double clamp, int64_t info[LSF_CURV_INFO_LEN], double *kappa_max);
int lsf_curvature_band_device(const double *d_phi, const int32_t *d_mask, double *d_kappa, double *d_gauss, double *d_gmag, int nx,
                              int ny, int nz, double dx, double clamp, int64_t info[LSF_CURV_INFO_LEN], double *kappa_max,
                              void *stream);

/* ---- the band time loop with a curvature term: F = a - b*kappa run inside lsf_evolve_band's loop ----------
 * No reference counterpart.  lsf_evolve_band freezes `speed` for a call, and a kappa handed in through `speed` is upwinded; motion
 * by mean curvature needs kappa*|grad(phi)| differenced centrally from every stage's own input field.  This call is lsf_evolve_band
 * with that term in the stage.  EVERYTHING NOT NAMED HERE IS lsf_evolve_band'S CONTRACT, word for word: the list, the step order, the
 * check, the open-edge rule, the rebuild, the outputs, info, margin, the empty list, steps = 0, the seams and LSF_ERR_NAN.
 *   equation phi_t + u . grad(phi) + F |grad(phi)| = bcurv * kappa * |grad(phi)|.  A sphere with phi < 0 inside has kappa = +2/r
 *            and shrinks: its radius is sqrt(R0^2 - 4*bcurv*t).
 *   stage    S(a) at a list cell, a being the stage's input field:
 *              t0 = a - dt*R0     R0 = T, N or T + N exactly as in lsf_advect_field_band (joint WENO rule, STRICT and FAST
 *                                 unchanged); with neither a velocity nor a speed t0 = a
 *              C  = bcurv * (H * g)   H and g of lsf_curvature_band's statement evaluated on a at the cell: the 19 values, px ... pyz,
 *                                 g2, g = sqrt(g2), num, mix, H = (num - 2.*mix)/(g2*g); DEGENERATE (g2 < 1e-24) gives H = 0.0; CLAMP
 *                                 with lim = clamp / dx, computed once on the host, is applied to H by the same comparisons
 *                                 (clamp == 0: none).  One rule for every interior cell, no first-order variant.
 *              t  = t0 + dt*C
 *            The RK3 / Euler blends are those of lsf_advect_field_band with this S.
 *   mode     STRICT evaluates as written, left to right, without contraction; / and sqrt are the IEEE ones.  FAST keeps R0 in the
 *            existing FAST arithmetic; C is computed uncontracted in FAST too (one arithmetic for the term) and enters as
 *            fma(dt, C, t0).
 *   inputs   u, v, w come together or all NULL and speed is optional, as before; BOTH groups may be absent when bcurv > 0 (pure
 *            curvature flow).  cfl is lsf_evolve_band's, and 0 when both groups are absent.
 *   diffusion  (may be NULL) (bcurv*dt)/(dx*dx), computed once on the host: reported, never judged; written wherever cfl is.
 *   bcurv==0 with a velocity or a speed: the stage kernel of lsf_evolve_band is launched, every output equals that call's bit for
 *            bit, clamp is ignored and diffusion = 0.
 *   errors   those of lsf_evolve_band, and LSF_ERR_INVALID before anything is written for: bcurv not finite or < 0; bcurv == 0 with
 *            neither a velocity nor a speed; clamp not finite or < 0.
 *   result   with LSF_ARITH_STRICT phi, mask, trace, cfl, diffusion, info and margin are those of the serial statement
 *            tests/evolve_band_curv_ref.py bit for bit, on both seams.
 *   seams    phi, mask and the inputs go through exactly the twins lsf_evolve_band uses (one staging function serves both calls).
 * Guidance: the term is explicit.  The explicit bound of the linear 3-D heat stencil is diffusion <= 1/6 for Euler; RK3 reaches
 * further.  The sweeps keep |grad(phi)| = 1 near the surface, where the term is bcurv*kappa; at the kinks of a distance (medial axis,
 * the +-far plateau) kappa is large and meaningless: clamp = 1 bounds it at 1/dx.  Serial statement, a sphere of radius 0.6 on 33^3
 * points over [-1.5,1.5]^3, the distance clamped to +-6 dx, mask |phi| < 6 dx, core = 3, ring = 3, 2 sweeps, h = 0.5 dx, bcurv = 1,
 * clamp = 1, RK3, no velocity and no speed, the radius read off the +x axis by linear interpolation against sqrt(R0^2 - 4*b*t):
 * t = 0.04 in 30 steps (diffusion 0.152): off by 0.012 dx, no rebuild; in 11 steps (0.414): 0.001 dx, and with Euler 0.061 dx;
 * t = 0.07 in 53 steps (0.150): one rebuild (after step 41), no flips, 0.048 dx (tests/test_evolve_band_curv_cpu.py asserts twice
 * that); with the term left out the same run stays 3.4 dx from the closed form.
 * Work: that of lsf_evolve_band; a stage gathers 31 values instead of 19 where a velocity or a speed is present (19 without).
 * Measured on one MI355X (profiles/evolve_band_curv_time.txt, made by profiles/micro/evolve_band_curv_time.py: the sphere, mask, velocity
 * and speed of lsf_evolve_band's measurement, RK3, STRICT, 2 sweeps, 20 steps, diffusion 0.15, ms per step): 0.17 at 256^3 and 0.44 at
 * 512^3, against 0.14 and 0.39 for lsf_evolve_band on the same inputs and 0.93 and 3.50 for the loop of public calls it replaces (per
 * step lsf_curvature_band, speed = a - b*kappa, lsf_evolve_band(steps = 1)); no rebuild in those runs.  No speed is claimed beyond
 * that record.
 * Out of scope: the term in lsf_advect_field / lsf_advect_field_band, a cutoff of the term towards the list's edge, implicit or
 * semi-implicit time stepping, a dt chosen from diffusion, anisotropic or Gaussian-curvature laws, fp32, multi-GPU (DESIGN.md
 * section 8). */
int lsf_evolve_band_curv(double *phi, int32_t *mask, const double *u, const double *v, const double *w, const double *speed, int nx,
                         int ny, int nz, double dx, double dt, int steps, int scheme, int mode, double core, int ring,
                         int reinit_sweeps, double h, int check_every, double bcurv, double clamp, int *steps_done, double *cfl,
                         double *diffusion, double *change_trace, int trace_cap, int64_t info[LSF_EVOLVE_INFO_LEN], double *margin);
int lsf_evolve_band_curv_device(double *d_phi, int32_t *d_mask, const double *d_u, const double *d_v, const double *d_w,
                                const double *d_speed, int nx, int ny, int nz, double dx, double dt, int steps, int scheme, int mode,
                                double core, int ring, int reinit_sweeps, double h, int check_every, double bcurv, double clamp,
                                int *steps_done, double *cfl, double *diffusion, double *change_trace, int trace_cap,
                                int64_t info[LSF_EVOLVE_INFO_LEN], double *margin, void *stream);

/* ---- extension on a cell list: a quantity carried off the frozen cells of a caller's mask, constant along the normals ----------
 * No reference counterpart.  lsf_extend_field on the list of lsf_reinit_band: what carries a speed known on or next to the surface
 * only -- F = a - b*kappa from lsf_curvature_band, a growth rate, a solver's velocity -- to every cell of the mask that
 * lsf_advect_field_band or lsf_evolve_band moves the surface on, at a cost proportional to the list and not to the grid.  The
 * operator is lsf_extend_field's visit; the raster sweeps are replaced by JACOBI passes over the list.  q, phi, mask and known have
 * the layout of every other entry point.  known, passes_done, changed_trace and info may be NULL; mask is required.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  Any other mask value means
 *            "not in the list"; a 1 on a wall point is ignored.
 *   FROZEN   with known != NULL: the list cells with known == 1; band is ignored, and so is known off the list.  With
 *            known == NULL: the list cells with |phi| < far; far = band * dx, computed once on the host.  Frozen cells hold the
 *            caller's q and are never written.  phi, mask and known are inputs only: read, never written.
 *   off list q is never read and never written at a point that is not in the list: what it holds there stays bit for bit, and a NaN
 *            there is legal -- what lsf_curvature_band leaves.  phi is read at list cells and at their six axis neighbours only.
 *   start    every non-frozen list cell is UNKNOWN: whatever q holds there on entry is ignored.  Unknown is represented in the
 *            field by NaN.
 *   pass     every non-frozen list cell is visited with q AS IT WAS AT THE START OF THE PASS: all reads of a pass come before its
 *            writes.  The visit of a cell p is that of lsf_extend_field, with f = |phi|.  For each axis A: n_A is the one of the
 *            two neighbours with the smaller f, the one at the lower index on a tie;  w_A = f(p) - f(n_A);  the axis is USED when
 *            w_A > 0, n_A is in the LIST and q(n_A) is not NaN.  The neighbour is chosen by f first: if it is not in the list
 *            the axis is unused, the other neighbour is not tried.
 *              t_A = w_A * q(n_A) and s_A = w_A when used, both 0.0 otherwise;
 *              den = (s_x + s_y) + s_z;  den == 0: nothing happens.  Otherwise new = ((t_x + t_y) + t_z) / den;
 *              if !(new == old) -- true for an unknown old -- new is stored and the visit is counted.
 *            Evaluated exactly as written, left to right, without contraction; / is the IEEE division.
 *   trace    changed_trace[p], p < trace_cap: the number of counted visits of pass p (an integer: no arrival order in it).
 *   stop     after the first pass whose count is 0 (that pass is counted) or after max_passes; passes_done = passes run.
 *            Reaching max_passes is LSF_OK.  A cell depends only on neighbours of strictly smaller |phi|, so the dependency graph
 *            has no cycle, the fixed point is unique, and Jacobi passes reach it EXACTLY in as many passes as the longest chain
 *            of dependent cells plus one: the passes stop by themselves, with a count of 0.
 *   info     [0] list cells  [1] frozen cells  [2] non-frozen list cells that hold a value on return  [3] UNREACHED list cells,
 *            still NaN on return: stored as NaN and reported, never filled with a guess (a cell all of whose chosen neighbours
 *            are outside the list, unknown themselves or not below it in |phi|).  Written on LSF_OK only, and so are
 *            passes_done and the trace.
 *   result   field, passes_done, trace and info are those of the serial statement tests/extend_band_ref.py bit for bit, on both
 *            seams, on any stream, from run to run -- after every pass, not only at the fixed point.  On a list that keeps clear
 *            of the walls and holds every point the full-grid call would draw on, the converged result at list cells equals the
 *            converged lsf_extend_field with the same frozen set.
 *   range    as in lsf_extend_field: the bit promise is stated for finite frozen q and finite phi whose products w * q do not
 *            overflow.
 *   errors   LSF_ERR_INVALID, all decided before q is written, the offending count in lsf_last_error() where there is one: a NULL
 *            q, phi or mask; the dimensions lsf_reinit_band refuses (nx, ny or nz < 2, a k-plane above 2 GB, more than 2^31 - 1
 *            points); dx not finite or <= 0; known == NULL with band not finite or <= 0; max_passes < 1; trace_cap < 0; q sharing
 *            a byte with phi; an empty list; no frozen cell; a non-finite q on a frozen cell (count); list cells that see a
 *            non-finite phi at themselves or at one of their six neighbours (count of such cells).  No device:
 *            LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   seams    lsf_extend_field_band takes phi through its twin under lsf_mirror as lsf_extend_field does, and the mask as
 *            lsf_reinit_band takes its mask.  known is staged in a workspace slot of its own on every call.  q has NO twin: it is
 *            staged as lsf_extend_field stages it, copied in on every call and copied back on LSF_OK only.
 *            lsf_extend_field_band_device returns after the stream is synchronised (the host reads the counts of 8 passes at a time).
 * Guidance: FIRST ORDER, every value a convex combination of frozen values, as in lsf_extend_field.  The recipe on ONE mask:
 * lsf_curvature_band (kappa at list cells, NaN elsewhere) -> speed = a - b*kappa -> lsf_extend_field_band with known = the cells
 * next to the surface -> lsf_advect_field_band or lsf_evolve_band with that speed.  The number of passes is the longest chain of
 * dependent cells plus one: about twice the width of the list in cells beyond the frozen band (12 for a 4.1-cell mask around a
 * 1.5-cell band, 20 for 8.1, serial statement).  Work: the list build of lsf_reinit_band, one plan launch (7 gathered loads of phi
 * per cell) and two launches per pass over the list (4 gathered loads of q, one division); the host reads 64 bytes per 8 passes.
 * Workspace beyond the list's: 46 bytes per list cell; the host seam adds one field for q and one for known.  Out of scope: several
 * quantities in one call, higher order, fp32, multi-GPU, keeping the list on the device across calls or inside lsf_evolve_band,
 * single-buffer passes.
 * Timed once on one MI355X beside lsf_extend_field on the same two-sphere field, frozen band 3.5 cells, mask |phi| < 8.1 dx
 * (profiles/extend_band_time.txt, from profiles/micro/extend_band_time.py; device seam, ms per call to convergence, list build
 * included): 1.10 against 115.8 at 256^3 (514 594 list cells, 3.1 % of the grid, 26 passes of 0.030 ms, 0.33 ms of list build, plan
 * and counts) and 3.05 against 660.8 at 512^3 (2 048 561 cells, 1.5 %, 28 passes of 0.086 ms, 0.64 ms fixed).  No speed is claimed
 * beyond that record. */
#define LSF_EXTEND_BAND_INFO_LEN 4
int lsf_extend_field_band(double *q, const double *phi, const int32_t *mask, const int32_t *known, int nx, int ny, int nz, double dx,
                          double band, int max_passes, int *passes_done, int64_t *changed_trace, int trace_cap,
                          int64_t info[LSF_EXTEND_BAND_INFO_LEN]);
int lsf_extend_field_band_device(double *d_q, const double *d_phi, const int32_t *d_mask, const int32_t *d_known, int nx, int ny,
                                 int nz, double dx, double band, int max_passes, int *passes_done, int64_t *changed_trace,
                                 int trace_cap, int64_t info[LSF_EXTEND_BAND_INFO_LEN], void *stream);

/* ---- iso-surface extraction: the zero (or iso) level of a field as an indexed triangle mesh (marching tetrahedra) ----------
 * No reference counterpart.  What gives the moved geometry back after lsf_advect_field: the level set phi = iso as nodes
 * surfX(nSurfNode,3) and triangles surfElem(nSurfElem,3), 1-based INTEGER*4, both Fortran-ordered -- the format lsf_phi0,
 * lsf_mesh_distance, lsf_mesh_check and lsf_stl_get use -- made on the device with a numbering that is a function of the field alone.
 * The field layout is that of every other entry point, the grid point (i,j,k) is xLo + (i,j,k)*dx as in lsf_mesh_distance, and the
 * linear index of a point is p = i + (nx+1)*(j + (ny+1)*k).  info may be NULL.  Extract and keep, then copy out (as lsf_stl_read /
 * lsf_stl_get): lsf_extract_surface returns the two counts, the caller allocates, lsf_extract_get fills.
 *   field    f = phi - iso at every grid point.  A point is INSIDE when f < 0; anything else is outside: +0, -0 (phi == iso) and NaN
 *            included -- the rule of lsf_distance_fill.
 *   cells    every cell (i,j,k), 0 <= i < nx and likewise j, k, named by its lower corner c0 and ordered by c0's linear index, is cut
 *            into the six Kuhn tetrahedra: tetrahedron 0..5 for the axis orders ABC = xyz, xzy, yxz, yzx, zxy, zyx has the vertices
 *            v0 = c0, v1 = v0 + e_A, v2 = v1 + e_B, v3 = v2 + e_C.  All six share the body diagonal v0-v3; the cut of a cell face is
 *            the same seen from both cells; there are no ambiguous cases and no case table.  PARITY: tetrahedra 0, 3, 4 (even
 *            permutations of xyz) are positive, 1, 2, 5 negative.
 *   edges    every tetrahedron edge runs from a grid point a to a + d, d in {0,1}^3 \ {0}, a the LOWER endpoint.  Edge TYPE
 *            e = d_x + 2*d_y + 4*d_z - 1:  0 x, 1 y, 2 xy, 3 z, 4 xz, 5 yz (face diagonals), 6 xyz (body diagonal).  A wall point
 *            owns only the types that stay inside the grid and no cell.
 *   nodes    one per CROSSED edge (exactly one endpoint inside), numbered from 1 in ascending order of 7*p(a) + e.  With
 *            fa = phi(a) - iso, fb = phi(a + d) - iso:   t = fa / (fa - fb)   (always from the lower endpoint, the IEEE division);
 *            coordinate A of the node is xLo[A] + ((double)i_A + t) * dx where d_A = 1 and xLo[A] + (double)i_A * dx where d_A = 0,
 *            evaluated as written, left to right, without contraction.
 *   triangles  a tetrahedron with 1 or 3 vertices inside yields one triangle, with 2 inside two; "uv" is the node on the edge between
 *            its vertices u and v, neg = the tetrahedron is negative:
 *              one vertex m alone on its side, the others a < b < c:  (ma, mb, mc); the last two are swapped when
 *                  neg xor (m odd) xor (3 inside);
 *              inside p < q, outside r < s: the quad pr, ps, qs, qr is cut along pr-qs: (pr, ps, qs) then (pr, qs, qr); the last two
 *                  of each are swapped when neg xor (p + q even).
 *            Every normal (v1-v0) x (v2-v0) then points towards f >= 0 (outward): the mesh of a closed body has a positive signed
 *            volume in lsf_mesh_check, and lsf_mesh_distance gives it the sign of phi.  Triangles are ordered by (cell, tetrahedron
 *            0..5, triangle 0..1).
 *   result   nodes, connectivity, counts and info are bit-identical from run to run, between the two seams and on any stream, and
 *            equal the serial statement tests/extract_ref.py with ==.  By construction every mesh edge that does not lie in a wall
 *            face of the grid is shared by exactly two triangles that traverse it in opposite directions; a level set that reaches
 *            the grid's walls gives an OPEN mesh whose only one-triangle edges lie in wall faces.  Where phi == iso exactly on a grid
 *            point (an outside point), the nodes of its crossed edges coincide there (t == 1, or t == 0 seen from it) and zero-area
 *            triangles appear: the connectivity is still closed, nothing is welded, and lsf_mesh_check counts those triangles as
 *            degenerate.
 *   info     [0] nodes  [1] triangles  [2] cells crossed (neither all corners inside nor all outside)  [3] nodes with t == 1.
 *            Written on LSF_OK only.
 *   empty    no crossed edge: LSF_OK, both counts 0; lsf_extract_get is then LSF_OK, writes nothing and accepts NULL pointers.
 *   keep     the result stays on the device, owned by the calling thread, until lsf_extract_get / lsf_extract_get_device copies it
 *            out and releases it.  EVERY call of lsf_extract_surface[_device], a failing one included, first releases an un-fetched
 *            result: a new extraction replaces it, a failed one keeps nothing.  A get without a result (a second get too) is
 *            LSF_ERR_INVALID; so is a get with a NULL pointer, which releases nothing.  lsf_release_workspace drops the calling
 *            thread's result.  The get runs on the device of the extraction (lsf_set_device).
 *   errors   LSF_ERR_INVALID, all detected before anything is kept, with the count in lsf_last_error() where there is one: NULL phi,
 *            xLo or count pointers; nx, ny or nz < 1, or more than 2^31 - 1 points; dx not finite or <= 0; iso not finite; crossed
 *            edges with a non-finite phi - iso on an endpoint (their number, found by the counting pass; a non-finite value on no
 *            crossed edge is accepted: NaN and +inf are outside, -inf inside); more than 2^31 - 1 nodes or triangles.  No device:
 *            LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   seams    phi is an input only: lsf_extract_surface treats it under lsf_mirror exactly as lsf_narrowband treats its phi.
 *            lsf_extract_surface_device returns after the stream is synchronised (the host reads the two totals);
 *            lsf_extract_get_device copies on `stream` and returns after it is synchronised (the kept arrays are freed).
 * Workspace beyond the caller's field: 10 bytes per grid point (crossed-edge mask and corner byte, node offset and triangle offset)
 * + 24 bytes per 1024 points, and the kept mesh (24 bytes per node, 12 per triangle).  Work: one pass over the field that loads four
 * values per point, three passes over the bytes (tile sums, ONE block scanning them 1024 at a time, offsets), one pass that writes
 * the mesh; plain launches only, no block waits for another.  Out of scope: marching cubes, fp32, a band-restricted extraction,
 * multi-GPU, welding of the coincident nodes at exact zeros.
 * Not timed on hardware yet: no speed is claimed (the measurement is profiles/micro/extract_surface_time.py).
 * lsf_stl_write is host code only and needs no device (like lsf_stl_read): binary STL, an 80-byte header (blank-padded text that
 * does not begin with "solid"), the INTEGER*4 count, and per triangle the unit normal, the three vertices -- all REAL*4 -- and an
 * INTEGER*2 zero.  The vertices are the coordinates rounded to REAL*4; the normal (v1-v0) x (v2-v0) / its length is computed in
 * double from the ROUNDED vertices and is (0,0,0) for a zero-area triangle.  LSF_ERR_INVALID, all detected before the file is
 * opened (an error leaves no file): a NULL pointer, nSurfElem < 1, nSurfNode < 1, an index outside 1..nSurfNode, a coordinate that
 * is not finite as REAL*4; and a path that cannot be opened or written.  lsf_stl_read returns the float-rounded nodes in the order
 * of their first use and merges nodes that round to the same REAL*4 triple. */
#define LSF_SURF_INFO_LEN 4
int lsf_extract_surface(const double *phi, int nx, int ny, int nz, double dx, const double xLo[3], double iso,
                        int *nSurfNode, int *nSurfElem, int64_t info[LSF_SURF_INFO_LEN]);
int lsf_extract_surface_device(const double *d_phi, int nx, int ny, int nz, double dx, const double xLo[3], double iso,
                               int *nSurfNode, int *nSurfElem, int64_t info[LSF_SURF_INFO_LEN], void *stream);
int lsf_extract_get(double *surfX, int32_t *surfElem);                          /* host arrays   */
int lsf_extract_get_device(double *d_surfX, int32_t *d_surfElem, void *stream); /* device arrays */
int lsf_stl_write(const char *path, const double *surfX, int nSurfNode, const int32_t *surfElem, int nSurfElem); /* host only */

/* ---- surface and volume integrals of the level set phi = iso over the cells of a caller's mask ----------
 * No reference counterpart.  How much surface there is and how much body it encloses, without a mesh: the area, the enclosed volume
 * and its first moments (by the divergence theorem surface integrals too), the first moments of the surface and the integral of a
 * field q over it, summed over the triangles lsf_extract_surface WOULD emit for the cells of the list.  Nothing is emitted and no
 * node is numbered.  q, cell_area and info may be NULL; M is required.  xLo, M and info are host arrays on both seams.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  Any other mask value means
 *            "not in the list"; a 1 on a wall point is ignored.  The mask is read and never written.
 *   MEASURED a cell of lsf_extract_surface (named by its lower corner c0) whose c0 is in LIST.  Its seven other corners are read
 *            from the field whether they are list points or not, as the band stages read their stencils; c0 is interior, so
 *            i + 1 <= nx, j + 1 <= ny, k + 1 <= nz always hold.
 *   surface  f = phi - iso; INSIDE means f < 0, exactly as in lsf_extract_surface.  Each measured cell is cut into the same six Kuhn
 *            tetrahedra; its crossed edges carry the same nodes, t = fa / (fa - fb) from the lower endpoint a, coordinate A
 *            xLo[A] + ((double)i_A + t) * dx where the edge runs along A and xLo[A] + (double)i_A * dx where it does not; its
 *            triangles have the same vertices in the same orientation and order (tetrahedron 0..5, triangle 0..1).
 *   triangle vertices P0, P1, P2.  Evaluated exactly as written, left to right, without contraction; / and sqrt are the IEEE ones:
 *              e1 = P1 - P0;  e2 = P2 - P0                                            (per component)
 *              nx = e1y*e2z - e1z*e2y;  ny = e1z*e2x - e1x*e2z;  nz = e1x*e2y - e1y*e2x        n = e1 x e2 points outward
 *              a  = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz)
 *              cx = P1y*P2z - P1z*P2y;  cy = P1z*P2x - P1x*P2z;  cz = P1x*P2y - P1y*P2x
 *              v  = ((P0x*cx + P0y*cy) + P0z*cz) / 6.                                 the term of lsf_mesh_check's signed volume
 *              m_A = (n_A * (((P0_A+P1_A)*(P0_A+P1_A) + (P1_A+P2_A)*(P1_A+P2_A)) + (P2_A+P0_A)*(P2_A+P0_A))) / 48.     A = x, y, z
 *              s_A = a * (((P0_A + P1_A) + P2_A) / 3.)                                A = x, y, z
 *              qa  = a * (((q0 + q1) + q2) / 3.)                                      with q only
 *            q at a node is q(a) + t * (q(a+d) - q(a)): linear along the crossed edge with the node's own t.  The mean is divided
 *            BEFORE it meets a, so that q == 1 gives qa == a bit for bit ((a*3.)/3. is not a for one double in seven).  Summed over
 *            a closed surface m_A is the integral of x_A over the body (the edge-midpoint rule, exact for x_A^2 n_A / 2 on a flat
 *            triangle) and s_A that of x_A over the surface.
 *   cell     a cell's contribution to each quantity starts at 0.0 and adds its triangles in their order.
 *   M        {area, volume, int x dV, int y dV, int z dV, int x dS, int y dS, int z dS, int q dS}; M[8] is 0.0 without q.  Each
 *            total is the sum of the per-cell contributions over the measured cells, in an order that is a function of field and
 *            mask alone: the brick-sorted list of lsf_reinit_band, one cell per lane, an xor butterfly over the 64 lanes of a
 *            wave, the four waves of a block of 256 entries in wave order, the blocks in block order on the host.  The totals are
 *            bit-identical from run to run, between the two seams and on any stream -- the promise the RMS of lsf_reinit_band
 *            makes.  They are NOT bit-identical to a sequential sum: with N crossed measured cells a total differs from the exact
 *            sum of the contributions by at most N * 2^-53 * sum|contribution|, the bound of any order of summation.
 *            volume and the three volume moments mean what their names say for a closed surface wholly inside the list; info[3]
 *            says when that fails.  They are taken about the origin of xLo's frame, as lsf_mesh_check's volume is: a body far
 *            from that origin loses digits to cancellation, and a caller who cares passes a shifted xLo.  The centroid of the
 *            body is M[2..4] / M[1], that of the surface M[5..7] / M[0].
 *   cell_area  optional, phi's layout.  At EVERY list point the area of the surface inside the cell it names -- that cell's
 *            contribution to `area`, 0.0 for an uncrossed cell; nothing is written anywhere else.  No order of summation enters
 *            it: it is the serial statement's bit for bit, the discrete delta(phi) |grad(phi)| dx^3.  It must not share a byte
 *            with phi, mask or q.
 *   info     [0] list cells; [1] crossed measured cells; [2] triangles; [3] OPEN crossed cells: crossed measured cells with at
 *            least one of the six face-neighbour cells (lower corners c0 +- e_A) not in LIST, a wall point included -- then the
 *            surface may continue outside the list and M describes an open piece; [4] triangles with a == 0.0, the exact zeros of
 *            phi - iso on grid points that lsf_extract_surface documents.  Written on LSF_OK only.  When every crossed cell of the
 *            grid has an interior lower corner in LIST, info[1] and info[2] equal lsf_extract_surface's info[2] and info[1].
 *   empty    an empty list, or no crossed measured cell: LSF_OK, M all 0.0, the counts as found, cell_area 0.0 at list points.
 *   errors   LSF_ERR_INVALID, all detected before anything is written, with the count in lsf_last_error() where there is one: a
 *            NULL phi, mask, xLo or M; the dimensions lsf_reinit_band refuses; dx not finite or <= 0; iso or a component of xLo
 *            not finite; cell_area overlapping phi, mask or q; a crossed edge of a measured cell with a non-finite phi - iso on an
 *            endpoint; with q, one with a non-finite q on an endpoint.  Both are counted once per measured cell that holds the
 *            edge (the 19 edges of its six tetrahedra), phi first.  q is read at those endpoints only: a NaN anywhere else is
 *            legal, so the kappa / gauss that lsf_curvature_band leaves NaN off its list plug straight in.  No device:
 *            LSF_ERR_NO_DEVICE -- there is no CPU fallback, no mode word, one arithmetic.
 *   result   cell_area and info equal the serial statement tests/measure_ref.py with ==, M within the bound above.
 *   seams    lsf_measure_band takes phi through its twin under lsf_mirror as lsf_extract_surface does and the mask as
 *            lsf_reinit_band does; q is staged as lsf_advect_field stages its inputs; cell_area has no twin: it is staged in a
 *            slot of its own as lsf_curvature_band stages its outputs, copied in on every call and copied back on LSF_OK only.
 *            lsf_measure_band_device returns after the stream is synchronised (the host finishes the per-block partials).
 * Guidance: the corners of a crossed cell have |phi| <= sqrt(3) dx on a distance field, so any mask of |phi| < 2.1 dx or wider
 * contains them; a closed surface needs every crossed cell's lower corner in the list (info[3] tells).  SECOND ORDER (serial
 * statement, sphere of radius 0.6, every interior point listed): the area is 1.12 % low on 25^3 points and 0.28 % on 49^3, the
 * volume 2.17 % and 0.54 % -- the polyhedron is inscribed.
 * Work: the list build of lsf_reinit_band and two launches over the list (validation, then the sums); 8 gathered loads per list
 * cell (16 with q) and the nodes of the crossed ones; the host reads 104 bytes per 256 list cells.  Workspace: that of the list;
 * the host seam adds one field for q and one for cell_area.  Out of scope: fp32, multi-GPU, a per-step trace inside
 * lsf_evolve_band, second moments, integrals over the interior cells instead of the divergence theorem.
 * Timed once on one MI355X beside lsf_curvature_band (all three outputs) on the same sphere and mask |phi| < 8.1 dx and beside
 * lsf_extract_surface + lsf_extract_get_device on the same field (profiles/measure_band_time.txt, from
 * profiles/micro/measure_band_time.py; device seam, ms per call, list build included): 0.36 against 0.24 and 0.68 at 256^3 (34 070
 * of 372 155 list cells crossed), 0.84 against 0.53 and 2.36 at 512^3.  No speed is claimed beyond that record. */
#define LSF_MEASURE_LEN 9
#define LSF_MEASURE_INFO_LEN 5
int lsf_measure_band(const double *phi, const int32_t *mask, const double *q, double *cell_area, int nx, int ny, int nz, double dx,
                     const double xLo[3], double iso, double M[LSF_MEASURE_LEN], int64_t info[LSF_MEASURE_INFO_LEN]);
int lsf_measure_band_device(const double *d_phi, const int32_t *d_mask, const double *d_q, double *d_cell_area, int nx, int ny,
                            int nz, double dx, const double xLo[3], double iso, double M[LSF_MEASURE_LEN],
                            int64_t info[LSF_MEASURE_INFO_LEN], void *stream);

/* ---- cut-cell volume fractions and face apertures on the cells of a caller's mask ----------
 * No reference counterpart.  What an embedded-boundary (cut-cell) flow solver needs of a level-set geometry: per cell of the list how
 * much of it lies inside the body phi < iso, how much of each lower face is open to it, the surface's area vector inside the cell,
 * and over the list the body's volume and the smallest cut-cell fraction (the "small cell" number).  The volume is an integral over
 * cells: it needs no closed surface inside the list.  The per-cell outputs have phi's layout.  volume, vof_min and info are host
 * scalars / a host array on both seams; all three may be NULL.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  Any other mask value means
 *            "not in the list"; a 1 on a wall point is ignored.  The mask is read and never written.
 *   cell     a list point c0 names the cell whose lower corner it is.  Its seven other corners are read from phi whether they are
 *            listed or not (c0 is interior, so i + 1 <= nx, j + 1 <= ny, k + 1 <= nz always hold).  f = phi - iso; INSIDE means
 *            f < 0.  The corner byte has bit x + 2y + 4z set where that corner is inside.  The cell is cut into the six Kuhn
 *            tetrahedra of lsf_extract_surface; nodes (t = fa / (fa - fb) from the lower endpoint u < v of a crossed edge),
 *            triangles, their orientation and their order (tetrahedron 0..5, triangle 0..1) are that call's.
 *   units    everything per cell is computed in CELL UNITS: c0 at the origin, dx = 1.  Coordinate A of the node on the edge {u, v}
 *            is bit_A(u) + t where the edge runs along A and bit_A(u) where it does not -- the node of lsf_measure_band with
 *            xLo = 0, (i,j,k) = 0 and dx = 1.  The per-cell outputs therefore do not depend on dx.
 *   s(m, j)  the fraction of the edge from corner m to the zero crossing on the edge {m, j}: the node's own t when m is the edge's
 *            lower endpoint, 1.0 - t otherwise.
 *   tri(a, b, c)  the inside fraction of a face triangle with linear f: no vertex inside 0.0; all three 1.0; one inside, m, the
 *            others o1, o2: s(m,o1) * s(m,o2); two inside i1, i2 and o outside: 1.0 - s(o,i1) * s(o,i2).
 *   face(A, base)  the aperture of the face normal to axis A at base in {0, 1 << A}, with b < c the bits of the two other axes:
 *              face = 0.5 * (tri(base, base|b, base|b|c) + tri(base, base|c, base|b|c))
 *            -- the face cut along the Kuhn diagonal base - base|b|c, as the tetrahedra cut it.  The upper face of c0 is, bit for
 *            bit, the lower face of c0 + e_A: the same four values through the same function.
 *   outputs  at a list point (written at list points only, never anywhere else):
 *              ax, ay, az   face(A, 0), the LOWER faces (the MAC convention: the upper face belongs to the neighbour);
 *              bx, by, bz   the sum of 0.5 * n_A over the cell's triangles, n = (P1 - P0) x (P2 - P0) written as in
 *                           lsf_measure_band, added to 0.0 in emission order: the surface's outward area vector in units of dx^2
 *                           (b_A = face(A, 0) - face(A, 1 << A) up to rounding: the cell's inside part is closed);
 *              vof          V = the sum of ((P0x*cx + P0y*cy) + P0z*cz) / 6. over the triangles, c = P1 x P2 as in lsf_measure_band,
 *                           added to 0.0 in emission order;  raw = ((up_x + up_y) + up_z) / 3. + V  with up_A = face(A, 1 << A)
 *                           -- the divergence theorem about c0, to which the lower faces contribute nothing;  the stored value is
 *                           raw < 0 ? 0.0 : (raw > 1 ? 1.0 : raw).
 *            Corner byte 0: vof = a = b = 0.0.  Corner byte 255: vof = 1.0, a = 1.0, b = 0.0.  Everything is evaluated exactly as
 *            written, left to right, without contraction; there is one arithmetic and no mode word.
 *   groups   vof, {ax, ay, az} and {bx, by, bz}: each group is given whole or left NULL.  At least one group, or volume, is given.
 *   totals   volume = (the sum of the stored vof over the list cells) * ((dx * dx) * dx), summed in lsf_measure_band's fixed order
 *            (an xor butterfly over the 64 lanes of a wave, the waves of a block of 256 entries in wave order, the blocks in block
 *            order on the host): bit-identical from run to run, between the seams and on any stream, and within
 *            N * 2^-53 * sum|vof| of the exact sum for N non-zero fractions.  vof_min: the smallest stored vof over the CUT cells
 *            (corner byte neither 0 nor 255), +inf when there is none.
 *   info     [0] list cells; [1] cut cells; [2] full cells (byte 255); [3] OPEN cut cells: at least one of the six face-neighbour
 *            cells (lower corners c0 +- e_A) is not in LIST, a wall point included, so the caller lacks some aperture next to
 *            it (lsf_measure_band's info[3]); [4] cut cells whose raw was clamped.  Written on LSF_OK only.
 *   empty    an empty list: LSF_OK, info all 0, volume 0.0, vof_min +inf, nothing else written.
 *   errors   LSF_ERR_INVALID, all detected before anything is written, with the count in lsf_last_error() where there is one: a
 *            NULL phi or mask; the dimensions lsf_reinit_band refuses; dx not finite or <= 0; iso not finite; an incomplete
 *            group; nothing requested; an output sharing a byte with phi, the mask or another output; a crossed edge of a listed
 *            cell with a non-finite phi - iso on an endpoint, counted as lsf_measure_band counts it.  No device:
 *            LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   result   every per-cell output, info and vof_min equal the serial statement tests/cut_cells_ref.py with ==, volume within the
 *            bound above.
 *   seams    lsf_cut_cells_band takes phi through its twin under lsf_mirror as lsf_measure_band does and the mask as
 *            lsf_reinit_band does; each given output is staged in a slot of its own as cell_area is: copied in on every call,
 *            copied back on LSF_OK only, no twin.  lsf_cut_cells_band_device returns after the stream is synchronised.
 * Guidance: to have every aperture of every cut cell (the upper faces are the neighbours' lower ones), dilate the mask by one cell.
 * A mask of phi < 2.1 dx (the inside plus a rim) makes volume the body's volume with no closed-surface assumption.  The fraction is
 * that of the polyhedron lsf_extract_surface emits: second order, 2.17 % low on the sphere of radius 0.6 at 25^3 points, 0.54 % at
 * 49^3.  Work: the list build and two launches over the list; 8 gathered loads per list cell, and for a cut cell its nodes and up to
 * 24 edge fractions.  Workspace: that of the list; the host seam adds one field per given output.  Out of scope: fp32, multi-GPU,
 * volume and face centroids, second moments, a per-step trace inside lsf_evolve_band, cell merging.
 * Timed once on one MI355X beside lsf_measure_band (totals only) and lsf_curvature_band (all three outputs) on the same sphere and
 * mask |phi| < 8.1 dx (profiles/cut_cells_time.txt, from profiles/micro/cut_cells_time.py; device seam, ms per call, list build
 * included): 0.34 with all outputs and 0.32 with volume only against 0.38 and 0.26 at 256^3 (34 070 of 372 155 list cells cut),
 * 0.68 and 0.62 against 0.82 and 0.52 at 512^3.  No speed is claimed beyond that record. */
#define LSF_CUT_INFO_LEN 5
int lsf_cut_cells_band(const double *phi, const int32_t *mask, int nx, int ny, int nz, double dx, double iso, double *vof, double *ax,
                       double *ay, double *az, double *bx, double *by, double *bz, double *volume, double *vof_min,
                       int64_t info[LSF_CUT_INFO_LEN]);
int lsf_cut_cells_band_device(const double *d_phi, const int32_t *d_mask, int nx, int ny, int nz, double dx, double iso, double *d_vof,
                              double *d_ax, double *d_ay, double *d_az, double *d_bx, double *d_by, double *d_bz, double *volume,
                              double *vof_min, int64_t info[LSF_CUT_INFO_LEN], void *stream);

/* ---- the field at arbitrary points: value, gradient, a second field and the foot point on phi = iso ----------
 * No reference counterpart (its setPhiSurf is private to lsf_advect_nodes, trilinear only, moves a node on the positive side only and
 * clamps instead of refusing).  A caller that holds particles, the nodes of another mesh or the nodes lsf_extract_surface has just
 * returned asks the grid a question: a pure gather, one lane per point, in the caller's order.  mask, q, grad, qval, foot, status and
 * info may be NULL; qval requires q, foot requires iters >= 1; q without a mask is legal and is then read wherever the stencil goes.
 * phi, mask, q and pts are inputs only.  xLo and info are host arrays on both seams.
 *   arrays   pts, grad and foot are REAL a(npts,3) in Fortran order: point t has x at [t], y at [t + npts], z at [t + 2 npts] -- the
 *            layout of surfX, so the output of lsf_extract_get / lsf_extract_get_device plugs in.  val, qval and status have npts
 *            entries.  phi, mask and q are fields of (nx+1)(ny+1)(nz+1) points; the grid point (i,j,k) is xLo + (i,j,k) dx.
 *   exact    every expression below is evaluated left to right as written, without contraction, with the IEEE / and sqrt: the numpy
 *            transcription tests/sample_ref.py is the yardstick bit for bit.
 *   locate   per axis A, n = nx, ny, nz:  s = (x - xLo[A]) / dx.  The point is INSIDE on that axis when s >= 0 && s <= n, compared
 *            in double BEFORE any conversion to an integer: NaN, +-inf and 1e300 fail it and never reach an index.
 *            i0 = min((int)floor(s), n - 1), so the upper wall belongs to the last cell with t = 1;  t = s - (double)i0.  A point
 *            that is not INSIDE on all three axes gets status LSF_SAMPLE_OUTSIDE.
 *   stencil  LSF_SAMPLE_CUBIC is used when 1 <= i0 <= n - 2 on ALL three axes (the joint rule, as for WENO in lsf_advect_field): the
 *            4 x 4 x 4 points i0 - 1 .. i0 + 2.  Otherwise, and always for LSF_SAMPLE_LINEAR, the 2 x 2 x 2 corners of the cell.  A
 *            cubic request served linearly is counted in info[3].
 *   band     with a mask a stencil point is IN when it is an interior point (1..n-1 on each axis) with mask == 1, the LIST rule of
 *            lsf_reinit_band.  A point whose used stencil holds a point that is not IN gets status LSF_SAMPLE_OFFBAND.  This is what
 *            makes q = kappa of lsf_curvature_band, written at list cells only, safe to sample.
 *   weights  cubic (Catmull-Rom):   w0 = 0.5*(((2.-t)*t-1.)*t)       w1 = 0.5*((3.*t-5.)*t*t+2.)
 *                                   w2 = 0.5*(((4.-3.*t)*t+1.)*t)    w3 = 0.5*((t-1.)*t*t)
 *            its derivative:        d0 = 0.5*((4.-3.*t)*t-1.)        d1 = 0.5*((9.*t-10.)*t)
 *                                   d2 = 0.5*((8.-9.*t)*t+1.)        d3 = 0.5*((3.*t-2.)*t)
 *            linear:                w0 = 1.-t, w1 = t;  d0 = -1., d1 = 1.
 *   value    contract along x first: r = ((w0*a0 + w1*a1) + w2*a2) + w3*a3, or w0*a0 + w1*a1 for linear; then the row results along y
 *            in the same form, then z.  val is that result for phi, qval the same for q.  grad[A] is the same contraction with d in
 *            place of w on axis A, divided by dx at the end.  At t = 0 the linear value is the grid value with ==.
 *   refused  for an OUTSIDE or OFFBAND point val, grad, qval and foot are NaN and nothing else of the point is computed.
 *   foot     iters >= 1: the foot of the point on phi = iso, on both sides of the surface.  Start with y = x.  At most iters times:
 *            sample v, g at y by the rules above; e = v - iso; if !(fabs(e) > tol*dx) converged; m = (g0*g0 + g1*g1) + g2*g2;
 *            if m == 0 status LSF_SAMPLE_FLAT, stop; y_A = y_A - (e * g_A) / m.  After the last move y is sampled once more for the
 *            convergence test; not converged: LSF_SAMPLE_NOT_CONVERGED.  A y that becomes OUTSIDE or OFFBAND ends the loop with that
 *            status.  foot holds the last y in every case except OUTSIDE / OFFBAND of the original point.  val, grad and qval always
 *            belong to the original point.  Precedence: the original point's OUTSIDE / OFFBAND first, then whatever ended the loop.
 *            The foot follows the interpolant's gradient: it is the closest point where phi is a distance, a point of the level set
 *            anywhere else.
 *   info     [0] points with status OK; [1] OUTSIDE; [2] OFFBAND; [3] linear fallbacks of a cubic request, among the points whose own
 *            sample was taken; [4] FLAT; [5] NOT_CONVERGED.  [0] + [1] + [2] + [4] + [5] == npts.  Integer counts: no order of
 *            summation enters them.  Written on LSF_OK only.
 *   errors   LSF_ERR_INVALID, all detected before any output is written: a NULL phi, pts, val or xLo; npts < 1; nx, ny or nz < 1 or
 *            more than 2^31 - 1 points; dx or xLo not finite, dx <= 0; iso not finite; an unknown order; iters < 0; iters >= 1 with
 *            tol not finite or < 0; qval without q; foot with iters == 0; any output sharing a byte with another output or with an
 *            input.  A non-finite phi or q VALUE is not an error: it flows into the outputs as NaN / inf, like any interpolation.
 *            No device: LSF_ERR_NO_DEVICE -- there is no CPU fallback, no mode word, one arithmetic.
 *   seams    lsf_sample_points takes phi through its twin under lsf_mirror as lsf_extract_surface does and the mask as
 *            lsf_curvature_band does; q is staged in a slot of its own (from its device twin where a current one exists under
 *            LSF_MIRROR_TRUST / LAZY) and never copied back; pts and the outputs are staged per call and the outputs come home on
 *            LSF_OK only.  lsf_sample_points_device returns after the stream is synchronised (the host finishes the block counts).
 *   flat     m == 0 is exact: on a constant field the linear gradient -a + a is 0.0 and the point is FLAT; the cubic d weights sum
 *            to 0 only to rounding, so a cubic request there may see a gradient of 1e-17, take a wild step and end OUTSIDE.
 * Accuracy (the statement, cubic, on phi = |x| - 0.25 over [-0.5, 0.5]^3 at points within 1.5 dx of the surface; 13^3 / 25^3 / 49^3
 * grid points): largest value error 2.0e-2 / 2.7e-3 / 4.3e-4 dx, largest gradient error 8.3e-2 / 8.8e-3 / 1.7e-3, largest foot
 * error (iters = 5, tol = 1e-9) 8.5e-2 / 1.1e-2 / 2.5e-3 dx.
 * Work: one launch; 8 or 64 gathered loads per sample and field (the mask as many), 1 + (moves made) samples per point.  Workspace:
 * 48 bytes per 256 points; the host seam adds one field for q and 92 bytes per point.  Out of scope: fp32, multi-GPU, binning or
 * sorting the points by brick, several q in one call, q sampled at the foot (project first, then sample), exact closest points
 * where the field is no distance, higher-order or monotone interpolants, the mesh -> grid scatter.
 * Timed once on one MI355X at the nodes of lsf_extract_surface on a sphere, in cell order and under a fixed random permutation,
 * beside lsf_curvature_band (kappa only) on the mask |phi| < 8.1 dx of the same field (profiles/sample_points_time.txt, from
 * profiles/micro/sample_points_time.py; device seam, ms per call): at 256^3 (101 898 nodes) linear 0.059 / shuffled 0.059, cubic
 * 0.055 / 0.061, cubic with iters = 3 0.061 / 0.078, cubic with q = kappa and the mask 0.077 / 0.112 against 0.257 for the curvature
 * call; at 512^3 (408 902 nodes) linear 0.064 / 0.073, cubic 0.072 / 0.130, cubic with iters = 3 0.085 / 0.197, cubic with q and the
 * mask 0.119 / 0.372 against 0.517.  No speed is claimed beyond that record. */
#define LSF_SAMPLE_LINEAR 0 /* order */
#define LSF_SAMPLE_CUBIC 1
#define LSF_SAMPLE_INFO_LEN 6
#define LSF_SAMPLE_OK 0 /* status[t] */
#define LSF_SAMPLE_OUTSIDE 1
#define LSF_SAMPLE_OFFBAND 2
#define LSF_SAMPLE_FLAT 3
#define LSF_SAMPLE_NOT_CONVERGED 4
int lsf_sample_points(const double *phi, const int32_t *mask, const double *q, int nx, int ny, int nz, double dx, const double xLo[3],
                      const double *pts, int npts, int order, double iso, int iters, double tol, double *val, double *grad,
                      double *qval, double *foot, int32_t *status, int64_t info[LSF_SAMPLE_INFO_LEN]);
int lsf_sample_points_device(const double *d_phi, const int32_t *d_mask, const double *d_q, int nx, int ny, int nz, double dx,
                             const double xLo[3], const double *d_pts, int npts, int order, double iso, int iters, double tol,
                             double *d_val, double *d_grad, double *d_qval, double *d_foot, int32_t *d_status,
                             int64_t info[LSF_SAMPLE_INFO_LEN], void *stream);

/* ---- the first hit of a ray with the level set: what the surface looks like from over there ----------
 * No reference counterpart.  Line-of-sight speed laws and shadowing, wall thickness (cast from a node of lsf_extract_surface against
 * its normal), depth images of the moved geometry without a mesh, probes: one lane per ray, in the caller's order, marching by
 * the field's own value between samples of lsf_sample_points' interpolant and skipping what a band list does not hold.  mask, q,
 * hit, grad, qval, status and info may be NULL; qval requires q.  phi, mask, q, org and dir are inputs only.  xLo and info are host
 * arrays on both seams.
 *   arrays   org, dir, hit and grad are REAL a(nrays,3) in Fortran order, the layout of surfX and of pts of lsf_sample_points; thit,
 *            qval and status have nrays entries.  phi, mask and q are fields of (nx+1)(ny+1)(nz+1) points.
 *   exact    every expression below is evaluated left to right as written, without contraction, with the IEEE / and sqrt: the numpy
 *            transcription tests/cast_ref.py is the yardstick bit for bit.  fmax(a, b) and fmin(a, b) are defined HERE: b where a
 *            is NaN; else a where b is NaN or a >= b (fmin: a <= b); else b.  That is C's fmax / fmin with the one thing C leaves
 *            open decided: on a tie, +0 against -0 included, the FIRST argument is returned.
 *   ray      o = org, d = dir of the ray.  A component of o or d that is not finite: status LSF_CAST_BAD.  L = sqrt((d0*d0 + d1*d1)
 *            + d2*d2); !(L > 0) or L not finite (a zero direction, 1e300): BAD.  u_A = d_A / L; every t below is a length.
 *   clip     slabs.  t0 = tmin, t1 = tmax; per axis A, n = nx, ny, nz:  lo = xLo[A], hi = xLo[A] + (double)n*dx.  u_A == 0: when
 *            !(o_A >= lo && o_A <= hi) status LSF_CAST_NOGRID.  Otherwise a = (lo - o_A)/u_A, b = (hi - o_A)/u_A,
 *            t0 = fmax(t0, fmin(a, b)), t1 = fmin(t1, fmax(a, b)).  After the three axes !(t0 <= t1): NOGRID.
 *   sample   at t the point is p_A = o_A + t*u_A.  Per axis s = (p_A - xLo[A]) / dx; the sample is refused as OUTSIDE when
 *            !(s >= -1e-6 && s <= (double)n + 1e-6), compared in double BEFORE any conversion to an integer -- the only guard
 *            between a wild ray and a load; the tolerance takes in the rounding of a point that the clip has put on a wall.  Then
 *            s = fmin(fmax(s, 0.), (double)n), i0 = min((int)floor(s), n - 1), t = s - (double)i0.  From here on the sample is
 *            lsf_sample_points': its stencil (the joint rule), its band rule (with a mask every stencil point an interior point
 *            with mask == 1, else the sample is OFF THE LIST and nothing of phi is read), its weights and its contraction.  At a
 *            point with 0 <= s <= n on every axis a ray sample equals lsf_sample_points at that point with ==.
 *   march    state: the reference (tr, er), the last on-list sample with e = v - iso; a flag gap, false at the start; a step
 *            count.  The first sample is at t = t0; after each sample that does not end the ray the next one is at
 *            tn = t + step, and if !(tn < t1) then tn = t1 and that sample is the LAST.  A sample, in this order:
 *              OUTSIDE                         status LSF_CAST_MISS, thit = t.
 *              off the list (mask only)        gap = true; step = skip*dx.
 *              on the list, no reference yet   it becomes the reference, gap = false; e == 0: a hit at t (bracket [t, t], no
 *                                              bisection, on to the full sample).
 *              on the list, with a reference   a CROSSING when e == 0 || (e > 0) != (er > 0); NaN counts as not > 0.  A crossing
 *                                              with gap set: status LSF_CAST_LOST -- the surface was crossed where the list has no
 *                                              cells, the ray's version of info[3] of lsf_measure_band.  A crossing without:
 *                                              the bracket is [ta, tb] = [tr, t], ea = er, eb = e, on to the refinement.  No
 *                                              crossing: the sample becomes the reference, gap = false.
 *              step (on the list)              step = fmin(fmax(safety*fabs(er), smin*dx), smax*dx), er the reference just set.
 *              it was the LAST sample          status MISS, thit = t.
 *              max_steps steps made already    status LSF_CAST_STEPS.  Otherwise one more step is counted.
 *            So a ray takes the first sample and at most max_steps further ones.
 *   refine   `refine` times: tm = 0.5*(ta + tb), sample there; refused (OUTSIDE or off the list): LOST; em = v - iso; when
 *            em == 0 || (em > 0) != (ea > 0) then tb = tm, eb = em, else ta = tm, ea = em.  Then quo = (ea*(tb - ta))/(eb - ea);
 *            th = ta - quo when eb != ea and quo is finite, else th = ta; th = fmin(fmax(th, ta), tb).  One full sample at th,
 *            with q where given: refused: LOST; else status LSF_CAST_HIT, thit = th, hit = o + th*u as sampled, grad and qval
 *            that sample's.
 *   outputs  a ray that is not HIT holds NaN in hit, grad and qval; thit is NaN for BAD, NOGRID, LOST and STEPS and the end of the
 *            march for MISS.  Every entry of every output given is written.
 *   info     [0..5] rays with status HIT, MISS, NOGRID, BAD, LOST, STEPS -- they add up to nrays; [6] samples of phi taken (every
 *            on-list sample of the march and the refinement and the full sample of a HIT); [7] off-list strides (off-list samples
 *            of the march); [8] rays that began on the inner side (e < 0 at their first reference).  Integer counts: no order of
 *            summation enters them.  Written on LSF_OK only.
 *   errors   LSF_ERR_INVALID, all detected before any output is written: a NULL phi, org, dir, thit or xLo; nrays < 1; nx, ny or
 *            nz < 1 or more than 2^31 - 1 points; dx or xLo not finite, dx <= 0; iso not finite; an unknown order; tmin not finite
 *            or < 0; tmax not finite or <= tmin; safety outside (0, 1]; smin not finite or <= 0; smax not finite or < smin; skip
 *            not finite or <= 0 (looked at with or without a mask); refine < 0; max_steps < 1; qval without q; any output sharing
 *            a byte with another output or with an input.  A non-finite phi or q VALUE is not an error: NaN is "not > 0".
 *            No device: LSF_ERR_NO_DEVICE -- there is no CPU fallback, no mode word, one arithmetic.
 *   seams    lsf_sample_points' own: phi through its twin under lsf_mirror, the mask as lsf_curvature_band takes it, q in a slot
 *            of its own and never copied back; org, dir and the outputs are staged per call and the outputs come home on LSF_OK
 *            only.  lsf_cast_rays_device returns after the stream is synchronised (the host finishes the block counts).
 * Guidance: where phi is a distance, safety <= 1 cannot step over the surface and smin bounds the work next to a grazing ray;
 * smax = 1 keeps a step inside the cells the last sample saw where phi is no distance.  skip <= the band's half width in cells
 * cannot jump a band.  A ray that starts inside the body (info[8]) hits the surface from within: thit is then the way OUT.
 * Accuracy (the statement on phi = |x| - 0.25 over [-0.5, 0.5]^3, 400 rays from outside the box aimed into the body, safety 0.9,
 * smin 0.05, smax 1, refine 30; 13^3 / 25^3 / 49^3 grid points; largest |thit - analytic| / dx, measured):
 * linear 1.39e-1 / 6.28e-2 / 3.29e-2, cubic 7.89e-3 / 1.58e-3 / 5.05e-4; as a length the linear error falls 4.4 x and 3.8 x per halving.
 * Work: one launch; 8 or 64 gathered loads per sample (the mask as many, 8 for most off-list strides); a wave runs as long as its longest ray.  Workspace:
 * 72 bytes per 256 rays; the host seam adds one field for q and 116 bytes per ray.  Out of scope: fp32, multi-GPU, secondary rays
 * and flux integrals over a hemisphere (a caller loops over directions), exact cell-by-cell traversal with the root of the cubic
 * along the ray, sorting rays for coherence, all hits of a ray instead of the first.
 * Timed once on one MI355X on a 512 x 512 pinhole image of two spheres (exact distance; 40 % of the rays hit), without a mask with
 * smax = 1 / smax = 8 / with the mask |phi| < 8.1 dx and skip = 4, beside lsf_sample_points with iters = 3 on as many points
 * (profiles/cast_rays_time.txt, from profiles/micro/cast_rays_time.py; device seam, ms per call, samples of phi per ray in
 * brackets): at 256^3 linear 0.857 [203] / 0.444 [39] / 0.542 [21 and 46 strides] against 0.066, cubic 1.866 / 0.996 / 1.440
 * against 0.081; at 512^3 linear 1.611 [393] / 0.662 [63] / 0.865 [20 and 94 strides] against 0.069, cubic 3.883 / 1.753 / 2.150
 * against 0.088.  The band rule is read with its loads side by side, not with lsf_sample_points' early exit.
 * No speed is claimed beyond that record. */
#define LSF_CAST_INFO_LEN 9
#define LSF_CAST_HIT 0 /* status[r] */
#define LSF_CAST_MISS 1
#define LSF_CAST_NOGRID 2
#define LSF_CAST_BAD 3
#define LSF_CAST_LOST 4
#define LSF_CAST_STEPS 5
int lsf_cast_rays(const double *phi, const int32_t *mask, const double *q, int nx, int ny, int nz, double dx, const double xLo[3],
                  const double *org, const double *dir, int nrays, int order, double iso, double tmin, double tmax, double safety,
                  double smin, double smax, double skip, int refine, int max_steps, double *thit, double *hit, double *grad,
                  double *qval, int32_t *status, int64_t info[LSF_CAST_INFO_LEN]);
int lsf_cast_rays_device(const double *d_phi, const int32_t *d_mask, const double *d_q, int nx, int ny, int nz, double dx,
                         const double xLo[3], const double *d_org, const double *d_dir, int nrays, int order, double iso, double tmin,
                         double tmax, double safety, double smin, double smax, double skip, int refine, int max_steps,
                         double *d_thit, double *d_hit, double *d_grad, double *d_qval, int32_t *d_status,
                         int64_t info[LSF_CAST_INFO_LEN], void *stream);

/* ---- points carried through the fields that move phi ----------
 * No reference counterpart (lsf_advect_nodes is the reference's own surface-node scheme and stays as it is).  Tracers, the nodes of
 * lsf_extract_surface, the markers of a particle level set, or points traced backwards with dt < 0 move along
 *     x' = (u, v, w)(x) + speed(x) * grad phi(x) / |grad phi(x)|
 * in fields that are frozen for the call: the law under which lsf_advect_field and lsf_evolve_band move phi.  One lane per point, in
 * the caller's order, the interpolant of lsf_sample_points unchanged.  u, v, w come together or all NULL; speed is optional; phi is
 * required exactly when speed is given (phi without speed is refused); at least one of the two groups is present.  mask, status,
 * cfl and info may be NULL.  xLo, cfl and info are host memory on both seams.  Every field is an input only.
 *   arrays   pts is REAL a(npts,3) in Fortran order, in and out; status has npts entries.  The fields have (nx+1)(ny+1)(nz+1) points.
 *   exact    every expression below is evaluated left to right as written, without contraction, with the IEEE / and sqrt: the numpy
 *            transcription tests/points_ref.py is the yardstick bit for bit.
 *   sample   K(y): the rules locate, stencil (the joint cubic rule with its linear fallback), band, weights and value of
 *            lsf_sample_points apply word for word, to every field under one set of weights; the sample is OK, OUTSIDE or OFFBAND.
 *            U_A is the value of u, v, w.  With speed: f the value of speed, g the grad of phi (its division by dx included),
 *            m = (g0*g0 + g1*g1) + g2*g2; m == 0: the sample is FLAT; nrm = sqrt(m); k_A = U_A + (f*g_A)/nrm, or k_A = (f*g_A)/nrm
 *            without the velocity group.  Without speed k_A = U_A.
 *   step     LSF_ADVECT_RK3 from x0:  k = K(x0); x1_A = x0_A + dt*k_A
 *                                     k = K(x1); x2_A = 0.75*x0_A + 0.25*(x1_A + dt*k_A)
 *                                     k = K(x2); xn_A = (1./3.)*x0_A + (2./3.)*(x2_A + dt*k_A)
 *            LSF_ADVECT_EULER: xn = x1.  A step COMPLETES when each of its samples was OK and xn is INSIDE on all three axes by
 *            locate.  Otherwise the point keeps the bits of x0, takes the status of what failed -- the first failed sample's
 *            OUTSIDE, OFFBAND or FLAT (later stages are not sampled); OUTSIDE for a wild xn, NaN included -- and stops.
 *   status   a point that completes nsteps steps is LSF_POINTS_OK.  A point that is not INSIDE on entry (NaN, +-inf, 1e300) is
 *            returned bit for bit with LSF_POINTS_OUTSIDE.  Every other returned point lies in the grid.  A non-finite field VALUE
 *            is not an error: it makes a position non-finite, and that position fails locate before any index exists.
 *   cfl      the largest fabs(dt*k_A)/dx over the stages and axes of completed steps, 0.0 if there is none; a maximum of bit
 *            patterns, so no order of reduction enters it.
 *   info     [0] points with status OK; [1] OUTSIDE; [2] OFFBAND; [3] FLAT -- they add up to npts; [4] completed steps summed over
 *            the points; [5] samples with status OK that served a cubic request linearly (every OK sample taken counts, those of a
 *            step that fails later included).  Written on LSF_OK only.
 *   errors   LSF_ERR_INVALID, all detected before anything is written: a NULL pts or xLo; a partial u, v, w; no group at all; speed
 *            and phi not given together; npts < 1; nx, ny or nz < 1 or more than 2^31 - 1 points; dx, xLo or dt not finite,
 *            dx <= 0; an unknown order or scheme; nsteps outside 1..LSF_ADVECT_POINTS_MAX_STEPS (the cap keeps a launch bounded: a
 *            caller loops for more); pts or status sharing a byte with each other or with an input.
 *            No device: LSF_ERR_NO_DEVICE with nothing written -- there is no CPU fallback, no mode word, one arithmetic.
 *   seams    u, v, w and speed are staged as lsf_advect_field stages them, phi goes through its twin as in lsf_sample_points, the
 *            mask as lsf_curvature_band takes it; pts is copied in on every call and comes home with status on LSF_OK only.
 *            lsf_advect_points_device returns after the stream is synchronised (the host finishes the block partials).
 * Accuracy: third order in dt for RK3 on smooth fields; a constant velocity is an exact translation to rounding, a rigid rotation
 * conserves the radius to third order (tests/test_points_cpu.py).  Work: one launch; per stage 8 or 64 gathered loads per field read
 * (the mask as many).  Workspace: 56 bytes per 256 points; the host seam adds up to four fields and 28 bytes per point.  Out of
 * scope: a velocity that changes inside a call, points sorted by brick, fp32, multi-GPU.
 * Kernel: 12 instances (order x velocity / speed / both x mask), 78 - 245 VGPRs, none with scratch.
 * Timed once on one MI355X on the markers of seedParticles(per_cell=16) around a sphere, in cell order, with the mask
 * |phi| < 8.1 dx (profiles/points_time.txt, from profiles/micro/points_time.py; device seam, ms per call, one RK3 step): at 256^3
 * (1 562 810 markers) linear 0.186 / with the mask 0.187, cubic 0.477 / 0.591, cubic with both groups and the mask 0.821, beside
 * lsf_sample_points cubic 0.134 on the same points and one step of lsf_advect_field_band 0.534 on the same mask; at 512^3
 * (6 269 922 markers) 0.504 / 0.481, 1.566 / 2.197, 2.933, beside 0.289 and 1.579.  No speed is claimed beyond that record. */
#define LSF_ADVECT_POINTS_INFO_LEN 6
#define LSF_ADVECT_POINTS_MAX_STEPS 4096
#define LSF_POINTS_OK 0 /* status[t] */
#define LSF_POINTS_OUTSIDE 1
#define LSF_POINTS_OFFBAND 2
#define LSF_POINTS_FLAT 3
int lsf_advect_points(const double *u, const double *v, const double *w, const double *phi, const double *speed, const int32_t *mask,
                      int nx, int ny, int nz, double dx, const double xLo[3], double *pts, int npts, int order, int scheme, double dt,
                      int nsteps, int32_t *status, double *cfl, int64_t info[LSF_ADVECT_POINTS_INFO_LEN]);
int lsf_advect_points_device(const double *d_u, const double *d_v, const double *d_w, const double *d_phi, const double *d_speed,
                             const int32_t *d_mask, int nx, int ny, int nz, double dx, const double xLo[3], double *d_pts, int npts,
                             int order, int scheme, double dt, int nsteps, int32_t *d_status, double *cfl,
                             int64_t info[LSF_ADVECT_POINTS_INFO_LEN], void *stream);

/* ---- the scatter from marker particles back to the grid: the correction of the particle level set ----------
 * No reference counterpart.  Enright, Fedkiw, Ferziger and Mitchell (2002): markers with a side and a radius ride the velocity
 * (lsf_advect_points); where one ends up on the wrong side of the surface by more than its radius, the grid values around it are
 * rebuilt from its sphere.  rad[t] carries the side in its sign (> 0: the marker belongs where phi > 0) and the radius in
 * r = fabs(rad); s = rad > 0 ? 1. : -1.  phi is in and out; mask, status, change and info may be NULL.  xLo, change and info are
 * host memory on both seams.
 *   arrays   pts is REAL a(npts,3) in Fortran order; rad and status have npts entries; phi and mask are fields.
 *   exact    as above: tests/points_ref.py is the yardstick bit for bit.  One arithmetic, no mode word.
 *   particle in this precedence: rad not finite or == 0: LSF_CORRECT_BADRADIUS.  Not INSIDE by locate of lsf_sample_points:
 *            OUTSIDE.  With a mask, any of the 8 corners of its cell not IN (the LIST rule: interior and mask == 1): OFFBAND.
 *            Otherwise val is the LINEAR value of phi at the point, read from the field as it was on entry (0*NaN and 0*inf are
 *            NaN, so val is non-finite whenever a corner is); a non-finite val: NONFINITE.  ESCAPED iff s*val < -(slack*r)
 *            (slack = 1 is Enright's rule, slack = 0 any marker on the wrong side).  Otherwise INPLACE.
 *   scatter  per ESCAPED particle at each corner i0 + o of its cell: xc_A = xLo[A] + (double)(i0_A + o_A)*dx; e_A = xc_A - x_A;
 *            d = sqrt((e0*e0 + e1*e1) + e2*e2); cand = s*(r - d); for s > 0 plus = max(plus, cand), otherwise
 *            minus = min(minus, cand).  plus and minus both start as phi.  max and min are taken in the total order of the bit
 *            patterns, in which -0.0 < +0.0: the result is a function of the SET of particles, not of their order.
 *   merge    at every point (every list point under a mask): phi = fabs(plus) <= fabs(minus) ? plus : minus.  A point no
 *            candidate reached keeps its bits.  Without a mask wall points are corrected like any other.
 *   change   the largest fabs(new - old) over the points whose bits changed, 0.0 if none; a maximum of bit patterns.
 *   info     [0] INPLACE; [1] ESCAPED; [2] OUTSIDE; [3] OFFBAND; [4] NONFINITE; [5] BADRADIUS -- they add up to npts; [6] points
 *            whose bits changed.  Written on LSF_OK only.
 *   errors   LSF_ERR_INVALID, all detected before anything is written: a NULL phi, pts, rad or xLo; npts < 1; nx, ny or nz < 1 or
 *            more than 2^31 - 1 points; dx or xLo not finite, dx <= 0; slack not finite or < 0; status sharing a byte with
 *            anything; phi sharing a byte with pts, rad or the mask.  No device: LSF_ERR_NO_DEVICE with nothing written.
 *   seams    phi is in and out through its twin, as lsf_reinit_band takes its field, and comes home on LSF_OK only; the mask as
 *            lsf_curvature_band takes it; pts and rad are staged per call.  lsf_correct_field_device returns after the stream is
 *            synchronised.
 * Work: three launches (keys over the list or the grid, one lane per particle with at most 8 integer atomics each, the merge).
 * Workspace: two fields of 64-bit keys, the list under a mask, 48 bytes per 256 particles; the host seam adds 36 bytes per
 * particle.  Out of scope: reseeding and deletion on the device, attraction of new markers to a target level, the radius refresh
 * (rad = s*clip(s*val, rmin, rmax) from lsf_sample_points is the caller's one line), iso != 0, fp32, multi-GPU (DESIGN.md
 * section 8).
 * The statement on LeVeque's vortex at 33^3 points (64 steps out, 64 back, no reinitialisation): the volume
 * falls from 0.013833 to 0.010747 (-22.3 %) without markers and to 0.012081 (-12.7 %) with 21 347 of them, the mean |phi - phi0|
 * near the surface is 0.336 against 0.191 dx; 2 385 escapes were used.
 * Timed once on the same markers as lsf_advect_points, phi shifted by 0.3 dx so that 1.2 % of them escape (profiles/points_time.txt;
 * ms per call): at 256^3 0.411 without a mask and 0.265 with it, at 512^3 1.956 and 0.656.  No speed is claimed beyond that record. */
#define LSF_CORRECT_INFO_LEN 7
#define LSF_CORRECT_INPLACE 0 /* status[t] */
#define LSF_CORRECT_ESCAPED 1
#define LSF_CORRECT_OUTSIDE 2
#define LSF_CORRECT_OFFBAND 3
#define LSF_CORRECT_NONFINITE 4
#define LSF_CORRECT_BADRADIUS 5
int lsf_correct_field(double *phi, const int32_t *mask, int nx, int ny, int nz, double dx, const double xLo[3], const double *pts,
                      const double *rad, int npts, double slack, int32_t *status, double *change, int64_t info[LSF_CORRECT_INFO_LEN]);
int lsf_correct_field_device(double *d_phi, const int32_t *d_mask, int nx, int ny, int nz, double dx, const double xLo[3],
                             const double *d_pts, const double *d_rad, int npts, double slack, int32_t *d_status, double *change,
                             int64_t info[LSF_CORRECT_INFO_LEN], void *stream);

/* ---- the maintenance of the marker population: keep, drop, re-radius and top up, on the device ----------
 * No reference counterpart.  The reseeding step of the particle level set (Enright et al. 2002) as one call: the old markers are
 * classified against phi as it is now, the kept ones get their radius refreshed and are counted per cell, every under-populated
 * cell next to the surface is topped up to per_cell with new markers attracted to a random target level, and one compacted set
 * comes back.  With npts == 0 it seeds from scratch.  The call pattern is "reseed and keep, then copy out", exactly as
 * lsf_extract_surface / lsf_extract_get: the call returns nout, the caller allocates, lsf_reseed_get fills the arrays and
 * releases the kept result; every call first releases an un-fetched result, a failing call keeps nothing, a get without a result
 * is LSF_ERR_INVALID, lsf_release_workspace drops the result.  phi, mask, pts and rad are inputs only; mask, status and info may
 * be NULL, src_out may be NULL in the get; xLo, nout and info are host memory on both seams.  With npts == 0 pts, rad and status
 * are ignored and may be NULL.
 *   arrays   pts, pts_out are REAL a(n,3) in Fortran order; rad has npts entries, the side in its sign and the radius in fabs, as
 *            for lsf_correct_field; status has npts entries; rad_out and src_out have nout.
 *   exact    every expression is evaluated left to right as written, without contraction, with IEEE / and sqrt:
 *            tests/reseed_ref.py is the yardstick bit for bit.  One arithmetic, no mode word.
 *   old      per old marker, in the precedence of lsf_correct_field: rad not finite or == 0: LSF_RESEED_BADRADIUS.  Not INSIDE by
 *            the locate of lsf_sample_points: OUTSIDE.  Under a mask, a corner of its cell not IN: OFFBAND.  val, the LINEAR value
 *            there, not finite: NONFINITE.  fabs(val) > band*dx: FAR.  Otherwise KEPT: s = rad < 0 ? -1. : 1.;
 *            rad' = s*fmin(fmax(s*val, rmin*dx), rmax*dx) (an escaped marker gets the smallest radius, as in Enright); its
 *            position is returned bit for bit; it adds 1 to count[c] of its cell c, the i0 of locate (an integer sum).
 *   cells    a cell is ELIGIBLE where all 8 corners have fabs(phi) < band*dx and, under a mask, are IN (the rule of seedParticles
 *            of the Python package); need[c] = max(per_cell - count[c], 0) there, 0 elsewhere.
 *   draws    candidate (c, j), 0 <= j < need[c]; p = i + (nx+1)*(j_c + (ny+1)*k) the index of the cell's lower corner, 64 bits.
 *            For d = 0..3, all mod 2^64: ctr = (p*4096 + j)*4 + d; z = seed + 0x9E3779B97F4A7C15*(ctr + 1);
 *            z = (z ^ (z >> 30))*0xBF58476D1CE4E5B9; z = (z ^ (z >> 27))*0x94D049BB133111EB; z = z ^ (z >> 31);
 *            u_d = (double)(z >> 11)*2^-53 (the splitmix64 finaliser).  x_A = xLo[A] + ((double)c_A + u_A)*dx.
 *   attract  v0 is the sample at x in the caller's order by the rules of lsf_sample_points (joint cubic rule, linear fallback, band
 *            rule); not OK or not finite: rejected.  s = v0 < 0 ? -1. : 1.; goal = s*((rmin + (band - rmin)*u_3)*dx).  Then the
 *            foot iteration of lsf_sample_points, word for word, with iso replaced by goal, the caller's iters and tol, y starting
 *            at x; any end status but OK rejects.  vl is the LINEAR value at the final y (lsf_correct_field classifies with it);
 *            accepted iff that sample is OK, fabs(vl) >= rmin*dx, fabs(vl) <= band*dx and (vl < 0 ? -1. : 1.) == s;
 *            rad = s*fmin(fmax(fabs(vl), rmin*dx), rmax*dx).
 *   output   the KEPT markers in the caller's order with src = their 1-based input position, then the accepted candidates in
 *            ascending (p, j) with src = 0; nout is the total.  The candidates depend on the input markers only through the
 *            integer counts: the new markers are a function of the SET of input markers, never of their order.  A caller varies
 *            seed from reseed to reseed: the same seed redraws the same offsets in a cell.
 *   info     [0..5] the six status counts (they add up to npts); [6] eligible cells; [7] candidates; [8] accepted; [9] rejected
 *            before or during the attraction; [10] rejected by the final range/side test ([8]+[9]+[10] == [7]); [11] cells with
 *            count > per_cell; [12] the largest count; [13] kept markers with s*val < 0.  nout == [0] + [8].  status, nout and
 *            info are written on LSF_OK only.
 *   errors   LSF_ERR_INVALID, all detected before anything is kept or written: a NULL phi, xLo or nout; npts < 0, or npts > 0 with
 *            a NULL pts or rad; a dimension < 1 or more than 2^31 - 1 points; dx or xLo not finite, dx <= 0; per_cell outside
 *            1..LSF_RESEED_MAX_PER_CELL; rmin, rmax or band not finite, or not 0 < rmin <= rmax, or not rmin < band; an unknown
 *            order; iters outside 1..LSF_RESEED_MAX_ITERS; tol not finite or < 0; npts + candidates > 2^31 - 1 (found after the
 *            count, the number in lsf_last_error()); status sharing a byte with an input.  No device: LSF_ERR_NO_DEVICE with
 *            nothing written.
 *   seams    phi goes through its twin as lsf_sample_points takes it, the mask as lsf_curvature_band takes it; pts and rad are
 *            staged per call, as lsf_correct_field does.  lsf_reseed_points_device returns after the stream is synchronised (the
 *            host reads totals).
 * Work: a launch per old marker, one per cell of the grid (of the list under a mask), three one-block scans, one lane per candidate,
 * two emits; two or three synchronisations.  Workspace: 4 bytes per grid point and per cell looked at, 16 per old marker, 36 per
 * candidate; the kept result has 36 bytes per marker.  Out of scope: thinning of over-full cells (info[11], info[12] report them;
 * which markers to drop is a policy that needs a per-cell order), iso != 0, per-side quotas, sorting by brick, fp32, multi-GPU
 * (DESIGN.md section 8). */
#define LSF_RESEED_INFO_LEN 14
#define LSF_RESEED_MAX_PER_CELL 4096
#define LSF_RESEED_MAX_ITERS 64
#define LSF_RESEED_KEPT 0 /* status[t] of INPUT marker t */
#define LSF_RESEED_OUTSIDE 1
#define LSF_RESEED_OFFBAND 2
#define LSF_RESEED_NONFINITE 3
#define LSF_RESEED_BADRADIUS 4
#define LSF_RESEED_FAR 5
int lsf_reseed_points(const double *phi, const int32_t *mask, int nx, int ny, int nz, double dx, const double xLo[3], const double *pts,
                      const double *rad, int npts, int per_cell, double rmin, double rmax, double band, int order, int iters, double tol,
                      uint64_t seed, int32_t *status, int *nout, int64_t info[LSF_RESEED_INFO_LEN]);
int lsf_reseed_points_device(const double *d_phi, const int32_t *d_mask, int nx, int ny, int nz, double dx, const double xLo[3],
                             const double *d_pts, const double *d_rad, int npts, int per_cell, double rmin, double rmax, double band,
                             int order, int iters, double tol, uint64_t seed, int32_t *d_status, int *nout,
                             int64_t info[LSF_RESEED_INFO_LEN], void *stream);
int lsf_reseed_get(double *pts_out, double *rad_out, int32_t *src_out);
int lsf_reseed_get_device(double *d_pts_out, double *d_rad_out, int32_t *d_src_out, void *stream);

/* ---- connected components of the level set on the cells of a caller's mask ----------
 * No reference counterpart.  How many bodies there are, which cell belongs to which, and whether two have merged or one has pinched
 * off: the 6-connected components of the list cells on either side of phi = iso, a pure graph problem on the cell list every band
 * call builds, with an exact integer answer that no order of execution reaches.  comp, ncomp and info may be NULL; phi and mask
 * are inputs only.  comp, ncomp and info are host arrays on both seams.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  Any other mask value means
 *            "not in the list"; a 1 on a wall point is ignored.  The mask is read and never written.  Fewer than 2^31 points; a
 *            grid whose brick keys do not fit 32 bits keeps the list in memory order.
 *   CLASS    d = phi - iso, evaluated once per cell.  INSIDE is d < 0; OUTSIDE is everything else that is finite, d == 0 and -0.0
 *            included.  A list cell with a non-finite d gives LSF_ERR_INVALID with the number of such cells in lsf_last_error(),
 *            before anything is written.  phi off the list may hold anything, NaN included: it is read at list cells only.
 *   side     LSF_LABEL_INSIDE labels the INSIDE cells only, LSF_LABEL_OUTSIDE the OUTSIDE cells only, LSF_LABEL_BOTH both classes;
 *            a component never holds cells of both.
 *   COMPONENT  two labelled list cells are LINKED when they are face neighbours (+-1 on one axis), both list cells, and of the same
 *            class.  The components are the classes of the transitive closure.  18- and 26-connectivity are out of scope.
 *   label    int32, phi's layout.  Written AT LIST CELLS and nowhere else: every other point keeps its bits, as kappa of
 *            lsf_curvature_band does.  A labelled cell receives the 0-based point index i + (nx+1)*(j + (ny+1)*k) of the smallest
 *            point index in its component; a list cell of a class that `side` leaves out receives -1.  label must not share a byte
 *            with phi or mask.
 *   comp     ncomp receives the number of components, always, even beyond comp_cap.  comp may be NULL with comp_cap == 0;
 *            otherwise it receives min(ncomp, comp_cap) rows of LSF_LABEL_COMP_LEN int64 values, in ascending order of root index:
 *              [0] root index   [1] cells   [2] -1 for INSIDE, +1 for OUTSIDE
 *              [3..8] imin, imax, jmin, jmax, kmin, kmax over the component's cells (0-based point coordinates)
 *              [9] EDGE cells: the component's cells with at least one of the six face neighbours not a list cell -- an interior
 *                  point off the list or a wall point.
 *            [9] == 0: the component is closed inside the list.  Anything else: it may continue beyond the list, and two
 *            components reported here may be one in truth.  Rows beyond min(ncomp, comp_cap) are not written.
 *   info     [0] list cells; [1] labelled cells; [2] INSIDE components; [3] OUTSIDE components; [4] passes run; [5] links still
 *            found by the last pass -- 0 means the labels are CERTIFIED final; [6] list cells left at -1; [7] 0, reserved.  info and
 *            ncomp are written on LSF_OK only.
 *   max_passes  >= 1.  When the passes run out with info[5] > 0 the call still returns LSF_OK, and the labels are a REFINEMENT of
 *            the truth: every label is the index of a cell of the same true component, and cells with one label are truly
 *            connected.  ncomp, comp, info[2] and info[3] then count that refinement: a caller must look at info[5].
 *   empty    LIST empty: LSF_OK, nothing written, info all 0, ncomp = 0.
 *   errors   LSF_ERR_INVALID, all detected before anything is written: a NULL phi, mask or label; comp == NULL with comp_cap > 0;
 *            comp_cap < 0; an unknown side; a non-finite iso; max_passes < 1; the dimensions lsf_reinit_band refuses (nx, ny or
 *            nz < 2, a k-plane above 2 GB, more than 2^31 - 1 points); label overlapping phi or mask; a non-finite d at a list
 *            cell.  No device: LSF_ERR_NO_DEVICE -- there is no CPU fallback.  LSF_ERR_HIP with a message if a chase of the forest
 *            meets a word that cannot be one (label written by someone else during the call).
 *   result   once certified, label, ncomp, the comp rows and info[0..3], info[5] and info[6] are a function of phi, mask, iso and
 *            side alone: they equal the serial statement tests/label_ref.py with ==, on both seams, on any stream, from run to
 *            run.  info[4], the passes, is reported and not part of that equality.
 *   seams    lsf_label_band takes phi, an input only, through its twin under lsf_mirror as lsf_curvature_band takes it, and the
 *            mask as lsf_reinit_band takes its mask.  label has NO twin: it is staged like kappa, in an int32 slot of its own,
 *            copied in on every call and copied back on LSF_OK only.  lsf_label_band_device returns after the stream is
 *            synchronised.
 * Guidance: compact ids 0 .. ncomp-1 are a binary search of a label in the root column comp[.][0] (ncomp <= comp_cap).  Merging
 * and pinching show as a change of info[2] between two calls on the in/out mask of lsf_evolve_band; per-component area and volume
 * are label combined with cell_area of lsf_measure_band.
 * Work: the list build of lsf_reinit_band; a check and an init launch; per pass a link launch (3 gathered neighbours, two chases
 * of the forest per same-class neighbour, one 32-bit atomicMin per edge between two trees) and a flatten launch, CHECK_EVERY passes
 * enqueued at a time; for the table a count, a collect, a sort of the roots and one launch with 64-bit integer atomics, one set per
 * wave and component.  The forest lives in label itself; workspace beyond the list: 2 ncomp ints, the sort's temporary storage
 * and comp_cap rows; the host seam adds one int32 field.  Out of scope: 18- and 26-connectivity, compact ids written by the call,
 * per-component area / volume, a per-step trace inside lsf_evolve_band, fp32, multi-GPU.
 * Timed once on one MI355X beside lsf_curvature_band (kappa only) on the same sphere and mask |phi| < 8.1 dx
 * (profiles/label_band_time.txt, from profiles/micro/label_band_time.py; device seam, side = both, ms per call, list build
 * included): 1.08 against 0.245 at 256^3 (0.68 without the table; 2 passes) and 3.84 against 0.511 at 512^3 (2.31; 3 passes); on
 * min of two sphere distances with every interior point of 256^3 listed 23.6 (5.70 without the table; 3 passes) -- the table's
 * atomics of a 16 M-cell component all meet on one row.  No test case and no timed field needed more than 3 passes.  No speed is
 * claimed beyond that record. */
#define LSF_LABEL_INSIDE 0 /* side */
#define LSF_LABEL_OUTSIDE 1
#define LSF_LABEL_BOTH 2
#define LSF_LABEL_COMP_LEN 10
#define LSF_LABEL_INFO_LEN 8
int lsf_label_band(const double *phi, const int32_t *mask, int32_t *label, int nx, int ny, int nz, double iso, int side,
                   int max_passes, int64_t *comp, int comp_cap, int64_t *ncomp, int64_t info[LSF_LABEL_INFO_LEN]);
int lsf_label_band_device(const double *d_phi, const int32_t *d_mask, int32_t *d_label, int nx, int ny, int nz, double iso, int side,
                          int max_passes, int64_t *comp, int comp_cap, int64_t *ncomp, int64_t info[LSF_LABEL_INFO_LEN],
                          void *stream);

/* ---- post-smoothing gradients + surface-node advection (the step after the hot path) ----------
 * Replaces set3d.f90:470-501: firstDeriv order 8 (subs.f90:309-347, with its
 * quirks) on the cells of phiSB, then every surface node is moved by x += phiSurf * gradPhiSurf with
 * setPhiSurf's trilinear interpolation (subs.f90:1056-1170) until phiSurf <= 1e-13 or `iters` (host: 1000)
 * passes.  surfXX is the host's REAL surfXX(nSurfNode,3) (Fortran-ordered HOST array), in = the nodes,
 * out = the advected nodes.  Bit-identical to the reference.
 *   phiSB    a cell is band where phiSB == 1 exactly; any other value (0, 7, -1) is not.  The gradient is 0 outside the band.
 *            firstDeriv's neighbours are addressed linearly, so a band cell fewer than 4 points from a wall reads the neighbouring
 *            row / plane; a read before the first or after the last element of phi yields 0.
 *   nodes    accepted where, on every axis, xLo <= x < xLo + dx*(n-1) with n = nx, ny, nz: the cells 0 .. n-2, whose eight corners
 *            exist and stay in the field when the quotient (x-xLo)/dx rounds up by one cell.  The upper bound itself, anything
 *            below xLo, NaN and +-inf are refused.  Only the positions on entry are checked: a node that phi carries out of that
 *            range is not reported, and its reads are clamped into the field.
 *   iters    >= 0; 0 returns the nodes as they came.  One call with iters = k equals k calls with iters = 1 whose nodes are in the
 *            accepted range on every entry.
 *   phiSurf  a node moves while phiSurf > 1e-13: a NaN phiSurf (a NaN corner) or a negative one leaves the node bit for bit as it is.
 * phi and phiSB are inputs only.  LSF_ERR_INVALID with a message, surfXX untouched: a NULL pointer, nSurfNode < 1, iters < 0, a node
 * outside the accepted range. */
int lsf_advect_nodes(const double *phi, const int32_t *phiSB, int nx, int ny, int nz, double dx,
                     const double xLo[3], double *surfXX, int nSurfNode, int iters);
int lsf_advect_nodes_device(const double *d_phi, const int32_t *d_phiSB, int nx, int ny, int nz, double dx,
                            const double xLo[3], double *surfXX, int nSurfNode, int iters, void *stream);

/* ---- device-resident chain behind the host seams -----------------
 * The reference's main program hands the same arrays from seam to seam (set3d.f90:196-582: inside/outside search ->
 * reinit #1 -> narrowBand -> min/max flow -> node advection -> reinit #2) and never changes them in between.  The
 * host-pointer entry points above keep the device copies of phi / phiNB / phiSB they worked on ("twins", tagged with the
 * host address and size).  lsf_mirror() lets a host that knows its own data flow use them:
 *   LSF_MIRROR_TRUST  a seam call whose host pointer and size match a current twin skips the host-to-device copy
 *                     (promise: the host has not written the array since the last seam call);
 *   LSF_MIRROR_LAZY   seam calls do not copy results back (promise: the host does not READ phi / phiNB / phiSB until it
 *                     has called lsf_mirror_sync on them); implies LSF_MIRROR_TRUST.
 * With both set the whole chain crosses PCIe once per array at most.  Default 0: every call copies in and out.
 * What the reference host does with phi between the seams has twins too:
 *   lsf_snapshot     phiO = phi                                   (set3d.f90:311)
 *   lsf_sumsq_diff   sum((phi - phiO)^2) over all points          (set3d.f90:505-516, the "Asymptotic Error")
 *   lsf_write_vti    the VTK ImageData writers                    (set3d.f90:319-351, :538-569)
 * Each works on the twins when they are current and on the host arrays otherwise.  */
#define LSF_MIRROR_TRUST 1
#define LSF_MIRROR_LAZY 2
int lsf_mirror(int flags);
/* copies the twin of `host` (phi, phiNB or phiSB of an earlier seam call) back if the host copy is stale */
int lsf_mirror_sync(void *host);
/* Drops the twin of `host` without copying anything.  A twin keeps the HOST ADDRESS of its array: under LSF_MIRROR_LAZY
 * an un-synced result is written through that address by lsf_release_workspace, by lsf_mirror() when LAZY is switched
 * off and by a later seam call that needs the slot for another array -- so an array with a twin must be synced
 * (lsf_mirror_sync) or forgotten (lsf_mirror_forget) BEFORE it is freed, and a new array that happens to get the same
 * address must not be taken for the old one (forget, or keep LSF_MIRROR_TRUST off).  Nothing of a FAILED seam call is ever
 * copied to the host.  What becomes of the twins it touched depends on how far the call came:
 *   - a call refused before it wrote anything keeps them as they were, an un-synced earlier result included, which a later
 *     lsf_mirror_sync still brings home: every LSF_ERR_INVALID of lsf_advect_field, lsf_advect_field_band, lsf_evolve_band,
 *     lsf_evolve_band_curv, lsf_curvature_band, lsf_measure_band, lsf_cut_cells_band, lsf_sample_points, lsf_extend_field, lsf_extend_field_band and lsf_extract_surface (argument checks and the checks of
 *     u, v, w, speed, q and the list alike: all are made before phi or the mask is written), and the argument checks of
 *     every other call, which come before the twins are looked at;
 *   - any other failure -- LSF_ERR_HIP anywhere, and an error that lsf_reinit, lsf_minmax, lsf_reinit_band or
 *     lsf_distance_fill find after their arrays were staged (iter < 0, say) -- drops the twins of the in/out arrays: an
 *     un-synced earlier result in those slots is lost with it (the error is the caller's signal).
 * LSF_ERR_NAN is a result, not a failure: the arrays come home (or stay on the device under LSF_MIRROR_LAZY) as on LSF_OK. */
int lsf_mirror_forget(const void *host);
int lsf_snapshot(const double *phi, double *phiO, int nx, int ny, int nz);
int lsf_sumsq_diff(const double *phi, const double *phiO, int nx, int ny, int nz, double *sum);
/* Writes `phi` as VTK ImageData (raw appended Float64, i fastest) with the reference's header text.  The reference
 * writes an INTEGER*4 byte count that is 3 x too large and overflows at >= 448^3 points (set3d.f90:330); this writer
 * stores the true count, as UInt32 when it fits and with header_type="UInt64" otherwise (or whenever the environment
 * holds LSF_VTI_WIDE=1).  The payload streams from the
 * device twin through two pinned staging buffers (copy of chunk n + 1 overlaps the write of chunk n). */
int lsf_write_vti(const char *path, const double *phi, int nx, int ny, int nz, double dx, const double xLo[3]);

/* ---- block-decomposed building blocks (multi-GPU Jacobi; one process per GPU) -------------
 * A rank holds a box of the global field: local extents (lx,ly,lz), whose element (0,0,0) is the
 * global point (gx0,gy0,gz0); global extents are (nx+1,ny+1,nz+1).  The box includes ghost layers
 * (3 points towards each neighbouring rank) and the physical wall points it owns.  All calls are
 * asynchronous on `stream`.  The sweep and BC calls keep their partial sums in a per-stream buffer that grows on demand
 * (an allocation, and inside a lsf_sumsq bracket a flush of what has been summed so far); lsf_box_reserve sizes it up
 * front, after which the calls neither allocate nor synchronise.
 */
int lsf_box_reserve(void *stream, size_t max_partials);
typedef struct lsf_box {
    int lx, ly, lz;    /* local allocation extents (points)                          */
    int gx0, gy0, gz0; /* global index of local point (0,0,0)                        */
    int nx, ny, nz;    /* global: field is (0:nx,0:ny,0:nz)                          */
} lsf_box;

/* One Jacobi update (subs.f90:747-750 per cell, all reads from d_in) of the local cells
 * [lo[0],hi[0]) x [lo[1],hi[1]) x [lo[2],hi[2]) (local indices; must be interior cells of the
 * global grid, 1..n-1).  Adds sum((out-in)^2) over those cells to *d_sumsq (a device double;
 * contributions are combined in a fixed order, so results are reproducible).  */
int lsf_jacobi_sweep_box(const double *d_in, double *d_out, const double *d_phiS, const lsf_box *box,
                         const int lo[3], const int hi[3], double dx, double h, int mode,
                         double *d_sumsq, void *stream);

/* Extrapolation boundary condition (subs.f90:859-897, closed form) on the wall points of the
 * global grid that lie inside the local index range [lo,hi); reads interior values from d_out,
 * writes the wall points of d_out, adds sum((out-in)^2) over those wall points to *d_sumsq. */
int lsf_bc_box(const double *d_in, double *d_out, const lsf_box *box, const int lo[3], const int hi[3],
               double dx, double *d_sumsq, void *stream);

/* Optional bracket around the box calls of one sweep on one stream: between lsf_sumsq_begin and lsf_sumsq_end the
 * calls above keep their partial sums and lsf_sumsq_end adds them to *d_sumsq in ONE fixed-order reduction (one
 * launch instead of one per call; all bracketed calls must name the same d_sumsq, a call naming another one is reduced
 * at once).  The value of *d_sumsq is complete after lsf_sumsq_end. */
int lsf_sumsq_begin(void *stream);
int lsf_sumsq_end(void *stream);

/* Pack / unpack the local sub-box [lo,hi) to / from a contiguous buffer (i fastest). */
/* Up to six sub-boxes in ONE launch (the face slabs of a block: a decomposed sweep packs and unpacks three to six of them, and
 * below ~200^3 points per block each of those launches is shorter than the gap between two launches).  lo / hi: nreg rows of
 * three; d_bufs[q]: the buffer of sub-box q.  Same element order as lsf_pack_box; empty sub-boxes are skipped. */
int lsf_pack_boxes(const double *d_field, const lsf_box *box, int nreg, const int (*lo)[3], const int (*hi)[3],
                   double *const *d_bufs, void *stream);
int lsf_unpack_boxes(double *d_field, const lsf_box *box, int nreg, const int (*lo)[3], const int (*hi)[3],
                     double *const *d_bufs, void *stream);
int lsf_pack_boxes_f32(const float *d_field, const lsf_box *box, int nreg, const int (*lo)[3], const int (*hi)[3],
                       float *const *d_bufs, void *stream);
int lsf_unpack_boxes_f32(float *d_field, const lsf_box *box, int nreg, const int (*lo)[3], const int (*hi)[3],
                         float *const *d_bufs, void *stream);
int lsf_pack_box(const double *d_field, const lsf_box *box, const int lo[3], const int hi[3],
                 double *d_buf, void *stream);
int lsf_unpack_box(double *d_field, const lsf_box *box, const int lo[3], const int hi[3],
                   const double *d_buf, void *stream);

/* ---- the surface format in front of the path: binary STL -----------------------------
 * stlRead (subs.f90:17-121) reads the triangles and merges repeated vertices with a linear search per vertex:
 * O(triangles x nodes), minutes for a million triangles.  lsf_stl_read does the same job with a hash and returns EXACTLY
 * the reference's node numbering and connectivity: a vertex is merged with the FIRST earlier node whose three REAL*4
 * coordinates differ by less than 1e-13 each (subs.f90:73-75), nodes created by the triangle being read are not yet
 * searchable (the search bound nSurfNode is updated once per triangle, subs.f90:91; it starts at 3), numbering follows
 * first occurrence.  Host-only (no device needed).
 *   lsf_stl_read   parses `path`, keeps the result for the calling thread, returns the counts
 *   lsf_stl_get    copies it out -- surfX(nSurfNode,3) REAL(8), surfElem(nSurfElem,3) INTEGER*4 1-based, both in
 *                  Fortran order -- and releases it */
int lsf_stl_read(const char *path, int *nSurfElem, int *nSurfNode);
int lsf_stl_get(double *surfX, int32_t *surfElem);

/* ---- one process, every GPU of the node (replaces the call site set3d.f90:308 for a host that wants them all) --------
 * lsf_reinit_multi has lsf_reinit's arguments plus a device list.  The field is split into dims[0] x dims[1] x dims[2]
 * blocks (dims NULL: 1x1x2, 1x2x2, 2x2x2 for 2, 4, 8 devices -- BASELINE configurations 4 and 5; x, the unit-stride
 * axis, is cut last -- otherwise the prime factors dealt to z, y, x in turn), one block per entry of `devices`; the
 * library runs the Jacobi sweep (LSF_ORDER_JACOBI; for LSF_ORDER_GS see below) with 3-cell face halos copied peer to peer
 * over xGMI on a communication stream per device while the interior cells are updated on the compute stream, and one
 * host thread per device that only enqueues; the RMS of sweep s is judged while sweep s + 1 runs.  The result is bit-
 * identical to lsf_reinit with the same mode on one device.  `devices` may name a device more than once (several blocks
 * share it): that is how the path is tested on a one-GPU machine.  `phi` is a HOST array; a device twin of it left by
 * an earlier seam call (lsf_mirror) is brought home first and dropped afterwards.  The lsf_multi_* calls are the same
 * thing in pieces, for callers that keep the blocks resident (bench.py).
 * The RMS is judged a window of sweeps late; a run that can stop (tol > 0) keeps the field at the start of the last two
 * windows (two more field copies per block) and goes back to the stop sweep, a NaN sweep included.  With tol <= 0 nothing is
 * kept: when such a run returns LSF_ERR_NAN the sweep count and the trace are exact, the FIELD is that of the last sweep
 * enqueued (up to two windows later) -- undefined for the caller, as after the reference's STOP (subs.f90:926).
 *
 * LSF_ORDER_GS (fp64; dims NULL or {1, 1, ndev}): the reference's in-place ordering (subs.f90:743-852) itself, over ndev
 * slabs of tile layers in z, devices[0] at k = 0.  Every slab runs the dataflow launch of lsf_reinit on its own tile columns
 * of the SAME tile graph; the three planes next to a cut, a flag per tile next to it, a hyperplane counter per sweep and the
 * sweep's stop verdict are stored by the producing kernel straight into the neighbour's memory (peer stores over xGMI,
 * system scope, drained before the flag that announces them).  Field, sweep count and RMS trace are those of lsf_reinit
 * with the same mode, bit for bit -- with LSF_ARITH_STRICT the reference's.  Field memory per device is its slab plus three
 * planes per cut.  Needs peer access between the devices; slabs that share a device (the one-GPU rehearsal) need
 * their launches resident together: at most three per device unless GPU_MAX_HW_QUEUES is raised.  A tile that waits longer
 * than 4 s for a predecessor ends the call with LSF_ERR_HIP on every slab (bounded spins, no hang).  lsf_slabs_info: the
 * last such call of this thread -- slabs, resident blocks per slab, whether the shared buffers were fine-grained
 * allocations (LSF_SLAB_FINEGRAINED = 0 / 1 overrides: on when the devices differ), sweeps, and the time the longest of the
 * slabs' launches took (device events; uploads, transpositions and downloads excluded). */
typedef struct lsf_multi lsf_multi;
int lsf_slabs_info(int *slabs, int *blocks_per_slab, int *finegrained, int *sweeps, double *kernel_s);
/* First-contact self-test of what those slab launches assume of memory shared between two devices (nothing in the reference
 * corresponds: it is serial, README.md:17): two kernels, one per device, that wait for each other -- 200 rounds of a
 * message-passing litmus in both directions at once (8 KB stored into the peer's memory at system scope, s_waitcnt vmcnt(0),
 * a flag; the peer polls the flag and checks every word) and an atomic-max contest on one word.  Returns LSF_OK, or
 * LSF_ERR_HIP with *violated = the assumption of DESIGN.md section 6.1 that failed: 1 / 2 a payload announced by its flag
 * was not there (the drain does not cover stores to the peer, or the peer's loads were stale), 3 the atomic lost an update,
 * 4 the kernels did not run at the same time (bounded spins: no hang).  devA == devB runs both kernels on one device.
 * lsf_reinit_multi(LSF_ORDER_GS) runs it once per process for every pair of distinct neighbouring devices. */
int lsf_peer_selftest(int devA, int devB, int *violated);
int lsf_reinit_multi(double *phi, int nx, int ny, int nz, int iter, double dx, double h, double tol, int mode,
                     const int *devices, int ndev, const int dims[3], int *sweeps_done, double *rms_trace, int trace_cap);
int lsf_reinit_multi_f32(float *phi, int nx, int ny, int nz, int iter, double dx, double h, double tol, int mode,
                         const int *devices, int ndev, const int dims[3], int *sweeps_done, double *rms_trace,
                         int trace_cap);
/* f32 != 0: float fields.  Allocates two field buffers, the sign field and the halo buffers of every block. */
int lsf_multi_create(int nx, int ny, int nz, const int *devices, int ndev, const int dims[3], int f32, lsf_multi **out);
int lsf_multi_destroy(lsf_multi *m);
/* geometry of block r: global index of its local point 0, local extents (ghost layers included), owned global range */
int lsf_multi_block(const lsf_multi *m, int r, int g0[3], int ext[3], int own_lo[3], int own_hi[3], int *device);
int lsf_multi_scatter(lsf_multi *m, const void *host_phi);              /* host field -> blocks (ghosts included) */
int lsf_multi_upload_block(lsf_multi *m, int r, const void *d_block);   /* device pointer on block r's device     */
int lsf_multi_run(lsf_multi *m, int iter, double dx, double h, double tol, int mode, int *sweeps_done, double *rms_trace,
                  int trace_cap);                                       /* continues from the current block fields */
int lsf_multi_gather(lsf_multi *m, void *host_phi);                     /* owned points of every block -> host     */
/* How the blocks talk and how often the host looks at the RMS.
 *   check_every  1..64 sweeps per judging window (default 8): the host threads only enqueue inside a window and read
 *                the window's block sums one window late; a run with tol > 0 keeps the field at the start of the last
 *                two windows and, when a window holds the stop sweep, repeats the sweeps from its start to that sweep:
 *                field, sweep count and RMS trace are those of a driver that looks after every sweep (subs.f90:915).
 *   transport    LSF_TRANSPORT_PEER  one peer copy per neighbour and sweep (hipMemcpyPeerAsync, xGMI between the devices
 *                                    of a node), events + a host hand-shake of the two neighbours' threads; works with
 *                                    several blocks on one device (default)
 *                LSF_TRANSPORT_RCCL  ncclGroupStart / ncclSend + ncclRecv per neighbour / ncclGroupEnd on the block's
 *                                    communication stream, one communicator per block (ncclCommInitAll over the device
 *                                    list; librccl.so is loaded on first use); needs a distinct device per block
 *                LSF_TRANSPORT_MOCK  test aid: the RCCL schedule with a stand-in for the library (pull copies) that runs
 *                                    with several blocks on one device
 * lsf_multi_defaults sets what lsf_multi_create / lsf_reinit_multi of the calling thread start from (the environment variables
 * LSF_MULTI_CHECK_EVERY and LSF_MULTI_TRANSPORT = peer | rccl | mock override it).  lsf_multi_info: NULL for what is not
 * wanted; rccl_ranks = communicators held (0 unless the RCCL transport is on); host_enqueue_s = the longest any block's
 * thread spent enqueuing during the last lsf_multi_run (waits for its neighbours' threads and, when blocks share a device,
 * for that device's enqueue lock included), host_calls_s = the longest any thread spent inside the runtime / library calls
 * themselves, wall_s = that run's wall clock. */
#define LSF_TRANSPORT_PEER 0
#define LSF_TRANSPORT_RCCL 1
#define LSF_TRANSPORT_MOCK 2
int lsf_multi_defaults(int check_every, int transport);   /* per calling thread */
int lsf_multi_defaults_get(int *check_every, int *transport);
int lsf_multi_configure(lsf_multi *m, int check_every, int transport);
int lsf_multi_info(const lsf_multi *m, int *check_every, int *transport, int *rccl_ranks, int *rccl_version,
                   double *host_enqueue_s, double *host_calls_s, double *wall_s, int *sweeps_enqueued);

/* ---- single precision (BASELINE.json configuration 5: 1536^3 fp32 on 2x2x2 GPUs) -------------------
 * The reference is fp64 only (Makefile:4, -fdefault-real-8): there is no fp32 field to be identical to,
 * so these entry points exist for the Jacobi ordering and the FAST arithmetic only (mode must be
 * LSF_ORDER_JACOBI | LSF_ARITH_FAST, anything else is LSF_ERR_INVALID).  Same update as subs.f90:743-852 with
 * weno :489-711 and phiSign :152-172; the epsilon floor 1e-99 of subs.f90:533-534, which fp32 cannot hold,
 * becomes 1e-30 (in the unscaled units of the FAST algebra) and the three non-linear weights of a WENO side
 * are formed from q_k / (q_0+q_1+q_2) so that their products stay inside the fp32 range.  Fields are
 * `float` with the layout of the fp64 entry points; dx, h, tol and the RMS trace stay double (the RMS is
 * accumulated in double from fp32 differences, and divided by the true product nx*ny*nz: the reference's
 * INTEGER*4 product, subs.f90:914, which the fp64 entry points reproduce, is negative for the 1536^3 grid of
 * configuration 5).  Checked against the fp64 oracle on the same fp32-rounded input: max and RMS of the
 * difference over the whole array stay within 3 x the distance that the float32 statement of the same sweep
 * (tests/reinit_f32_ref.py: the oracle's operations in numpy, every constant and intermediate in float32) has
 * from that oracle; every kernel instance returns the same bits (tests/test_gpu_f32_statement.py).
 * Value range, derived from the kernels and not measured: the smoothness terms are formed unscaled, as squares of
 * second differences of phi, so the differences |dphi| between neighbouring points must stay below roughly 1e18 or
 * the terms overflow; below roughly 2e-12 the 1e-30 floor takes over from the reference's relative epsilon
 * (1e-6 * dphi^2 / 3 < 1e-30) and the weights drift towards the linear ones.  Tested with phi, dx and h scaled
 * by 1e-8 and 1e8 (the accuracy rule above is asserted) and by 1e-13 and 1e15 (|dphi| ~ 8e-15 and 8e13: a finite
 * field and RMS trace are asserted; at 1e-13 the field is measured 27 eps32 * max|phi| from the oracle after one
 * sweep and 671 after nine, at 1e15 as close as inside the range). */
int lsf_reinit_f32(float *phi, int nx, int ny, int nz, int iter, double dx, double h, double tol, int mode,
                   int *sweeps_done, double *rms_trace, int trace_cap);
int lsf_reinit_f32_device(float *d_phi, const float *d_phiS, int nx, int ny, int nz, int iter, double dx,
                          double h, double tol, int mode, int *sweeps_done, double *rms_trace, int trace_cap,
                          void *stream);
/* fp32 twins of the block-decomposed building blocks above (same contracts) */
int lsf_jacobi_sweep_box_f32(const float *d_in, float *d_out, const float *d_phiS, const lsf_box *box,
                             const int lo[3], const int hi[3], double dx, double h, int mode,
                             double *d_sumsq, void *stream);
int lsf_bc_box_f32(const float *d_in, float *d_out, const lsf_box *box, const int lo[3], const int hi[3],
                   double dx, double *d_sumsq, void *stream);
int lsf_pack_box_f32(const float *d_field, const lsf_box *box, const int lo[3], const int hi[3],
                     float *d_buf, void *stream);
int lsf_unpack_box_f32(float *d_field, const lsf_box *box, const int lo[3], const int hi[3],
                       const float *d_buf, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSF_H */
