/* lsf_redistance.h -- closest-point redistancing of a cell list: lsf_redistance_band.  A public header beside lsf.h, which it
 * includes: the return codes, lsf_last_error(), lsf_mirror and the status words LSF_SAMPLE_* are lsf.h's.  The symbols live in
 * liblsf_hip.so; LSF_VERSION is unchanged.
 *
 * ---- redistance a band from closest points -----------------------------------------------------------------------------------
 * No reference counterpart.  The pseudo-time sweeps (lsf_reinit, lsf_reinit_band, the reinit_sweeps of lsf_evolve_band) carry
 * information one cell per sweep and move the surface a little every time.  This call does neither: the distance of a cell next to
 * the surface is the length of the segment to its foot on the zero level set of the field's interpolant, and the rest of the list is
 * filled from those cells by the first-order Godunov visit of lsf_distance_fill.  phi and mask have the layout of every other entry
 * point.  phi is in/out; mask is read and never written.  passes_done, changed_trace, change and info may be NULL and are HOST memory
 * on both seams.  There is no mode word and one arithmetic: everything below is evaluated left to right as written, without
 * contraction, with the IEEE / and sqrt, as in the point calls.
 *   LIST     the rule of lsf_reinit_band: the interior points (1..n-1 on each axis) with mask == 1.  Any other mask value means "not
 *            in the list"; a 1 on a wall point is ignored.  Points outside the list are never written, and phi is never read there:
 *            the band rule admits stencils of list points only.
 *   FOOT     per list cell (i, j, k): the point x = ((double)i*dx, (double)j*dx, (double)k*dx) of the grid with xLo = (0, 0, 0) is
 *            located, sampled and projected by the rules of lsf_sample_points, word for word: order LSF_SAMPLE_CUBIC (its joint rule
 *            with the linear fallback), the call's mask as the band, iso = 0, iters, tol.  "Locate" is applied to x as to any
 *            point, and whichever cell it returns is used.  The status is that call's status[t].
 *              d_A = x_A - foot_A;   dist = sqrt((d_0*d_0 + d_1*d_1) + d_2*d_2).
 *            The cell is FROZEN when the status is LSF_SAMPLE_OK and dist < near*dx (that product is computed once on the host).
 *            s = -1 when phi(p) < 0 on entry, +1 otherwise: the sign comes from the field value, not from the sample.  A frozen
 *            cell's new value is s*dist; a frozen cell with dist == 0.0 keeps its value on entry, so no cell changes the answer of
 *            (phi < 0).  dist is the distance to a point of the interpolant's level set: never below the true distance to it.
 *   FILL     magnitudes u: dist at frozen cells, +inf at every other list cell.  JACOBI passes: every non-frozen list cell is
 *            visited with u AS IT WAS AT THE START OF THE PASS.  The visit is lsf_distance_fill's, word for word: per axis the
 *            smaller of the two neighbour magnitudes, a neighbour that is not in the LIST counting as +inf; nothing happens when all
 *            three are +inf; otherwise a, b, c, the three candidates, new = min(old, t).  A visit with new < old is counted.
 *   trace    changed_trace[p], p < trace_cap: the number of counted visits of pass p (an integer: no arrival order in it).
 *   stop     after the first pass whose count is 0 (that pass is counted) or after max_passes; passes_done = passes run.  Reaching
 *            max_passes is LSF_OK.
 *   RESULT   non-frozen list cells with a finite u take s*u.  Cells still at +inf -- a piece of the list without a frozen cell --
 *            are UNREACHED: they keep their value on entry and are counted, never guessed.  change = the largest |new - old| over
 *            the written cells, as a maximum of bit patterns (0.0 if none).
 *   info     [0] list cells  [1] frozen  [2] filled  [3] unreached  [4] feet LSF_SAMPLE_OFFBAND  [5] _OUTSIDE  [6] _FLAT
 *            [7] _NOT_CONVERGED  [8] LSF_SAMPLE_OK but dist >= near*dx.   [1]+[4]+[5]+[6]+[7]+[8] == [0] == [1]+[2]+[3].
 *            passes_done, the trace, change and info are written on LSF_OK only.
 *   result   field, passes_done, trace, change and info are those of the serial statement tests/redistance_ref.py bit for bit, on
 *            both seams, on any stream, from run to run -- after every pass, not only at the fixed point.  On a list whose frozen
 *            cells and every cell the full-grid call would draw on lie in the list and clear of the walls, the converged magnitudes
 *            at list cells equal the converged lsf_distance_fill with the frozen cells as its mask.
 *   errors   LSF_ERR_INVALID, all decided before phi is written, the offending count in lsf_last_error() where there is one: a NULL
 *            phi or mask; the dimensions lsf_reinit_band refuses (nx, ny or nz < 2, a k-plane above 2 GB, more than 2^31 - 1
 *            points); dx not finite or <= 0; near not finite or <= 0; iters < 1; tol not finite or < 0; max_passes < 1;
 *            trace_cap < 0; phi sharing a byte with mask; an empty list; list cells with a non-finite phi at themselves (count); no
 *            frozen cell.  No device: LSF_ERR_NO_DEVICE -- there is no CPU fallback.
 *   seams    lsf_redistance_band stages phi and the mask as lsf_reinit_band stages them under lsf_mirror; phi comes home on LSF_OK
 *            only (a refused call leaves the twin as it was).  lsf_redistance_band_device returns after the stream is synchronised
 *            (the host reads the counts of 8 passes at a time).
 * Guidance: `near` is the caller's parameter, 2 to 3 cells.  Far from the surface the foot of a field that is not a distance is a
 * point of the level set, not the closest one: with near = 6.5 on the strongly distorted sphere of DESIGN.md section 4.27 the
 * frozen cells are wrong by 1.3 dx at 41^3, with 2.5 by 0.07 dx.  The frozen values are as accurate as the cubic (second order
 * measured), the filled values FIRST ORDER as in lsf_distance_fill (about 0.5 dx at the edge of an 8.1-cell mask).  Passes: the width
 * of the list beyond the frozen cells in cells, times about 2.  Work: the list build of lsf_reinit_band, one foot launch (up to
 * iters + 1 gathers of 64 + 64 values per cell), two launches per pass over the list (7 gathered loads, at most two square
 * roots), one finish launch.  Workspace beyond the list's: 28 bytes per list cell.  Out of scope: iso != 0, a linear foot, a
 * higher-order fill, fp32, multi-GPU, the call inside lsf_evolve_band's rebuild, several fields.
 * Timed once on one MI355X beside lsf_reinit_band with 20 sweeps and ONE round of lsf_distance_fill on the same mildly distorted
 * two-sphere field, mask |d| < 8.1 dx, near 2.5 (profiles/redistance_band_time.txt, from profiles/micro/redistance_band_time.py;
 * device seam, ms per call to convergence, list build included): 1.22 against 0.68 and 15.4 at 256^3 (514 594 list cells, 30 passes
 * of 0.027 ms, 0.40 ms of list build, feet, seed and finish) and 3.62 against 1.84 and 39.5 at 512^3 (2 048 561 cells, 32 passes of
 * 0.083 ms, 0.97 ms fixed).  No speed is claimed beyond that record. */
#ifndef LSF_REDISTANCE_H
#define LSF_REDISTANCE_H

#include "lsf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSF_REDISTANCE_INFO_LEN 9
int lsf_redistance_band(double *phi, const int32_t *mask, int nx, int ny, int nz, double dx, double near, int iters, double tol,
                        int max_passes, int *passes_done, int64_t *changed_trace, int trace_cap, double *change,
                        int64_t info[LSF_REDISTANCE_INFO_LEN]);
int lsf_redistance_band_device(double *d_phi, const int32_t *d_mask, int nx, int ny, int nz, double dx, double near, int iters,
                               double tol, int max_passes, int *passes_done, int64_t *changed_trace, int trace_cap, double *change,
                               int64_t info[LSF_REDISTANCE_INFO_LEN], void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSF_REDISTANCE_H */
