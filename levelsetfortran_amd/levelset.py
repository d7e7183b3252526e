"""Host-side mirror of the reference's interface for the hot path.

Same names, argument meaning and error behaviour as the Fortran module procedures and the loop
they replace (citations are into /root/reference):

  reinit(phi, gradPhi, gradPhiMag, nx, ny, nz, iter, dx, h)     subs.f90:717-931
  narrowBand(nx, ny, nz, dx, phi, phiNB, phiSB)                 subs.f90:178-207
  minmaxFlow(phi, phiNB, phiSB, nx, ny, nz, iter, dx, h1)       set3d.f90:394-462 (hoisted)

and, without a reference counterpart, reinit on the cells of a mask only:

  reinitBand(phi, mask, nx, ny, nz, iter, dx, h)                include/lsf.h: lsf_reinit_band

and the exact signed distance from the triangle mesh, clamped to a tube (the reference has the centroid test of phi0Init only):

  meshDistance(phi, nx, ny, nz, dx, xLo, surfX, surfElem)       include/lsf.h: lsf_mesh_distance
  meshCheck(surfX, surfElem)                                    include/lsf.h: lsf_mesh_check (host only)

and the first-order distance on the rest of the grid from a frozen band (fast sweeping; no reference counterpart):

  distanceFill(phi, nx, ny, nz, dx, band=... | mask=...)        include/lsf.h: lsf_distance_fill

and the transport of lsf_advect_field on the cells of a mask only (no reference counterpart):

  advectFieldBand(phi, mask, nx, ny, nz, dx, dt, steps, ...)    include/lsf.h: lsf_advect_field_band
  evolveBand(phi, mask, nx, ny, nz, dx, dt, steps, ...)         include/lsf.h: lsf_evolve_band
  evolveBandCurv(phi, mask, nx, ny, nz, dx, dt, steps, curvature=b, ...)  include/lsf.h: lsf_evolve_band_curv

and the mean and Gaussian curvature of the level sets on the cells of a mask (the reference's own is commented out, subs.f90:426-448):

  curvatureBand(phi, mask, nx, ny, nz, dx, kappa, ...)          include/lsf.h: lsf_curvature_band

and the area, the enclosed volume, the centroids and the integral of a field over the surface, summed on the cells of a mask:

  measureBand(phi, mask, nx, ny, nz, dx, xLo, ...)              include/lsf.h: lsf_measure_band

and what a cut-cell solver takes from the geometry -- volume fraction, face apertures and area vector per cell of a mask:

  cutCellsBand(phi, mask, nx, ny, nz, dx, ...)                  include/lsf.h: lsf_cut_cells_band

and the field, its gradient, a second field and the foot point on the surface at arbitrary points (particles, nodes of another mesh):

  samplePoints(phi, nx, ny, nz, dx, xLo, pts, ...)              include/lsf.h: lsf_sample_points

and the first hit of a ray with the surface, marching by the field's own value and skipping what a band mask does not hold:

  castRays(phi, nx, ny, nz, dx, xLo, org, dir, ...)             include/lsf.h: lsf_cast_rays

and points carried through the fields that move phi, with the correction of the particle level set that they make possible:

  advectPoints(pts, nx, ny, nz, dx, xLo, dt, steps, ...)        include/lsf.h: lsf_advect_points
  correctField(phi, nx, ny, nz, dx, xLo, pts, rad, ...)         include/lsf.h: lsf_correct_field (markers from seedParticles)

and how many bodies there are and which cell belongs to which, the connected components on the cells of a mask:

  labelBand(phi, mask, nx, ny, nz, label, ...)                  include/lsf.h: lsf_label_band

and a quantity known on that band carried to the rest of the grid constant along the normals (no reference counterpart):

  extendField(q, phi, nx, ny, nz, dx, band=... | mask=...)      include/lsf.h: lsf_extend_field

and the distance property restored on the cells of a mask from closest points, without pseudo-time sweeps:

  redistanceBand(phi, mask, nx, ny, nz, dx, near=2.5, ...)      include/lsf_redistance.h: lsf_redistance_band

Fields are updated IN PLACE like the INTENT(INOUT) dummies of the reference.  A field is either
  * a numpy float64 array, Fortran-ordered with shape (nx+1, ny+1, nz+1) (or 1-D of that size):
    the host seam -- the library copies it to HBM and back (lsf_reinit / lsf_minmax), or
  * a torch CUDA float64 tensor, C-contiguous with shape (nz+1, ny+1, nx+1) (or 1-D): the same
    bytes already resident in HBM (lsf_*_device); nothing crosses PCIe.

All arithmetic happens in liblsf_hip.so (hand-written HIP for gfx950).  This module contains no
numerical code and no fallback.
"""
from __future__ import annotations

import ctypes
import os
import sys
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional

import numpy as np

from . import _lib, _seam
from ._lib import LSF_ARITH_FAST, LSF_ARITH_STRICT, LSF_ORDER_GS, LSF_ORDER_JACOBI, LsfError, LsfNaNError
from ._seam import Seam

__all__ = ["cutCellsBand", "CutCellsReport", "advectPoints","AdvectPointsReport", "correctField", "CorrectReport", "seedParticles", "reinit", "reinitBand", "narrowBand", "minmaxFlow", "phi0Init", "meshDistance", "meshCheck", "MeshInfo", "distanceFill", "FillReport", "extendField", "ExtendReport", "extendFieldBand", "ExtendBandReport", "redistanceBand", "RedistanceReport", "advectField", "AdvectReport", "advectFieldBand", "AdvectBandReport", "evolveBand", "EvolveBandReport", "evolveBandCurv", "EvolveBandCurvReport", "curvatureBand", "CurvatureReport", "extractSurface", "SurfaceInfo", "measureBand", "MeasureReport", "samplePoints", "SampleReport", "castRays", "CastReport", "stlWrite", "advectNodes", "SweepReport", "mode_word", "LsfError", "LsfNaNError", "peer_selftest"]

REINIT_TOL = 1.0e-5  # subs.f90:915
MINMAX_TOL = 1.0e-7  # set3d.f90:448


def mode_word(order: str = "gs", arith: str = "fast") -> int:
    """Build the `mode` argument of include/lsf.h from readable names."""
    o = {"gs": LSF_ORDER_GS, "jacobi": LSF_ORDER_JACOBI}[order]
    a = {"fast": LSF_ARITH_FAST, "strict": LSF_ARITH_STRICT}[arith]
    return o | a


@dataclass
class SweepReport:
    """What the reference prints while iterating (subs.f90:916,923 / set3d.f90:449,456)."""

    count: int  # sweeps / iterations executed
    rms: List[float] = field(default_factory=list)  # RMS change after each of them
    converged: bool = False  # last RMS < tol -> the "steady state" line

    def lines(self, first_index: int, steady_msg: str) -> List[str]:
        """The stdout lines of the reference for this run (list-directed formatting aside)."""
        out = []
        n_print = self.count - 1 if self.converged else self.count
        for s in range(n_print):
            out.append(f"  Iteration:  {s + first_index}   RMS Error:  {self.rms[s]!r}")
        if self.converged:
            out.append(steady_msg)
        return out


_SCHEMES = {"rk3": _lib.LSF_ADVECT_RK3, "euler": _lib.LSF_ADVECT_EULER}
_ARITHS = {"strict": LSF_ARITH_STRICT, "fast": LSF_ARITH_FAST}
_SAMPLE_ORDERS = {"linear": _lib.LSF_SAMPLE_LINEAR, "cubic": _lib.LSF_SAMPLE_CUBIC}
_EXTEND_KINDS = ("numpy arrays (host seam)", "torch CUDA tensors (device seam)")


def _sweep_report(rc, done, trace, tol, first_index, steady_msg, echo) -> SweepReport:
    """The report of a sweep loop, echoed like the reference if asked for, then the library's verdict"""
    n = done.value
    rep = SweepReport(n, [float(v) for v in trace[:n]], bool(n and trace[n - 1] < tol))
    if echo:
        for ln in rep.lines(first_index, steady_msg):
            print(ln)
        print()
        sys.stdout.flush()
    _lib.check(rc)
    return rep


def _check_report(rc, rep):
    """`rep` if the call succeeded; an LsfNaNError carries it as `.report` (the steps run, the NaN one included)"""
    try:
        _lib.check(rc)
    except LsfNaNError as e:
        e.report = rep
        raise
    return rep


def _transport_fields(velocity, speed):
    """The (name, field) pairs that move phi in advectField and its band forms: u, v, w of a checked velocity, then the speed"""
    if velocity is not None:
        if not isinstance(velocity, (tuple, list)) or len(velocity) != 3 or any(c is None for c in velocity):
            raise ValueError("velocity must be a 3-tuple (u, v, w) of fields")
    return [(n, f) for n, f in zip("uvw", velocity or ())] + ([("speed", speed)] if speed is not None else [])


def reinit(phi, gradPhi=None, gradPhiMag=None, nx: int = 0, ny: int = 0, nz: int = 0, iter: int = 0,
           dx: float = 0.0, h: float = 0.0, *, tol: float = REINIT_TOL, order: str = "gs", arith: str = "fast",
           first_raster: int = 0, phiS=None, echo: bool = False) -> SweepReport:
    """SUBROUTINE reinit (subs.f90:717-931) on the GPU; `phi` is updated in place.

    gradPhi / gradPhiMag are accepted for signature parity and left untouched: the reference never
    reads what reinit stores there (set3d.f90:372-375 zeroes them).
    Runs at most iter+1 sweeps (subs.f90:735).  Raises LsfNaNError where the reference STOPs.
    echo=True prints the reference's per-sweep lines.
    A float32 field (numpy or torch) selects the single-precision path of BASELINE configuration 5, which
    exists for order="jacobi", arith="fast" only (the reference is fp64; see include/lsf.h).
    """
    cap = int(iter) + 1
    trace = np.zeros(max(cap, 1), dtype=np.float64)
    done = ctypes.c_int(0)
    mode = mode_word(order, arith)
    s = Seam(phi, nx, ny, nz)
    f32 = s.is_f32(phi)  # single precision: Jacobi ordering, FAST arithmetic only (include/lsf.h)
    dtype = np.float32 if f32 else np.float64
    p = s.field(phi, "phi", dtype)
    head = (nx, ny, nz, int(iter), float(dx), float(h), float(tol), mode)
    tail = (ctypes.byref(done), trace.ctypes.data, cap)
    if s.dev:  # the device forms take phiS, and the fp64 one first_raster, besides the stream
        ps = s.optional(phiS, "phiS", dtype)
        if f32:
            if first_raster != 0:
                raise ValueError("first_raster has no meaning for the Jacobi ordering")
            rc = _lib.load().lsf_reinit_f32_device(p, ps, *head, *tail, s.stream())
        else:
            rc = _lib.load().lsf_reinit_device(p, ps, *head, int(first_raster), *tail, s.stream())
    else:
        if first_raster != 0 or phiS is not None:
            raise ValueError("first_raster / phiS are only available on the device seam")
        rc = s.call("lsf_reinit_f32" if f32 else "lsf_reinit", p, *head, *tail)
    return _sweep_report(rc, done, trace, tol, 0, "  Distance function time integration has reached steady state ", echo)


def reinitBand(phi, mask, nx: int, ny: int, nz: int, iter: int, dx: float, h: float, *, tol: float = REINIT_TOL,
               arith: str = "fast", phiS=None, echo: bool = False) -> SweepReport:
    """Reinitialisation on the cells of `mask` only (include/lsf.h: lsf_reinit_band); `phi` is updated in place.

    mask: int32, same layout as phi (e.g. phiSB of narrowBand); the interior points where it is 1 are updated with the
    Jacobi ordering of reinit, every other point -- wall points included -- keeps its value and no boundary condition is
    applied.  Runs at most iter+1 sweeps and stops after the first whose RMS over the LIST cells is < tol (not comparable
    with reinit's RMS over the whole grid).  phiS (device seam only): the sign field to use instead of phi on entry, which
    makes a call continue an earlier one.  Make the mask wider than the band whose values are trusted: cells within three
    cells of its edge read frozen neighbours.  Raises LsfNaNError on a NaN RMS.
    """
    cap = int(iter) + 1
    trace = np.zeros(max(cap, 1), dtype=np.float64)
    done = ctypes.c_int(0)
    mode = mode_word("jacobi", arith)  # a raster order has no meaning on a list
    s = Seam(phi, nx, ny, nz)
    p, m = s.field(phi, "phi"), s.field(mask, "mask", np.int32)
    args = (nx, ny, nz, int(iter), float(dx), float(h), float(tol), mode, ctypes.byref(done), trace.ctypes.data, cap)
    if s.dev:  # the device form takes phiS besides the stream
        rc = _lib.load().lsf_reinit_band_device(p, s.optional(phiS, "phiS"), m, *args, s.stream())
    else:
        if phiS is not None:
            raise ValueError("phiS is only available on the device seam")
        rc = s.call("lsf_reinit_band", p, m, *args)
    return _sweep_report(rc, done, trace, tol, 0, "  Distance function time integration has reached steady state ", echo)


def narrowBand(nx: int, ny: int, nz: int, dx: float, phi, phiNB, phiSB) -> None:
    """SUBROUTINE narrowBand (subs.f90:178-207): phiNB = |phi| < 4.1 dx, phiSB = |phi| < 8.1 dx."""
    s = Seam(phi, nx, ny, nz)
    _lib.check(s.call("lsf_narrowband", s.field(phi, "phi"), s.field(phiNB, "phiNB", np.int32), s.field(phiSB, "phiSB", np.int32),
                      nx, ny, nz, float(dx)))


def minmaxFlow(phi, phiNB, phiSB, nx: int, ny: int, nz: int, iter: int, dx: float, h1: float, *,
               tol: float = MINMAX_TOL, order: str = "gs", echo: bool = False) -> SweepReport:
    """The min/max-flow loop of the main program (set3d.f90:394-462) as one call.

    phi, phiNB, phiSB are updated in place; the masks come back as the host would hold them after
    the loop (refreshed only on the non-exit path, set3d.f90:448-460).
    """
    cap = max(int(iter), 1)
    trace = np.zeros(cap, dtype=np.float64)
    done = ctypes.c_int(0)
    mode = mode_word(order, "strict")  # min/max has a single (exact) arithmetic
    s = Seam(phi, nx, ny, nz)
    rc = s.call("lsf_minmax", s.field(phi, "phi"), s.field(phiNB, "phiNB", np.int32), s.field(phiSB, "phiSB", np.int32), nx, ny, nz,
                int(iter), float(dx), float(h1), float(tol), mode, ctypes.byref(done), trace.ctypes.data, cap)
    return _sweep_report(rc, done, trace, tol, 1, "  Min/max time integration has reached steady state ", echo)


def phi0Init(phi, nx: int, ny: int, nz: int, dx: float, xLo, minX, maxX, surfX, surfElem) -> None:
    """Inside/outside initialisation of the main program (set3d.f90:196-268) as one call.

    phi (numpy F-ordered or torch CUDA, see module docstring) receives sgn in (-1,1) within 3 cells of the
    surface bounding box and 1.0 elsewhere.  surfX: (nSurfNode,3) float64, surfElem: (nSurfElem,3) int32,
    1-based, as stlRead returns them (subs.f90:17-121); xLo/minX/maxX as the host computes them
    (set3d.f90:94-157).  Bit-identical to the reference.
    """
    sX = np.asfortranarray(surfX, dtype=np.float64)
    sE = np.asfortranarray(surfElem, dtype=np.int32)
    lo, mn, mx = (np.ascontiguousarray(v, dtype=np.float64) for v in (xLo, minX, maxX))
    s = Seam(phi, nx, ny, nz)
    _lib.check(s.call("lsf_phi0", s.field(phi, "phi"), nx, ny, nz, float(dx), lo.ctypes.data, mn.ctypes.data, mx.ctypes.data, sX.ctypes.data,
                      sX.shape[0], sE.ctypes.data, sE.shape[0]))


class MeshInfo(NamedTuple):
    """The counts of lsf_mesh_distance / lsf_mesh_check (include/lsf.h: info[0..3]); volume: lsf_mesh_check only."""
    tube_points: int
    degenerate_triangles: int
    defective_edges: int
    triangles_off_grid: int
    signed_volume: Optional[float] = None


def _surface(surfX, surfElem):
    """(surfX, surfElem) as the Fortran-ordered float64 (nSurfNode,3) / int32 (nSurfElem,3) arrays the library reads."""
    sX, sE = np.asarray(surfX), np.asarray(surfElem)
    if sX.ndim != 2 or sX.shape[1] != 3 or sX.shape[0] < 1:
        raise ValueError("surfX must have shape (nSurfNode, 3) with nSurfNode >= 1")
    if sE.ndim != 2 or sE.shape[1] != 3 or sE.shape[0] < 1:
        raise ValueError("surfElem must have shape (nSurfElem, 3) with nSurfElem >= 1")
    if sX.dtype.kind != "f" or sE.dtype.kind not in "iu":
        raise TypeError("surfX must be a float array and surfElem an integer array")
    return np.asfortranarray(sX, dtype=np.float64), np.asfortranarray(sE, dtype=np.int32)


def meshCheck(surfX, surfElem) -> MeshInfo:
    """Degenerate triangles, defective edges and the signed volume of a mesh (include/lsf.h: lsf_mesh_check).  Host code
    only: no device is needed.  A signed meshDistance wants defective_edges == 0."""
    sX, sE = _surface(surfX, surfElem)
    info = np.zeros(_lib.LSF_MESH_INFO_LEN, dtype=np.int64)
    vol = ctypes.c_double(0.0)
    _lib.check(_lib.load().lsf_mesh_check(sX.ctypes.data, sX.shape[0], sE.ctypes.data, sE.shape[0], info.ctypes.data, ctypes.byref(vol)))
    return MeshInfo(*(int(v) for v in info), vol.value)


def meshDistance(phi, nx: int, ny: int, nz: int, dx: float, xLo, surfX, surfElem, *, width: float = 4.0, signed: bool = True) -> MeshInfo:
    """Exact signed distance from the triangle mesh, clamped to a tube of `width` cells (include/lsf.h: lsf_mesh_distance).

    phi (numpy F-ordered or torch CUDA, see module docstring) is an output: points within width*dx of the surface receive
    the Euclidean distance to the nearest triangle, negative inside (angle-weighted pseudonormals), every other point
    +-width*dx with the sign carried along its k column.  surfX / surfElem as for phi0Init; the grid point is xLo + i*dx.
    signed=False: the unsigned distance, no requirement on the mesh (a signed call refuses a mesh with defective edges,
    see meshCheck).  Returns the counts of the call.  The field is clamped, not a distance everywhere: reinit takes it as
    its start and needs far fewer sweeps than from phi0Init's smeared sign.
    """
    sX, sE = _surface(surfX, surfElem)
    lo = _seam.xlo(xLo, finite=False)
    width = float(width)
    if not (np.isfinite(width) and width >= 1.5):
        raise ValueError("width must be finite and >= 1.5 (cells)")
    dx = _seam.positive(dx, "dx must be > 0")
    info = np.zeros(_lib.LSF_MESH_INFO_LEN, dtype=np.int64)
    s = Seam(phi, nx, ny, nz)
    _lib.check(s.call("lsf_mesh_distance", s.field(phi, "phi"), nx, ny, nz, dx, lo.ctypes.data, sX.ctypes.data, sX.shape[0], sE.ctypes.data,
                      sE.shape[0], width, 0 if signed else _lib.LSF_MESH_UNSIGNED, info.ctypes.data))
    return MeshInfo(*(int(v) for v in info))


class FillReport(NamedTuple):
    """What lsf_distance_fill reports (include/lsf.h): rounds of 8 sweeps run, the visits that lowered a value in each of them,
    the size of the frozen set, and whether the last round lowered nothing."""
    rounds: int
    changed: List[int]
    frozen_points: int
    converged: bool


def distanceFill(phi, nx: int, ny: int, nz: int, dx: float, *, band: Optional[float] = None, mask=None, max_rounds: int = 64) -> FillReport:
    """First-order distance on every point outside a frozen set, by fast sweeping (include/lsf.h: lsf_distance_fill); `phi` is
    updated in place.

    Exactly one of `band` / `mask`: band=w freezes the points with |phi| < w*dx on entry (the tube of meshDistance(width=w)),
    mask (int32, same layout as phi, e.g. phiNB of narrowBand) freezes the points where it is 1.  Frozen points are never
    written; every other point keeps its sign and receives the Godunov first-order solution of |grad phi| = 1, rounds of 8 raster
    sweeps until a round lowers nothing or max_rounds is reached (then converged is False).  The frozen set must separate the
    signs.  The result is first order (errors of 1 - 2 dx far from the surface on the test inputs); reinit afterwards is
    optional and shorter.
    """
    if (band is None) == (mask is None):
        raise ValueError("give exactly one of band= (cells; freezes |phi| < band*dx) and mask= (int32; freezes mask == 1)")
    cap = max(int(max_rounds), 1)
    trace = np.zeros(cap, dtype=np.int64)
    done = ctypes.c_int(0)
    frozen = ctypes.c_int64(0)
    s = Seam(phi, nx, ny, nz)
    _lib.check(s.call("lsf_distance_fill", s.field(phi, "phi"), s.optional(mask, "mask", np.int32), nx, ny, nz, float(dx),
                      0.0 if band is None else float(band), int(max_rounds), ctypes.byref(done), trace.ctypes.data, cap, ctypes.byref(frozen)))
    n = done.value
    changed = [int(v) for v in trace[:n]]
    return FillReport(n, changed, int(frozen.value), bool(n and changed[-1] == 0))


class ExtendReport(NamedTuple):
    """What lsf_extend_field reports (include/lsf.h): rounds of 8 sweeps run, the visits that changed a value in each of them, the
    size of the frozen set, the other points that hold a value / are still NaN, and whether the last round changed nothing."""
    rounds: int
    changed: List[int]
    frozen_points: int
    reached: int
    unreached: int
    converged: bool


def extendField(q, phi, nx: int, ny: int, nz: int, dx: float, *, band: Optional[float] = None, mask=None, max_rounds: int = 64) -> ExtendReport:
    """Carries `q` off a frozen set constant along the normals of `phi`, grad(q) . grad(phi) = 0 (include/lsf.h: lsf_extend_field);
    `q` is updated in place, `phi` and `mask` are read only.

    Exactly one of `band` / `mask`, as in distanceFill: band=w freezes the points with |phi| < w*dx, mask (int32, same layout)
    freezes the points where it is 1.  Frozen points keep the caller's q; what q holds elsewhere on entry is ignored.  Every other
    point receives the first-order upwind value, rounds of 8 raster sweeps until a round changes nothing or max_rounds is reached
    (then converged is False).  A point that a plateau of |phi| keeps out of reach stays NaN and is counted in `unreached`: run
    distanceFill or reinit on phi first.  q and phi are both numpy arrays or both torch CUDA tensors.
    """
    if (band is None) == (mask is None):
        raise ValueError("give exactly one of band= (cells; freezes |phi| < band*dx) and mask= (int32; freezes mask == 1)")
    s = Seam(q, nx, ny, nz, "q, phi and mask", (phi,), (mask,), kinds=_EXTEND_KINDS, check_device=False)
    cap = max(int(max_rounds), 1)
    trace = np.zeros(cap, dtype=np.int64)
    done = ctypes.c_int(0)
    info = np.zeros(_lib.LSF_EXTEND_INFO_LEN, dtype=np.int64)
    p, f, m = s.field(q, "q"), s.field(phi, "phi"), s.optional(mask, "mask", np.int32)
    s.one_device()
    _lib.check(s.call("lsf_extend_field", p, f, m, nx, ny, nz, float(dx), 0.0 if band is None else float(band), int(max_rounds),
                      ctypes.byref(done), trace.ctypes.data, cap, info.ctypes.data))
    n = done.value
    changed = [int(v) for v in trace[:n]]
    return ExtendReport(n, changed, int(info[0]), int(info[1]), int(info[2]), bool(n and changed[-1] == 0))


class ExtendBandReport(NamedTuple):
    """What lsf_extend_field_band reports (include/lsf.h): Jacobi passes run, whether the last one changed nothing, the visits that
    changed a value in each pass (at most trace_cap of them), the list cells, the frozen ones among them, and the other list cells
    that hold a value / are still NaN."""
    passes: int
    converged: bool
    trace: List[int]
    cells: int
    frozen: int
    reached: int
    unreached: int


_EXTEND_BAND_TRACE = 1 << 16  # passes whose counts the Python layer keeps at most


def extendFieldBand(q, phi, mask, dx: float, known=None, band: Optional[float] = None, max_passes: int = 256, trace_cap: Optional[int] = None):
    """Carries `q` off the frozen cells of the list of `mask` constant along the normals of `phi`, on the list only (include/lsf.h:
    lsf_extend_field_band).  Returns (q, ExtendBandReport); `q` is updated in place, `phi`, `mask` and `known` are read only.

    q, phi: 3-D float64 fields of one shape -- numpy, Fortran-ordered (nx+1, ny+1, nz+1), or torch CUDA tensors (nz+1, ny+1, nx+1);
    mask and known: int32, same layout and kind.  The list is the interior points with mask == 1, as in reinitBand, advectFieldBand
    and curvatureBand.  Exactly one of `known` / `band`: known freezes the list cells where it is 1, band=w those with
    |phi| < w*dx.  Frozen cells keep the caller's q; every other list cell receives the first-order upwind value by Jacobi passes
    until a pass changes nothing or max_passes is reached (then converged is False).  Points outside the list are neither read nor
    written in q -- NaN is fine there, which is what curvatureBand leaves -- and a list cell no value reaches stays NaN and is
    counted in `unreached`.  The recipe on one mask: curvatureBand -> extendFieldBand -> advectFieldBand / evolveBand.
    """
    if mask is None:
        raise ValueError("mask (int32) must be a field of phi's shape")
    if (known is None) == (band is None):
        raise ValueError("give exactly one of known= (int32; freezes the list cells with known == 1) and band= (cells; freezes |phi| < band*dx)")
    s = Seam(q, None, None, None, "q, phi, mask and known", (phi, mask), (known,), kinds=_EXTEND_KINDS, check_device=False)
    if not s.dev and not isinstance(q, np.ndarray):
        raise TypeError("q must be a numpy array of float64 or a CUDA tensor of torch.float64")
    if len(q.shape) != 3:
        raise ValueError("q must be a 3-D field: the grid size is taken from its shape")
    nx, ny, nz = (int(n) - 1 for n in (tuple(q.shape)[::-1] if s.dev else q.shape))  # i is the unit-stride axis of both
    s.nx, s.ny, s.nz = nx, ny, nz  # the grid is q's own, and its shape can be read only once the kinds are known to agree
    dx = _seam.positive(dx)
    if band is not None and (not (float(band) > 0.0) or float(band) == float("inf")):
        raise ValueError("band must be finite and > 0")
    max_passes = int(max_passes)
    if max_passes < 1:
        raise ValueError("max_passes must be >= 1")
    if trace_cap is not None and int(trace_cap) < 0:
        raise ValueError("trace_cap must be >= 0")
    p, f, m, k = s.field(q, "q"), s.field(phi, "phi"), s.field(mask, "mask", np.int32), s.optional(known, "known", np.int32)
    s.one_device()
    if p == f:
        raise ValueError("q and phi must be different arrays")
    cap = min(max_passes, _EXTEND_BAND_TRACE)
    trace = np.zeros(cap, dtype=np.int64)
    done = ctypes.c_int(0)
    info = np.zeros(_lib.LSF_EXTEND_BAND_INFO_LEN, dtype=np.int64)
    _lib.check(s.call("lsf_extend_field_band", p, f, m, k, nx, ny, nz, dx, 0.0 if band is None else float(band), max_passes, ctypes.byref(done),
                      trace.ctypes.data, cap, info.ctypes.data))
    n = done.value
    converged = n < max_passes or bool(0 < n <= cap and trace[n - 1] == 0)
    keep = min(n, cap if trace_cap is None else min(cap, int(trace_cap)))
    return q, ExtendBandReport(n, converged, [int(v) for v in trace[:keep]], int(info[0]), int(info[1]), int(info[2]), int(info[3]))


class RedistanceReport(NamedTuple):
    """What lsf_redistance_band reports (include/lsf_redistance.h): Jacobi passes of the fill, whether the last one lowered nothing,
    the visits that lowered a value in each pass, the largest |new - old| over the written cells, and the nine counts of info:
    list cells, the frozen, filled and unreached ones among them, and the feet by status (offband, outside, flat, not_converged;
    far = found, but not closer than near*dx).  frozen + offband + outside + flat + not_converged + far == cells ==
    frozen + filled + unreached."""
    passes: int
    converged: bool
    trace: List[int]
    change: float
    cells: int
    frozen: int
    filled: int
    unreached: int
    offband: int
    outside: int
    flat: int
    not_converged: int
    far: int


def redistanceBand(phi, mask, nx: int, ny: int, nz: int, dx: float, near: float = 2.5, iters: int = 8, tol: float = 1e-9,
                   max_passes: int = 64) -> RedistanceReport:
    """Redistances the list of `mask` from closest points, without pseudo-time sweeps (include/lsf_redistance.h:
    lsf_redistance_band); `phi` is updated in place, `mask` is read only.

    phi: float64, numpy Fortran-ordered (nx+1, ny+1, nz+1) or a torch CUDA tensor (nz+1, ny+1, nx+1); mask: int32, same layout and
    kind.  The list is the interior points with mask == 1, as in reinitBand.  A list cell whose foot on the cubic interpolant's zero
    level set is found (at most `iters` Newton steps to |phi| <= tol*dx) closer than near*dx takes that distance with the sign it
    had; the other list cells are filled from those by Jacobi passes of distanceFill's visit until a pass lowers nothing or
    max_passes is reached (then converged is False).  No cell changes the answer of (phi < 0); list cells no frozen cell reaches keep
    their value and are counted in `unreached`; points outside the list are neither read nor written.  near: 2 to 3 cells -- far
    from the surface the foot of a field that is not a distance is not the closest point.
    """
    dx = _seam.positive(dx)
    near = float(near)
    if not (np.isfinite(near) and near > 0.0):
        raise ValueError("near must be finite and > 0")
    iters = int(iters)
    if iters < 1:
        raise ValueError("iters must be >= 1")
    tol = float(tol)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0")
    max_passes = int(max_passes)
    if max_passes < 1:
        raise ValueError("max_passes must be >= 1")
    s = Seam(phi, nx, ny, nz)
    p, m = s.field(phi, "phi"), s.field(mask, "mask", np.int32)
    cap = min(max_passes, _EXTEND_BAND_TRACE)  # passes whose counts the Python layer keeps at most
    trace = np.zeros(cap, dtype=np.int64)
    done, change = ctypes.c_int(0), ctypes.c_double(0.0)
    info = np.zeros(_lib.LSF_REDISTANCE_INFO_LEN, dtype=np.int64)
    _lib.check(s.call("lsf_redistance_band", p, m, nx, ny, nz, dx, near, iters, tol, max_passes, ctypes.byref(done), trace.ctypes.data, cap,
                      ctypes.byref(change), info.ctypes.data))
    n = done.value
    converged = n < max_passes or bool(0 < n <= cap and trace[n - 1] == 0)
    return RedistanceReport(n, converged, [int(v) for v in trace[:min(n, cap)]], change.value, *(int(v) for v in info))


class AdvectReport(NamedTuple):
    """What lsf_advect_field reports (include/lsf.h): steps run, the CFL number (dt * max(|u|+|v|+|w|+|speed|)) / dx of the inputs,
    and the largest |new - old| over the interior cells of each step."""
    steps: int
    cfl: float
    change: List[float]


def advectField(phi, nx: int, ny: int, nz: int, dx: float, dt: float, steps: int, *, velocity=None, speed=None, scheme: str = "rk3",
                arith: str = "strict") -> AdvectReport:
    """Transport of the level set, phi_t + u.grad(phi) + F |grad(phi)| = 0, by `steps` explicit steps of size dt on the whole grid
    (include/lsf.h: lsf_advect_field); `phi` is updated in place.

    velocity: a 3-tuple (u, v, w) of fields with phi's layout and kind (numpy arrays on the host seam, CUDA tensors on the device
    seam, which runs on the tensor's current stream); speed: one such field, the speed along the normal (> 0 grows the region
    phi < 0).  At least one of the two; both are inputs, frozen for the call.  WENO5 one-sided derivatives (first order within
    three cells of a wall), upwinding by the sign of each velocity component and Godunov's Hamiltonian for the speed;
    scheme="rk3" (TVD Runge-Kutta of Shu and Osher) or "euler"; the extrapolation boundary condition after every stage.  The CFL
    number is reported, not judged: keep it below 1.  Raises LsfNaNError when a step produced a NaN (phi holds that step; the
    exception carries the AdvectReport as `.report`).
    """
    scheme, arith = _seam.named("scheme", scheme, _SCHEMES), _seam.named("arith", arith, _ARITHS)
    if velocity is None and speed is None:
        raise ValueError("give velocity=(u, v, w), speed=F, or both")
    inputs = _transport_fields(velocity, speed)
    s = Seam(phi, nx, ny, nz, "phi, velocity and speed", [f for _, f in inputs])
    cap = max(int(steps), 1)
    trace = np.zeros(cap, dtype=np.float64)
    done = ctypes.c_int(0)
    cfl = ctypes.c_double(0.0)
    p = s.field(phi, "phi")
    q = {n: s.field(f, n) for n, f in inputs}
    rc = s.call("lsf_advect_field", p, q.get("u"), q.get("v"), q.get("w"), q.get("speed"), nx, ny, nz, float(dx), float(dt), int(steps), scheme,
                LSF_ORDER_JACOBI | arith, ctypes.byref(done), ctypes.byref(cfl), trace.ctypes.data, cap)
    n = done.value
    return _check_report(rc, AdvectReport(n, float(cfl.value), [float(x) for x in trace[:n]]))


class AdvectBandReport(NamedTuple):
    """What lsf_advect_field_band reports (include/lsf.h): steps run, the CFL number of the inputs over the list cells, the largest
    |new - old| over the list cells of each step, the list cells, the edge cells among them (a neighbour outside the list), the edge
    cells whose sign changed during the call (> 0: the surface reached the edge of the list) and the smallest |phi| over the edge
    cells on return.  cells, edge_cells, edge_flips and margin are None where the library did not report them (LsfNaNError)."""
    steps: int
    cfl: float
    change: List[float]
    cells: Optional[int]
    edge_cells: Optional[int]
    edge_flips: Optional[int]
    margin: Optional[float]


def advectFieldBand(phi, mask, nx: int, ny: int, nz: int, dx: float, dt: float, steps: int, *, velocity=None, speed=None,
                    scheme: str = "rk3", arith: str = "strict") -> AdvectBandReport:
    """advectField on the cells of `mask` only (include/lsf.h: lsf_advect_field_band); `phi` is updated in place.

    mask: int32, phi's layout and kind (e.g. phiSB of narrowBand); the interior points where it is 1 take the steps of advectField,
    every other point -- wall points included -- keeps its value and no boundary condition is applied.  velocity, speed, scheme and
    arith as in advectField; the inputs are read at the list cells only (a NaN elsewhere is legal).  Make the mask wider than the band
    whose values are trusted and keep steps * cfl well below its width: `edge_flips` > 0 says the surface reached the edge of the
    list, and `margin` (compare it with a few dx) says when to rebuild the mask.  Raises LsfNaNError when a step produced a NaN (phi
    holds that step; the exception carries the AdvectBandReport as `.report`).
    """
    scheme, arith = _seam.named("scheme", scheme, _SCHEMES), _seam.named("arith", arith, _ARITHS)
    if velocity is None and speed is None:
        raise ValueError("give velocity=(u, v, w), speed=F, or both")
    inputs = _transport_fields(velocity, speed)
    if mask is None:
        raise ValueError("mask must be an int32 field of phi's shape")
    s = Seam(phi, nx, ny, nz, "phi, mask, velocity and speed", [f for _, f in inputs] + [mask])
    cap = max(int(steps), 1)
    trace = np.zeros(cap, dtype=np.float64)
    done = ctypes.c_int(0)
    cfl = ctypes.c_double(0.0)
    info = np.full(_lib.LSF_ADVECT_BAND_INFO_LEN, -1, dtype=np.int64)
    margin = ctypes.c_double(float("nan"))
    p, m = s.field(phi, "phi"), s.field(mask, "mask", np.int32)
    q = {n: s.field(f, n) for n, f in inputs}
    rc = s.call("lsf_advect_field_band", p, m, q.get("u"), q.get("v"), q.get("w"), q.get("speed"), nx, ny, nz, float(dx), float(dt), int(steps),
                scheme, LSF_ORDER_JACOBI | arith, ctypes.byref(done), ctypes.byref(cfl), trace.ctypes.data, cap, info.ctypes.data,
                ctypes.byref(margin))
    n = done.value
    told = rc == _lib.LSF_OK  # info and margin are written on LSF_OK only
    return _check_report(rc, AdvectBandReport(n, float(cfl.value), [float(x) for x in trace[:n]],
                                              *((int(v) for v in info) if told else (None, None, None)), float(margin.value) if told else None))


class EvolveBandReport(NamedTuple):
    """What lsf_evolve_band reports (include/lsf.h): steps run, the CFL number of the inputs over all points, the largest |new - old|
    over the list cells of each step's transport, then info[0..5] -- the list cells on return, the open-edge cells among them (an
    interior neighbour outside the list), the open-edge cells whose sign had changed at the last check (> 0: the surface reached the
    edge between two checks and the call ended there), the rebuilds, the cells that entered over all rebuilds, the wall-adjacent list
    cells with |phi| < core dx -- and the smallest |phi| over the open-edge cells on return.  The last seven are None where the
    library did not report them (LsfNaNError)."""
    steps: int
    cfl: float
    change: List[float]
    cells: Optional[int]
    open_cells: Optional[int]
    flips: Optional[int]
    rebuilds: Optional[int]
    entered: Optional[int]
    near_wall: Optional[int]
    margin: Optional[float]


def evolveBand(phi, mask, nx: int, ny: int, nz: int, dx: float, dt: float, steps: int, *, velocity=None, speed=None, scheme: str = "rk3",
               arith: str = "strict", core: float = 3.0, ring: int = 3, reinit_sweeps: int = 2, h: Optional[float] = None,
               check_every: int = 1) -> EvolveBandReport:
    """The band time loop (include/lsf.h: lsf_evolve_band): per step the transport of advectFieldBand, `reinit_sweeps` sweeps of
    reinitBand and, every `check_every` steps, a look at the open edge of the list; `phi` AND `mask` are updated in place.

    mask: int32, phi's layout and kind; on entry the interior points where it is 1 are the list, on return it is 1 on the cells of
    the current list and 0 elsewhere.  When the smallest |phi| over the open-edge cells falls below core*dx the list is rebuilt: the
    cells with |phi| < core*dx dilated by `ring` cells, entering cells set to -+(core + ring)*dx for the sweeps to correct (so keep
    reinit_sweeps > 0, ring >= 3 and check_every * cfl well below core).  h: the pseudo-time step of the sweeps, 0.5*dx when None.
    velocity, speed, scheme and arith as in advectField; the inputs must be finite at all points.  `flips` > 0 in the report says the
    call ended early (`steps` < the steps asked for).  Raises LsfNaNError when a step produced a NaN (phi holds that step; the
    exception carries the EvolveBandReport as `.report`).
    """
    return _evolve_band(phi, mask, nx, ny, nz, dx, dt, steps, velocity, speed, scheme, arith, core, ring, reinit_sweeps, h, check_every, None)


def _evolve_band(phi, mask, nx, ny, nz, dx, dt, steps, velocity, speed, scheme, arith, core, ring, reinit_sweeps, h, check_every, curv):
    """evolveBand (curv is None) and evolveBandCurv (curv = (curvature, clamp)): validation, the pointers, the call, the report"""
    scheme, arith = _seam.named("scheme", scheme, _SCHEMES), _seam.named("arith", arith, _ARITHS)
    if curv is not None:
        bcurv, clamp = (float(x) for x in curv)
        if not (bcurv >= 0.0) or bcurv == float("inf"):
            raise ValueError("curvature must be finite and >= 0")
        if not (clamp >= 0.0) or clamp == float("inf"):
            raise ValueError("clamp must be finite and >= 0 (0: no clamp)")
        if velocity is None and speed is None and bcurv == 0.0:
            raise ValueError("give velocity=(u, v, w), speed=F, a curvature > 0, or several of them")
    elif velocity is None and speed is None:
        raise ValueError("give velocity=(u, v, w), speed=F, or both")
    inputs = _transport_fields(velocity, speed)
    if mask is None:
        raise ValueError("mask must be an int32 field of phi's shape")
    if h is None:
        h = 0.5 * float(dx)
    if not (float(core) > 0.0 and np.isfinite(float(core))):
        raise ValueError("core must be finite and > 0")
    if int(ring) != ring or not 1 <= int(ring) <= 8:
        raise ValueError("ring must be an integer in 1..8")
    if int(reinit_sweeps) != reinit_sweeps or reinit_sweeps < 0:
        raise ValueError("reinit_sweeps must be an integer >= 0")
    if reinit_sweeps > 0 and not (float(h) > 0.0 and np.isfinite(float(h))):
        raise ValueError("h must be finite and > 0")
    if int(check_every) != check_every or check_every < 1:
        raise ValueError("check_every must be an integer >= 1")
    s = Seam(phi, nx, ny, nz, "phi, mask, velocity and speed", [f for _, f in inputs] + [mask])
    cap = max(int(steps), 1)
    trace = np.zeros(cap, dtype=np.float64)
    done = ctypes.c_int(0)
    cfl = ctypes.c_double(0.0)
    info = np.full(_lib.LSF_EVOLVE_INFO_LEN, -1, dtype=np.int64)
    margin = ctypes.c_double(float("nan"))
    p, m = s.field(phi, "phi"), s.field(mask, "mask", np.int32)
    q = {n: s.field(f, n) for n, f in inputs}
    diffusion = ctypes.c_double(0.0)
    head = (p, m, q.get("u"), q.get("v"), q.get("w"), q.get("speed"), nx, ny, nz, float(dx), float(dt), int(steps), scheme, LSF_ORDER_JACOBI | arith,
            float(core), int(ring), int(reinit_sweeps), float(h), int(check_every))
    tail = (trace.ctypes.data, cap, info.ctypes.data, ctypes.byref(margin))
    if curv is None:
        rc = s.call("lsf_evolve_band", *head, ctypes.byref(done), ctypes.byref(cfl), *tail)
    else:
        rc = s.call("lsf_evolve_band_curv", *head, bcurv, clamp, ctypes.byref(done), ctypes.byref(cfl), ctypes.byref(diffusion), *tail)
    n = done.value
    told = rc == _lib.LSF_OK  # info and margin are written on LSF_OK only
    rest = (*((int(v) for v in info) if told else (None,) * 6), float(margin.value) if told else None)
    if curv is None:
        return _check_report(rc, EvolveBandReport(n, float(cfl.value), [float(x) for x in trace[:n]], *rest))
    return _check_report(rc, EvolveBandCurvReport(n, float(cfl.value), float(diffusion.value), [float(x) for x in trace[:n]], *rest))


class EvolveBandCurvReport(NamedTuple):
    """What lsf_evolve_band_curv reports (include/lsf.h): EvolveBandReport's fields with `diffusion`, the number
    curvature*dt/dx^2 of the explicit curvature term (reported, never judged), after `cfl`."""
    steps: int
    cfl: float
    diffusion: float
    change: List[float]
    cells: Optional[int]
    open_cells: Optional[int]
    flips: Optional[int]
    rebuilds: Optional[int]
    entered: Optional[int]
    near_wall: Optional[int]
    margin: Optional[float]


def evolveBandCurv(phi, mask, nx: int, ny: int, nz: int, dx: float, dt: float, steps: int, *, curvature: float, velocity=None, speed=None,
                   clamp: float = 1.0, scheme: str = "rk3", arith: str = "strict", core: float = 3.0, ring: int = 3, reinit_sweeps: int = 2,
                   h: Optional[float] = None, check_every: int = 1) -> EvolveBandCurvReport:
    """The band time loop with a curvature term (include/lsf.h: lsf_evolve_band_curv): evolveBand for
    phi_t + u.grad(phi) + F |grad(phi)| = curvature * kappa * |grad(phi)|, the term differenced centrally from each stage's own input
    field -- the speed law F = a - b*kappa with b = `curvature`, run inside one call.

    Everything is evolveBand's except: `curvature` (finite, >= 0) is b; `clamp` limits |kappa| to clamp/dx as in curvatureBand (0: no
    clamp); velocity and speed may both be absent when curvature > 0 (motion by mean curvature: a sphere of radius R0 shrinks to
    sqrt(R0^2 - 4 b t)); the report carries `diffusion` = b*dt/dx^2.  The term is explicit: keep `diffusion` small (the heat stencil's
    bound for Euler is 1/6).  curvature=0 with a velocity or a speed is evolveBand bit for bit.
    """
    return _evolve_band(phi, mask, nx, ny, nz, dx, dt, steps, velocity, speed, scheme, arith, core, ring, reinit_sweeps, h, check_every,
                        (curvature, clamp))


class CurvatureReport(NamedTuple):
    """What lsf_curvature_band reports (include/lsf.h): the list cells, those with |grad(phi)|^2 < 1e-24 (kappa = gauss = 0 there),
    those where the clamp changed a written value, and the largest |kappa| as stored over the list cells."""
    cells: int
    degenerate: int
    clamped: int
    kappa_max: float


def curvatureBand(phi, mask, nx: int, ny: int, nz: int, dx: float, kappa, *, gauss=None, gmag=None, clamp: float = 0.0) -> CurvatureReport:
    """Mean curvature k1 + k2 = div(grad(phi)/|grad(phi)|) of the level sets of `phi` on the cells of `mask` only (include/lsf.h:
    lsf_curvature_band), written into `kappa`; optionally the Gaussian curvature k1 * k2 into `gauss` and |grad(phi)| into `gmag`.

    mask: int32, phi's layout and kind; the interior points where it is 1 are the list.  kappa, gauss, gmag: fields of phi's layout
    and kind, written at the list cells and nowhere else -- what they hold at other points stays, NaNs included, so kappa can be
    handed to advectFieldBand as (part of) `speed` on the same mask.  phi and mask are read only.  Second-order central differences;
    a sphere with phi < 0 inside has kappa = +2/r.  clamp=c > 0 limits |kappa| to c/dx and |gauss| to (c/dx)^2 (a grid cannot resolve
    more than 1/dx: clamp=1 is the usual choice); 0 means no clamp.  Raises LsfNaNError when a list cell received a non-finite
    value (the outputs hold what was computed; the message carries the count).  All arrays are numpy arrays (host seam) or all are
    torch CUDA tensors (device seam, on the tensor's current stream).
    """
    if mask is None or kappa is None:
        raise ValueError("mask (int32) and kappa (float64) must be fields of phi's shape")
    s = Seam(phi, nx, ny, nz, "phi, mask, kappa, gauss and gmag", (mask, kappa), (gauss, gmag))
    clamp = float(clamp)
    if not (clamp >= 0.0) or clamp == float("inf"):
        raise ValueError("clamp must be finite and >= 0 (0: no clamp)")
    info = np.zeros(_lib.LSF_CURV_INFO_LEN, dtype=np.int64)
    kmax = ctypes.c_double(0.0)
    _lib.check(s.call("lsf_curvature_band", s.field(phi, "phi"), s.field(mask, "mask", np.int32), s.field(kappa, "kappa"),
                      s.optional(gauss, "gauss"), s.optional(gmag, "gmag"), nx, ny, nz, float(dx), clamp, info.ctypes.data, ctypes.byref(kmax)))
    return CurvatureReport(int(info[0]), int(info[1]), int(info[2]), float(kmax.value))


class MeasureReport(NamedTuple):
    """What lsf_measure_band reports (include/lsf.h): M as named fields -- `centroid` is the body's (volume moments / volume) and
    `surface_centroid` the surface's (surface moments / area), NaN where the divisor is 0 -- and info[0..4].  `open` > 0: the surface
    may continue outside the list, and volume and centroid then describe an open piece."""
    area: float
    volume: float
    centroid: tuple
    surface_centroid: tuple
    q_integral: float
    cells: int
    crossed: int
    triangles: int
    open: int
    degenerate: int


def measureBand(phi, mask, nx: int, ny: int, nz: int, dx: float, xLo, iso: float = 0.0, q=None, cell_area=None) -> MeasureReport:
    """Area, enclosed volume, centroids and the integral of `q` over the level set phi = iso, summed on the cells of `mask` only
    (include/lsf.h: lsf_measure_band): the triangles extractSurface would emit for the cells whose lower corner is a list point,
    measured where they are and never emitted.

    mask: int32, phi's layout and kind; the interior points where it is 1 are the list (any mask of |phi| < 2.1 dx or wider holds the
    crossed cells of a distance field).  q: a field of phi's layout and kind, read on the endpoints of crossed edges only -- NaN
    anywhere else is fine, which is what curvatureBand leaves.  cell_area: a field of phi's layout and kind that receives, at every
    list point, the area of the surface inside the cell the point names, and is left alone elsewhere.  phi, mask and q are read only.
    The grid point (i,j,k) is xLo + (i,j,k)*dx; volume and centroid are taken about the origin of that frame.  The totals are
    bit-identical from run to run and between the seams.  All arrays are numpy arrays (host seam) or all are torch CUDA tensors
    (device seam, on the tensor's current stream).
    """
    if mask is None:
        raise ValueError("mask (int32) must be a field of phi's shape")
    lo, dx, iso = _seam.xlo(xLo), _seam.positive(dx), _seam.finite_iso(iso)
    s = Seam(phi, nx, ny, nz, "phi, mask, q and cell_area", (mask,), (q, cell_area))
    M = np.zeros(_lib.LSF_MEASURE_LEN, dtype=np.float64)
    info = np.zeros(_lib.LSF_MEASURE_INFO_LEN, dtype=np.int64)
    _lib.check(s.call("lsf_measure_band", s.field(phi, "phi"), s.field(mask, "mask", np.int32), s.optional(q, "q"),
                      s.optional(cell_area, "cell_area"), nx, ny, nz, dx, lo.ctypes.data, iso, M.ctypes.data, info.ctypes.data))
    M = [float(v) for v in M]
    over = lambda num, den: tuple(v / den if den != 0.0 else float("nan") for v in num)
    return MeasureReport(M[0], M[1], over(M[2:5], M[1]), over(M[5:8], M[0]), M[8], *(int(v) for v in info))


class CutCellsReport(NamedTuple):
    """What lsf_cut_cells_band reports (include/lsf.h): the volume of the body over the list cells, the smallest stored fraction of
    a cut cell (+inf without one) and info[0..4].  `open` > 0: a cut cell has a face neighbour outside the list, whose lower-face
    aperture (this cell's upper one) the caller therefore lacks."""
    volume: float
    vof_min: float
    cells: int
    cut: int
    full: int
    open: int
    clamped: int


def cutCellsBand(phi, mask, nx: int, ny: int, nz: int, dx: float, iso: float = 0.0, vof=None, aperture=None, area_vector=None) -> CutCellsReport:
    """Volume fraction, lower-face apertures and surface area vector of every cell of `mask`, for the body phi < iso
    (include/lsf.h: lsf_cut_cells_band): the cell a list point names is cut by the triangles extractSurface would emit for it.

    mask: int32, phi's layout and kind; the interior points where it is 1 are the list.  vof: a field of phi's layout and kind that
    receives the fraction of each list cell inside the body; aperture: a 3-tuple (ax, ay, az) of such fields for the open fractions
    of the cell's lower faces; area_vector: a 3-tuple (bx, by, bz) for the surface's outward area vector in units of dx^2.  Each is
    written at list points only and may be left out; the report's volume is always formed.  phi and mask are read only.  All
    arrays are numpy arrays (host seam) or all are torch CUDA tensors (device seam, on the tensor's current stream).
    """
    if mask is None:
        raise ValueError("mask (int32) must be a field of phi's shape")
    dx, iso = _seam.positive(dx), _seam.finite_iso(iso)
    outs = [] if vof is None else [("vof", vof)]
    for name, group, parts in (("aperture", aperture, ("ax", "ay", "az")), ("area_vector", area_vector, ("bx", "by", "bz"))):
        if group is None:
            continue
        if not isinstance(group, (tuple, list)) or len(group) != 3 or any(a is None for a in group):
            raise ValueError(f"{name} must be a 3-tuple of fields of phi's shape")
        outs += list(zip(parts, group))
    s = Seam(phi, nx, ny, nz, "phi, mask and the outputs", [a for _, a in outs] + [mask])
    p, m = s.field(phi, "phi"), s.field(mask, "mask", np.int32)
    o = {n: s.field(a, n) for n, a in outs}
    tot = np.zeros(2, dtype=np.float64)  # volume, vof_min
    info = np.zeros(_lib.LSF_CUT_INFO_LEN, dtype=np.int64)
    _lib.check(s.call("lsf_cut_cells_band", p, m, nx, ny, nz, dx, iso, *(o.get(n) for n in ("vof", "ax", "ay", "az", "bx", "by", "bz")),
                      tot.ctypes.data, tot.ctypes.data + 8, info.ctypes.data))
    return CutCellsReport(float(tot[0]), float(tot[1]), *(int(v) for v in info))


class LabelReport(NamedTuple):
    """What lsf_label_band reports (include/lsf.h): the number of components, the first min(ncomp, comp_cap) rows of the table (int64,
    shape (rows, 10): root index, cells, -1 INSIDE / +1 OUTSIDE, imin, imax, jmin, jmax, kmin, kmax, edge cells; ascending root index),
    the passes run, whether the last pass found no link any more (`certified`: the labels are final) and the raw info[0..7]."""
    ncomp: int
    components: np.ndarray
    passes: int
    certified: bool
    info: tuple


_LABEL_SIDES = {"inside": _lib.LSF_LABEL_INSIDE, "outside": _lib.LSF_LABEL_OUTSIDE, "both": _lib.LSF_LABEL_BOTH}


def labelBand(phi, mask, nx: int, ny: int, nz: int, label, *, iso: float = 0.0, side: str = "inside", max_passes: int = 64,
              comp_cap=None) -> LabelReport:
    """The 6-connected components of the cells of `mask` on either side of phi = iso (include/lsf.h: lsf_label_band): how many bodies
    there are and which cell belongs to which.

    mask: int32, phi's layout and kind; the interior points where it is 1 are the list.  label: int32, phi's layout and kind, written
    at the list cells and nowhere else: a labelled cell receives the point index i + (nx+1)*(j + (ny+1)*k) of the smallest point of its
    component, a list cell of the class `side` leaves out receives -1.  side: "inside" (phi - iso < 0), "outside" (everything else,
    phi == iso included) or "both"; a component never holds cells of both classes.  Two cells are linked when they are face
    neighbours, both in the list and of one class.  phi and mask are read only; phi is read at list cells only.  comp_cap: the rows of
    the table to return at most (None: 1024); `ncomp` counts every component.  A row's last entry counts the component's cells at the
    edge of the list: 0 means it is closed inside the list.  `certified` False (max_passes ran out): the labels are a refinement of
    the truth.  All arrays are numpy arrays (host seam) or all are torch CUDA tensors (device seam, on the tensor's current stream).

    Compact ids 0 .. ncomp-1 (ncomp <= comp_cap), at the labelled cells:
        rep = labelBand(phi, mask, nx, ny, nz, label)
        ids = np.searchsorted(rep.components[:, 0], label[label >= 0])
    """
    if mask is None or label is None:
        raise ValueError("mask and label (int32) must be fields of phi's shape")
    if side not in _LABEL_SIDES:
        raise ValueError('side must be "inside", "outside" or "both"')
    iso, max_passes = _seam.finite_iso(iso), int(max_passes)
    if max_passes < 1:
        raise ValueError("max_passes must be >= 1")
    cap = 1024 if comp_cap is None else int(comp_cap)
    if cap < 0:
        raise ValueError("comp_cap must be >= 0")
    s = Seam(phi, nx, ny, nz, "phi, mask and label", (mask, label))
    comp = np.zeros((cap, _lib.LSF_LABEL_COMP_LEN), dtype=np.int64)
    info = np.zeros(_lib.LSF_LABEL_INFO_LEN, dtype=np.int64)
    ncomp = ctypes.c_int64(0)
    _lib.check(s.call("lsf_label_band", s.field(phi, "phi"), s.field(mask, "mask", np.int32), s.field(label, "label", np.int32), nx, ny, nz, iso,
                      _LABEL_SIDES[side], max_passes, comp.ctypes.data if cap else None, cap, ctypes.byref(ncomp), info.ctypes.data))
    n = int(ncomp.value)
    return LabelReport(n, comp[:min(n, cap)].copy(), int(info[4]), int(info[5]) == 0, tuple(int(v) for v in info))


class SampleReport(NamedTuple):
    """What lsf_sample_points returns (include/lsf.h): `val` (npts), `grad` (npts, 3; None with want_grad=False), `qval` (npts; None
    without q), `foot` (npts, 3; None with iters == 0), `status` (npts, int32: 0 OK, 1 OUTSIDE, 2 OFFBAND, 3 FLAT, 4 NOT_CONVERGED)
    and `info`, the six counts [OK, OUTSIDE, OFFBAND, linear fallbacks of a cubic request, FLAT, NOT_CONVERGED].  The (npts, 3)
    arrays are Fortran-ordered, the layout of surfX."""
    val: object
    grad: object
    qval: object
    foot: object
    status: object
    info: tuple


def samplePoints(phi, nx: int, ny: int, nz: int, dx: float, xLo, pts, *, order: str = "cubic", mask=None, q=None, iso: float = 0.0,
                 iters: int = 0, tol: float = 1e-6, want_grad: bool = True) -> SampleReport:
    """The field at arbitrary points (include/lsf.h: lsf_sample_points): phi, its gradient, a second field q and, with iters >= 1, the
    foot of each point on the level set phi = iso, interpolated trilinearly (order="linear") or by Catmull-Rom cubics ("cubic",
    linear in the cells next to the walls).

    pts: (npts, 3) float64 in Fortran order -- what extractSurface returns as surfX plugs in; it is never written.  mask: int32 field;
    a point whose stencil leaves the interior points with mask == 1 is refused with status OFFBAND, which makes a q that exists on
    a list only (kappa of curvatureBand) safe to sample.  A point outside the grid, NaN and inf included, gets status OUTSIDE.
    Refused points hold NaN in every output.  phi, mask, q and pts are read only.  The grid point (i,j,k) is xLo + (i,j,k)*dx.
    Numpy in gives numpy out (host seam); CUDA tensors in give CUDA tensors out (device seam, on the tensor's current stream).
    """
    lo, dx, iso, tol, iters = _seam.xlo(xLo), _seam.positive(dx), _seam.finite_iso(iso), float(tol), int(iters)
    order = _seam.named("order", order, _SAMPLE_ORDERS)
    if iters < 0:
        raise ValueError("iters must be >= 0")
    if iters >= 1 and not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0")
    _seam.grid(nx, ny, nz)
    s = Seam(phi, nx, ny, nz, "phi, mask, q and pts", (pts,), (mask, q))
    npts = s.points(pts)
    p, m, qq = s.field(phi, "phi"), s.optional(mask, "mask", np.int32), s.optional(q, "q")
    info = np.zeros(_lib.LSF_SAMPLE_INFO_LEN, dtype=np.int64)
    val, status = s.out(npts), s.out(npts, np.int32)
    grad = s.out3(npts) if want_grad else None
    qval = s.out(npts) if q is not None else None
    foot = s.out3(npts) if iters >= 1 else None
    _lib.check(s.call("lsf_sample_points", p, m, qq, nx, ny, nz, dx, lo.ctypes.data, s.ptr(pts), npts, order, iso, iters, tol, s.ptr(val),
                      s.ptr(grad), s.ptr(qval), s.ptr(foot), s.ptr(status), info.ctypes.data))
    return SampleReport(val, grad, qval, foot, status, tuple(int(v) for v in info))


class CastReport(NamedTuple):
    """What lsf_cast_rays returns (include/lsf.h): `thit` (nrays; the length along the ray to the hit, the end of the march for a MISS,
    NaN otherwise), `hit` (nrays, 3; None with want_hit=False), `grad` (nrays, 3; None with want_grad=False), `qval` (nrays; None
    without q), `status` (nrays, int32: 0 HIT, 1 MISS, 2 NOGRID, 3 BAD, 4 LOST, 5 STEPS) and `info`, the nine counts [HIT, MISS, NOGRID,
    BAD, LOST, STEPS, samples of phi taken, off-list strides, rays that began on the inner side].  The (nrays, 3) arrays are
    Fortran-ordered, the layout of surfX."""
    thit: object
    hit: object
    grad: object
    qval: object
    status: object
    info: tuple


def castRays(phi, nx: int, ny: int, nz: int, dx: float, xLo, org, dir, *, order: str = "cubic", mask=None, q=None, iso: float = 0.0,
             tmin: float = 0.0, tmax: float = 1e30, safety: float = 0.9, smin: float = 0.05, smax: float = 1.0, skip: float = 1.0,
             refine: int = 24, max_steps: int = 4096, want_hit: bool = True, want_grad: bool = True) -> CastReport:
    """The first hit of each ray org + t * dir / |dir|, tmin <= t <= tmax, with the level set phi = iso (include/lsf.h: lsf_cast_rays):
    a march in steps of safety * |phi - iso|, kept between smin and smax cells, over the interpolant of samplePoints (order="linear"
    or "cubic"), `refine` bisections of the first sign change and one secant step.

    org, dir: (nrays, 3) float64 in Fortran order -- what extractSurface returns as surfX and samplePoints as grad plug in; they are
    never written.  mask: int32 field; where a sample's stencil leaves the interior points with mask == 1 the ray strides on by
    `skip` cells without reading phi, and a sign change found across such a gap is reported as LOST, never as a hit.  q: a second
    field, sampled at the hit.  A ray that is not HIT holds NaN in hit, grad and qval.  More than max_steps steps: status STEPS.
    Numpy in gives numpy out (host seam); CUDA tensors in give CUDA tensors out (device seam, on the tensor's current stream).
    """
    lo, dx, iso = _seam.xlo(xLo), _seam.positive(dx), _seam.finite_iso(iso)
    tmin, tmax, safety, smin, smax, skip = (float(v) for v in (tmin, tmax, safety, smin, smax, skip))
    refine, max_steps = int(refine), int(max_steps)
    order = _seam.named("order", order, _SAMPLE_ORDERS)
    if not (np.isfinite(tmin) and tmin >= 0.0 and np.isfinite(tmax) and tmax > tmin):
        raise ValueError("tmin must be finite and >= 0, tmax finite and > tmin")
    if not (0.0 < safety <= 1.0):
        raise ValueError("safety must lie in (0, 1]")
    if not (np.isfinite(smin) and smin > 0.0 and np.isfinite(smax) and smax >= smin):
        raise ValueError("smin must be finite and > 0, smax finite and >= smin")
    if not (np.isfinite(skip) and skip > 0.0):
        raise ValueError("skip must be finite and > 0")
    if refine < 0 or max_steps < 1:
        raise ValueError("refine must be >= 0 and max_steps >= 1")
    _seam.grid(nx, ny, nz)
    s = Seam(phi, nx, ny, nz, "phi, mask, q, org and dir", (org, dir), (mask, q))
    if len(org.shape) != 2 or org.shape[1] != 3 or org.shape[0] < 1 or tuple(dir.shape) != tuple(org.shape):
        raise ValueError("org and dir must have one shape (nrays, 3) with nrays >= 1")
    nrays = s.points(org, "org", "nrays")
    s.points(dir, "dir", "nrays")
    p, m, qq = s.field(phi, "phi"), s.optional(mask, "mask", np.int32), s.optional(q, "q")
    info = np.zeros(_lib.LSF_CAST_INFO_LEN, dtype=np.int64)
    thit, status = s.out(nrays), s.out(nrays, np.int32)
    hit = s.out3(nrays) if want_hit else None
    grad = s.out3(nrays) if want_grad else None
    qval = s.out(nrays) if q is not None else None
    _lib.check(s.call("lsf_cast_rays", p, m, qq, nx, ny, nz, dx, lo.ctypes.data, s.ptr(org), s.ptr(dir), nrays, order, iso, tmin, tmax, safety,
                      smin, smax, skip, refine, max_steps, s.ptr(thit), s.ptr(hit), s.ptr(grad), s.ptr(qval), s.ptr(status), info.ctypes.data))
    return CastReport(thit, hit, grad, qval, status, tuple(int(v) for v in info))


class AdvectPointsReport(NamedTuple):
    """What lsf_advect_points returns (include/lsf.h): `pts` (npts, 3; the moved points, Fortran-ordered), `status` (npts, int32: 0 OK,
    1 OUTSIDE, 2 OFFBAND, 3 FLAT), `cfl` (the largest |dt * k| / dx over the completed steps) and `info`, the six counts [OK, OUTSIDE,
    OFFBAND, FLAT, completed steps summed over the points, linear fallbacks of a cubic request]."""
    pts: object
    status: object
    cfl: float
    info: tuple


def advectPoints(pts, nx: int, ny: int, nz: int, dx: float, xLo, dt: float, steps: int, *, velocity=None, speed=None, phi=None, mask=None,
                 order: str = "cubic", scheme: str = "rk3") -> AdvectPointsReport:
    """Points carried through the fields that move phi (include/lsf.h: lsf_advect_points): x' = velocity(x) + speed(x) * grad phi(x) /
    |grad phi(x)| in fields frozen for the call, `steps` steps of TVD-RK3 ("rk3") or Euler ("euler") of size dt (dt < 0 traces
    backwards), over the interpolant of samplePoints (order="linear" or "cubic").

    pts: (npts, 3) float64 in Fortran order -- tracers, the surfX of extractSurface, markers of seedParticles; it is never written:
    the moved points come back in the report.  velocity: (u, v, w) fields; speed needs phi and phi needs speed.  A point that leaves
    the grid, walks off the mask or meets a flat phi keeps the position of its last completed step and says why in status.
    Numpy in gives numpy out (host seam); CUDA tensors in give CUDA tensors out (device seam, on the tensor's current stream).
    """
    lo, dx = _seam.xlo(xLo), _seam.positive(dx)
    _seam.grid(nx, ny, nz)
    dt, steps = float(dt), int(steps)
    if not np.isfinite(dt):
        raise ValueError("dt must be finite")
    order, scheme = _seam.named("order", order, _SAMPLE_ORDERS), _seam.named("scheme", scheme, _SCHEMES)
    if not 1 <= steps <= _lib.LSF_ADVECT_POINTS_MAX_STEPS:
        raise ValueError(f"steps must be in 1..{_lib.LSF_ADVECT_POINTS_MAX_STEPS}")
    if velocity is not None and (len(velocity) != 3 or any(f is None for f in velocity)):
        raise ValueError("velocity must be (u, v, w)")
    if velocity is None and speed is None:
        raise ValueError("neither a velocity nor a speed is given")
    if (speed is None) != (phi is None):
        raise ValueError("speed and phi are given together")
    u, v, w = (None, None, None) if velocity is None else velocity
    s = Seam(pts, nx, ny, nz, "pts and the fields", optional=(u, v, w, phi, speed, mask), check_device=False)
    npts = s.points(pts)
    s.one_device()
    f = [s.optional(a, n) for n, a in (("u", u), ("v", v), ("w", w), ("phi", phi), ("speed", speed))] + [s.optional(mask, "mask", np.int32)]
    info = np.zeros(_lib.LSF_ADVECT_POINTS_INFO_LEN, dtype=np.int64)
    cfl = ctypes.c_double(0.0)
    out, status = s.copy3(pts), s.out(npts, np.int32)
    _lib.check(s.call("lsf_advect_points", *f, nx, ny, nz, dx, lo.ctypes.data, s.ptr(out), npts, order, scheme, dt, steps, s.ptr(status),
                      ctypes.byref(cfl), info.ctypes.data))
    return AdvectPointsReport(out, status, float(cfl.value), tuple(int(v) for v in info))


class CorrectReport(NamedTuple):
    """What lsf_correct_field returns (include/lsf.h): `status` (npts, int32: 0 INPLACE, 1 ESCAPED, 2 OUTSIDE, 3 OFFBAND, 4 NONFINITE,
    5 BADRADIUS), `change` (the largest |new - old| over the points whose bits changed) and `info`, the seven counts [INPLACE, ESCAPED,
    OUTSIDE, OFFBAND, NONFINITE, BADRADIUS, points whose bits changed]."""
    status: object
    change: float
    info: tuple


def correctField(phi, nx: int, ny: int, nz: int, dx: float, xLo, pts, rad, *, mask=None, slack: float = 1.0) -> CorrectReport:
    """The correction step of the particle level set (include/lsf.h: lsf_correct_field): phi, in place, is rebuilt around every marker
    that has ESCAPED -- one that sits on the wrong side of the surface by more than slack times its radius -- from the marker's sphere.

    pts: (npts, 3) float64 in Fortran order; rad: (npts) float64, the side in its sign (> 0: the marker belongs where phi > 0) and the
    radius in its magnitude (seedParticles makes both).  With a mask only list cells are corrected and markers whose cell has a corner
    off the list are left out (status OFFBAND).  The result does not depend on the order of the particles.  Numpy in: host seam; CUDA
    tensors in: device seam, on the tensor's current stream.
    """
    lo, dx = _seam.xlo(xLo), _seam.positive(dx)
    _seam.grid(nx, ny, nz)
    slack = float(slack)
    if not (np.isfinite(slack) and slack >= 0.0):
        raise ValueError("slack must be finite and >= 0")
    s = Seam(phi, nx, ny, nz, "phi, mask, pts and rad", (pts, rad), (mask,), check_device=False)
    npts = s.points(pts)
    s.one_device()
    s.vector(rad, npts, "rad")
    p, m = s.field(phi, "phi"), s.optional(mask, "mask", np.int32)
    info = np.zeros(_lib.LSF_CORRECT_INFO_LEN, dtype=np.int64)
    change = ctypes.c_double(0.0)
    status = s.out(npts, np.int32)
    _lib.check(s.call("lsf_correct_field", p, m, nx, ny, nz, dx, lo.ctypes.data, s.ptr(pts), s.ptr(rad), npts, slack, s.ptr(status),
                      ctypes.byref(change), info.ctypes.data))
    return CorrectReport(status, float(change.value), tuple(int(v) for v in info))


def seedParticles(phi, nx: int, ny: int, nz: int, dx: float, xLo, *, mask=None, per_cell: int = 16, rmin: float = 0.1, rmax: float = 0.5,
                  band: float = 3.0, seed: int = 0):
    """Marker particles for correctField, on the host (run once per simulation and at reseeds): (pts (npts, 3) Fortran-ordered, rad).

    The cells whose 8 corners all have |phi| < band * dx (and, under a mask, are all interior points with mask == 1) each get per_cell
    points drawn uniformly from np.random.default_rng(seed), cell after cell with k the slowest index; phi is sampled there with
    samplePoints(order="linear"); the points with rmin * dx <= |val| <= band * dx are kept and rad = sign(val) * clip(|val|, rmin * dx,
    rmax * dx).  phi and mask are numpy arrays of shape (nx+1, ny+1, nz+1) in Fortran order.
    """
    lo, dx = _seam.xlo(xLo), _seam.positive(dx)
    _seam.grid(nx, ny, nz)
    f = np.asarray(phi)
    if f.shape != (nx + 1, ny + 1, nz + 1):
        raise ValueError("phi must be a numpy array of shape (nx+1, ny+1, nz+1)")
    near = np.abs(f) < band * dx
    if mask is not None:
        lst = np.zeros(f.shape, bool)
        lst[1:-1, 1:-1, 1:-1] = np.asarray(mask)[1:-1, 1:-1, 1:-1] == 1
        near &= lst
    c = near[:-1, :-1, :-1].copy()
    for oa in range(2):
        for ob in range(2):
            for oc in range(2):
                c &= near[oa:nx + oa, ob:ny + ob, oc:nz + oc]
    cells = np.argwhere(c)
    off = np.random.default_rng(seed).random((cells.shape[0], int(per_cell), 3))
    pts = np.asfortranarray((lo + (cells[:, None, :] + off) * dx).reshape(-1, 3))
    if not pts.shape[0]:
        return np.zeros((0, 3), order="F"), np.zeros(0)
    val = samplePoints(phi, nx, ny, nz, dx, lo, pts, order="linear", mask=mask, want_grad=False).val
    with np.errstate(invalid="ignore"):
        keep = (np.abs(val) >= rmin * dx) & (np.abs(val) <= band * dx)
    val = val[keep]
    return np.asfortranarray(pts[keep]), np.sign(val) * np.clip(np.abs(val), rmin * dx, rmax * dx)


class ReseedReport(NamedTuple):
    """What lsf_reseed_points and lsf_reseed_get return (include/lsf.h): the marker set `pts` (nout, 3; Fortran-ordered), `rad` (nout)
    and `src` (nout, int32: the 1-based position of a kept marker in the input, 0 for a new one), `status` of the INPUT markers (npts,
    int32: 0 KEPT, 1 OUTSIDE, 2 OFFBAND, 3 NONFINITE, 4 BADRADIUS, 5 FAR) and `info`, the fourteen counts [the six statuses, eligible
    cells, candidates, accepted, rejected before or during the attraction, rejected by the final test, cells with more than per_cell
    kept markers, the largest count, kept markers on the wrong side]."""
    pts: object
    rad: object
    src: object
    status: object
    info: tuple


def reseedParticles(phi, nx: int, ny: int, nz: int, dx: float, xLo, pts=None, rad=None, *, mask=None, per_cell: int = 16, rmin: float = 0.1,
                    rmax: float = 0.5, band: float = 3.0, order: str = "cubic", iters: int = 4, tol: float = 1e-3, seed: int = 0) -> ReseedReport:
    """The maintenance of the marker population on the device (include/lsf.h: lsf_reseed_points): the old markers (pts, rad) that are
    still usable -- inside the grid, on the band, within band * dx of the surface, with a sound radius -- are kept with their radius
    refreshed, every cell next to the surface that holds fewer than per_cell of them is topped up with new markers attracted to a
    random level between rmin * dx and band * dx on their own side, and one compacted set comes back: the kept markers in the
    caller's order, then the new ones.  Without pts and rad it seeds from scratch.

    Vary `seed` from reseed to reseed (the step number will do): the same seed redraws the same offsets in a cell.  Over-full cells
    are reported (info[11], info[12]) and left alone.  Numpy in gives numpy out (host seam); CUDA tensors in give CUDA tensors out
    (device seam, on the tensor's current stream).
    """
    lo, dx = _seam.xlo(xLo), _seam.positive(dx)
    _seam.grid(nx, ny, nz)
    per_cell, iters, seed = int(per_cell), int(iters), int(seed)
    rmin, rmax, band, tol = float(rmin), float(rmax), float(band), float(tol)
    order = _seam.named("order", order, _SAMPLE_ORDERS)
    if not 1 <= per_cell <= _lib.LSF_RESEED_MAX_PER_CELL:
        raise ValueError(f"per_cell must be in 1..{_lib.LSF_RESEED_MAX_PER_CELL}")
    if not 1 <= iters <= _lib.LSF_RESEED_MAX_ITERS:
        raise ValueError(f"iters must be in 1..{_lib.LSF_RESEED_MAX_ITERS}")
    if not (np.isfinite(rmin) and np.isfinite(rmax) and np.isfinite(band) and 0.0 < rmin <= rmax and rmin < band):
        raise ValueError("0 < rmin <= rmax and rmin < band are required, all finite")
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0")
    if (pts is None) != (rad is None):
        raise ValueError("pts and rad are given together")
    if pts is not None and pts.shape[0] == 0:
        pts = rad = None
    s = Seam(phi, nx, ny, nz, "phi, mask, pts and rad", optional=(pts, rad, mask), check_device=False)
    npts = 0
    if pts is not None:
        npts = s.points(pts)
    s.one_device()
    if pts is not None:
        s.vector(rad, npts, "rad")
    p, m = s.field(phi, "phi"), s.optional(mask, "mask", np.int32)
    info = np.zeros(_lib.LSF_RESEED_INFO_LEN, dtype=np.int64)
    nout = ctypes.c_int(0)
    useed = ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF)
    status = s.out(npts, np.int32)
    _lib.check(s.call("lsf_reseed_points", p, m, nx, ny, nz, dx, lo.ctypes.data, s.ptr(pts), s.ptr(rad), npts, per_cell, rmin, rmax, band, order,
                      iters, tol, useed, s.ptr(status) if npts else None, ctypes.byref(nout), info.ctypes.data))
    n = nout.value
    out, orad, src = s.out3(n), s.out(n), s.out(n, np.int32)
    _lib.check(s.call("lsf_reseed_get", *((s.ptr(out), s.ptr(orad), s.ptr(src)) if n else (None, None, None))))
    return ReseedReport(out, orad, src, status, tuple(int(v) for v in info))


class SurfaceInfo(NamedTuple):
    """The counts of lsf_extract_surface (include/lsf.h: info[0..3])."""
    nodes: int
    triangles: int
    cells_crossed: int
    nodes_on_grid_points: int


def extractSurface(phi, nx: int, ny: int, nz: int, dx: float, xLo, *, iso: float = 0.0):
    """The level set phi = iso as an indexed triangle mesh (include/lsf.h: lsf_extract_surface): marching tetrahedra on the six Kuhn
    tetrahedra of every cell, one node per crossed edge, made on the device.  Returns (surfX, surfElem, SurfaceInfo).

    phi is an input (numpy F-ordered or torch CUDA, see module docstring); the grid point is xLo + i*dx as for meshDistance.
    surfX is (nSurfNode, 3) float64 and surfElem (nSurfElem, 3) int32, 1-based, both Fortran-ordered -- what meshCheck, meshDistance,
    phi0Init and stlWrite take.  Numpy in gives numpy out; a CUDA tensor in gives CUDA tensors out through the device seam, on the
    tensor's current stream.  Triangle normals point towards phi >= iso; the numbering is a function of the field alone.  A level set
    that reaches the walls of the grid gives an open mesh; an empty one gives arrays with 0 rows.
    """
    lo, dx, iso = _seam.xlo(xLo, finite=False), _seam.positive(dx), _seam.finite_iso(iso)
    _seam.grid(nx, ny, nz)
    s = Seam(phi, nx, ny, nz)
    nn, nt = ctypes.c_int(0), ctypes.c_int(0)
    info = np.zeros(_lib.LSF_SURF_INFO_LEN, dtype=np.int64)
    _lib.check(s.call("lsf_extract_surface", s.field(phi, "phi"), nx, ny, nz, dx, lo.ctypes.data, iso, ctypes.byref(nn), ctypes.byref(nt),
                      info.ctypes.data))
    sX, sE = s.out3(nn.value), s.out3(nt.value, np.int32)
    _lib.check(s.call("lsf_extract_get", s.ptr(sX) if nn.value else None, s.ptr(sE) if nt.value else None))
    return sX, sE, SurfaceInfo(*(int(v) for v in info))


def stlWrite(path, surfX, surfElem) -> None:
    """Binary STL from nodes + 1-based connectivity (include/lsf.h: lsf_stl_write): vertices rounded to float32, unit normals
    computed from the rounded vertices.  Host code only: no device is needed.  CUDA tensors are copied to the host first."""
    surfX, surfElem = (a.cpu().numpy() if _seam.is_torch(a) else a for a in (surfX, surfElem))
    sX, sE = _surface(surfX, surfElem)
    _lib.check(_lib.load().lsf_stl_write(os.fsencode(path), sX.ctypes.data, sX.shape[0], sE.ctypes.data, sE.shape[0]))


def advectNodes(phi, phiSB, nx: int, ny: int, nz: int, dx: float, xLo, surfXX, iter: int = 1000) -> None:
    """Order-8 gradients on the stencil band + surface-node advection, set3d.f90:470-501, as one call.

    surfXX: (nSurfNode,3) float64 numpy array (Fortran-ordered), the nodes on entry and the advected nodes on
    return (this is what the host writes to the .s3d file, set3d.f90:606-608).  phi / phiSB as for minmaxFlow.
    Bit-identical to the reference (including subs.f90:346's repeated j+1 neighbour).
    """
    if not (isinstance(surfXX, np.ndarray) and surfXX.dtype == np.float64 and surfXX.ndim == 2
            and surfXX.shape[1] == 3 and surfXX.flags.f_contiguous and surfXX.flags.writeable):
        raise ValueError("surfXX must be a writeable Fortran-ordered float64 array of shape (nSurfNode, 3)")
    lo = np.ascontiguousarray(xLo, dtype=np.float64)
    s = Seam(phi, nx, ny, nz)
    _lib.check(s.call("lsf_advect_nodes", s.field(phi, "phi"), s.field(phiSB, "phiSB", np.int32), nx, ny, nz, float(dx), lo.ctypes.data,
                      surfXX.ctypes.data, surfXX.shape[0], int(iter)))


TRANSPORTS = {"peer": _lib.LSF_TRANSPORT_PEER, "rccl": _lib.LSF_TRANSPORT_RCCL, "mock": _lib.LSF_TRANSPORT_MOCK}


def reinit_multi(phi, nx: int, ny: int, nz: int, iter: int, dx: float, h: float, devices, *, dims=None,
                 tol: float = REINIT_TOL, arith: str = "fast", check_every: int = 8, transport: str = "peer",
                 order: str = "jacobi") -> SweepReport:
    """reinit on every device of `devices` from ONE process (include/lsf.h: lsf_reinit_multi; the call site
    set3d.f90:308 for a host that wants all the GPUs of the node).  phi: Fortran-ordered numpy array, float64 or
    float32, updated in place.  order="jacobi": blocks with ghost layers, bit-identical to reinit(..., order="jacobi")
    on one device.  order="gs" (float64): the reference's in-place ordering (subs.f90:743-852) over z slabs, one per
    device, bit-identical to reinit(..., order="gs") and so, with arith="strict", to the reference; dims, check_every
    and transport do not apply.  A device may be named more than once (several blocks / slabs share it).
    check_every: sweeps between two looks at the RMS (the stop sweep, the field and the trace do not depend on it);
    transport: "peer" (peer copies), "rccl" (ncclSend / ncclRecv, a distinct device per block) or "mock" (test aid)."""
    lib = _lib.load()
    if transport not in TRANSPORTS:
        raise ValueError(f"transport must be one of {sorted(TRANSPORTS)}, not {transport!r}")
    if order not in ("jacobi", "gs"):
        raise ValueError(f"order must be 'jacobi' or 'gs', not {order!r}")
    if order == "gs" and (check_every != 8 or transport != "peer"):
        raise ValueError("order='gs' (the reference's ordering over z slabs) takes no check_every or transport")
    old_ce, old_tr = ctypes.c_int(8), ctypes.c_int(_lib.LSF_TRANSPORT_PEER)
    lib.lsf_multi_defaults_get(ctypes.byref(old_ce), ctypes.byref(old_tr))  # this thread's: put back afterwards
    _lib.check(lib.lsf_multi_defaults(int(check_every), TRANSPORTS[transport]))
    cap = int(iter) + 1
    trace = np.zeros(max(cap, 1), dtype=np.float64)
    done = ctypes.c_int(0)
    mode = mode_word(order, arith)
    devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
    dm = (ctypes.c_int * 3)(*[int(d) for d in dims]) if dims is not None else None
    f32 = isinstance(phi, np.ndarray) and phi.dtype == np.float32
    p = _seam.host_field(phi, "phi", np.float32 if f32 else np.float64, nx, ny, nz)  # a host call: the devices are named, not implied
    fn = lib.lsf_reinit_multi_f32 if f32 else lib.lsf_reinit_multi
    try:
        rc = fn(p, nx, ny, nz, int(iter), float(dx), float(h), float(tol), mode, devs, len(devices), dm, ctypes.byref(done),
                trace.ctypes.data, cap)
    finally:
        lib.lsf_multi_defaults(old_ce.value, old_tr.value)
    return _sweep_report(rc, done, trace, tol, 0, "", False)


def peer_selftest(dev_a: int, dev_b: int) -> int:
    """include/lsf.h: lsf_peer_selftest -- the litmus test of the device-to-device hand-offs the exact ordering across z slabs
    relies on.  Returns 0, or raises LsfError whose message names the violated assumption."""
    lib = _lib.load()
    bad = ctypes.c_int(0)
    _lib.check(lib.lsf_peer_selftest(int(dev_a), int(dev_b), ctypes.byref(bad)))
    return bad.value
