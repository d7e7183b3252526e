"""Inputs shared by the tests of lsf_reseed_points, and the statement's results on them (computed once per process, read-only)."""
from __future__ import annotations

import functools

import numpy as np

import points_ref as P
import reseed_ref as R
import sample_ref as S

# 20 x 18 x 16 cells; dx and xLo are binary fractions.  (The 12 x 9 x 7 grid of the other point tests is too small here: under the
# mask the cubic stencil leaves it for 40 % of the candidates.)
SHAPE, DX, LO = (21, 19, 17), 0.125, (-0.75, 0.25, 1.0)
RADIUS, OFF = 0.55, (0.03, 0.06, 0.09)
MAIN = dict(per_cell=8, rmin=0.1, rmax=0.5, band=1.5, iters=4, tol=1e-3)
NPTS = (0, 1, 63, 65, 2037)
FULL_CELL = (14, 9, 8)  # the planted over-full cell: MAIN["per_cell"] + 3 markers
NAN_AT, ZERO_AT = (6, 9, 8), (10, 14, 8)  # grid points next to the surface (|phi| < 0.4 dx there)


def grid_coords():
    ax = [LO[A] + np.arange(SHAPE[A]) * DX for A in range(3)]
    return np.meshgrid(*ax, indexing="ij")


def _sphere(shift=0.0):
    X, Y, Z = grid_coords()
    c = [LO[A] + 0.5 * (SHAPE[A] - 1) * DX + OFF[A] for A in range(3)]
    return np.sqrt((X - c[0] - shift) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - RADIUS


@functools.lru_cache(maxsize=None)
def fields(kind="sphere"):
    """(phi, mask): the sphere and the mask |phi| < 4.1 dx with holes 0, 7 and -1; kind "nan" plants a NaN and a -0.0 next to the
    surface, "flat" a constant patch across it."""
    phi = _sphere()
    mask = (np.abs(phi) < 4.1 * DX).astype(np.int32)
    mask[1, 1, 1], mask[19, 17, 15], mask[1, 17, 1] = 0, 7, -1  # the positions of points_inputs.py: off this band anyway
    mask[10, 17, 8], mask[18, 9, 8], mask[10, 9, 8] = 0, 7, -1  # ... and about 3.3 dx from the surface, where band = 3.0 meets them
    if kind == "nan":
        phi[NAN_AT], phi[ZERO_AT] = np.nan, -0.0
    elif kind == "flat":
        phi[14:18, 8:12, 7:11] = 0.25 * DX
    out = [np.asfortranarray(phi), np.asfortranarray(mask)]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def old_markers():
    """(pts, rad): markers by the statement's seed_particles on the sphere shifted by 0.8 dx (out to 2 dx from it, so that the band
    of 1.5 dx drops some as FAR), shuffled, and planted among them rad 0, NaN and +-inf, a FAR marker and an over-full cell (all
    below index 63, so that every truncation but npts = 1 holds them) and, from index 70, the special points of sample_ref (walls,
    one ulp beyond, NaN, +-inf, 1e300).  Read-only."""
    pts, rad = P.seed_particles(np.asfortranarray(_sphere(0.8 * DX)), DX, LO, per_cell=8, rmin=0.1, rmax=0.5, band=2.0, seed=3)
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(rad))  # (seed_particles emits cell after cell: a truncation would otherwise see one corner of the sphere)
    pts, rad = np.array(pts[perm]), rad[perm].copy()
    rad[5], rad[17], rad[29], rad[41] = 0.0, np.nan, np.inf, -np.inf
    sp = S.special_points(SHAPE, DX, LO)[0]
    pts[70:70 + len(sp)] = sp
    pts[2] = [LO[0] + 1.5 * DX, LO[1] + 1.5 * DX, LO[2] + 1.5 * DX]  # a corner of the grid: FAR
    for m in range(MAIN["per_cell"] + 3):  # the over-full cell, on the surface
        pts[44 + m] = [LO[A] + (FULL_CELL[A] + 0.1 + 0.07 * m) * DX for A in range(3)]
        rad[44 + m] = 0.2 * DX
    pts = np.asfortranarray(pts)
    pts.setflags(write=False)
    rad.setflags(write=False)
    return pts, rad


def markers(npts):
    pts, rad = old_markers()
    return (None, None) if npts == 0 else (np.asfortranarray(pts[:npts]), rad[:npts].copy())


@functools.lru_cache(maxsize=None)
def want(order, masked, npts, kind="sphere", seed=5, **kw):
    phi, mask = fields(kind)
    pts, rad = markers(npts)
    return R.reseed_points(phi, DX, LO, pts, rad, mask=mask if masked else None, order=order, seed=seed, **dict(MAIN, **kw))


# ------------------------------------------------------------------------------------- the vortex configuration, reseeded
VORTEX = dict(per_cell=16, rmin=0.1, rmax=0.5, band=3.0, order=R.CUBIC, iters=4, tol=1e-3)


@functools.lru_cache(maxsize=None)
def vortex_reseed_run(every=16):
    """points_inputs.vortex_run(True) with reseed_points after every `every`-th step (seed = the 1-based step number):
    dict(phi, pts, rad, infos (per step: advect info, correct info, reseed info or None))"""
    import advect_ref as A
    import points_inputs as PI

    phi0, vel = PI.vortex_fields()
    neg = tuple(np.asfortranarray(-a) for a in vel)
    phi = phi0.copy(order="F")
    pts, rad = P.seed_particles(phi0, PI.VDX, PI.VLO)
    infos = []
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(2 * PI.VSTEPS):
            V = vel if n < PI.VSTEPS else neg
            phi = A.step(phi, V, None, PI.VDX, PI.VDT)
            a = P.advect_points(pts, PI.VDX, PI.VLO, PI.VDT, 1, velocity=V, order=P.CUBIC, scheme=P.RK3)
            pts = a.pts
            c = P.correct_field(phi, PI.VDX, PI.VLO, pts, rad)
            phi = c.phi
            r = None
            if (n + 1) % every == 0:
                r = R.reseed_points(phi, PI.VDX, PI.VLO, pts, rad, seed=n + 1, **VORTEX)
                pts, rad = r.pts, r.rad
            infos.append((tuple(a.info), tuple(c.info), None if r is None else tuple(r.info)))
    phi.setflags(write=False)
    return dict(phi=phi, pts=pts, rad=rad, infos=infos)
