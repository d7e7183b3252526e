"""Inputs shared by the tests of lsf_advect_points and lsf_correct_field, and the statement's own run of the vortex configuration
(computed once per process and left unchanged)."""
from __future__ import annotations

import functools

import numpy as np

import points_ref as P
import sample_ref as S

# ------------------------------------------------------------------------------------- the small grid of test_gpu_sample_points.py
SHAPE, DX, LO = (13, 10, 8), 0.125, (-0.75, 0.25, 1.0)  # 12 x 9 x 7 cells; dx and xLo are binary fractions
CENTRE, RADIUS = (0.0, 0.8125, 1.4375), 0.25


def grid_coords(shape=SHAPE, dx=DX, lo=LO):
    ax = [lo[A] + np.arange(shape[A]) * dx for A in range(3)]
    return np.meshgrid(*ax, indexing="ij")


@functools.lru_cache(maxsize=None)
def small_fields():
    """(phi, u, v, w, speed, mask): a sphere distance, smooth fields with |.| <= 1, and a mask of 1s (walls included) with holes 0, 7
    and -1.  Read-only."""
    X, Y, Z = grid_coords()
    phi = np.sqrt((X - CENTRE[0]) ** 2 + (Y - CENTRE[1]) ** 2 + (Z - CENTRE[2]) ** 2) - RADIUS
    # |u|, |v|, |w| <= 0.6 and |speed| <= 0.4: |k_A| <= 1 on every axis with both groups present
    u = 0.6 * np.sin(1.7 * Y + 0.4) * np.cos(0.9 * Z)
    v = 0.6 * np.cos(1.3 * X - 0.2) * np.sin(1.1 * Z + 0.5)
    w = 0.6 * np.sin(0.8 * X + 1.9 * Y)
    f = 0.4 * np.cos(1.5 * X + 0.7 * Y - 0.9 * Z)
    mask = np.ones(SHAPE, np.int32)
    mask[1, 1, 1], mask[11, 8, 6], mask[1, 8, 1] = 0, 7, -1  # (near the corners: on so small a grid a hole in the middle empties it)
    out = [np.asfortranarray(a) for a in (phi, u, v, w, f, mask)]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def draw_points(npts, masked, seed=0):
    """npts points.  Under a mask all are drawn with i0 in 3 .. n-4: they move at most 1.2 dx from a margin of 3 cells.  Without one
    they come from anywhere in the grid, the cells next to the walls included -- but a point within 1.2 dx of a wall may walk out, and
    with every point drawn so a fifth of them does (measured on the statement), so eleven in twelve are kept 1.25 cells clear of the
    walls and the twelfth falls anywhere.  From the 71st on one in fourteen is a special point of sample_ref (walls, one ulp beyond,
    NaN, +-inf, 1e300).  (npts, 3) in Fortran order, read-only."""
    rng = np.random.default_rng(seed + 7 * npts + (1000 if masked else 0))
    n = [s - 1 for s in SHAPE]
    pts = np.empty((npts, 3))
    free = rng.random(npts) < 1.0 / 12.0
    for A in range(3):
        a, b = (3.0, n[A] - 3.0) if masked else (1.25, n[A] - 1.25)
        pts[:, A] = LO[A] + (a + (b - a) * rng.random(npts)) * DX
        if not masked:
            pts[free, A] = LO[A] + (n[A] * rng.random(npts) * DX)[free]
    sp = S.special_points(SHAPE, DX, LO)[0]
    for m, t in enumerate(range(70, npts, 14)):
        pts[t] = sp[m % len(sp)]
    pts = np.asfortranarray(pts)
    pts.setflags(write=False)
    return pts


# the cases of tests/test_gpu_advect_points.py: all 12 instances x both schemes, with npts, the sign of dt and nsteps cycling through them
NPTS = (1, 63, 65, 256, 2037)
INSTANCES = [(o, g, m) for o in (P.LINEAR, P.CUBIC) for g in ("vel", "speed", "both") for m in (False, True)]


def advect_cases():
    out = []
    for c, ((order, group, masked), scheme) in enumerate((i, s) for i in INSTANCES for s in (P.RK3, P.EULER)):
        out.append(dict(order=order, group=group, masked=masked, scheme=scheme, npts=NPTS[c % 5], dt=(0.4 if (c // 3) % 2 == 0 else -0.4) * DX,
                        nsteps=(1, 3)[(c // 4 + c // 2 + c) % 2]))
    return out


def advect_args(case):
    """the keyword arguments of points_ref.advect_points for a case (fields shared, read-only)"""
    phi, u, v, w, f, mask = small_fields()
    g = case["group"]
    return dict(velocity=(u, v, w) if g in ("vel", "both") else None, speed=f if g in ("speed", "both") else None,
                phi=phi if g in ("speed", "both") else None, mask=mask if case["masked"] else None, order=case["order"], scheme=case["scheme"])


@functools.lru_cache(maxsize=None)
def advect_want(c):
    case = advect_cases()[c]
    return P.advect_points(draw_points(case["npts"], case["masked"]), DX, LO, case["dt"], case["nsteps"], **advect_args(case))


# the inputs of tests/test_gpu_correct_field.py
NAN_AT, ZERO_AT = (8, 4, 3), (9, 7, 5)  # a NaN next to the surface; -0.0 at a point that a candidate of +0.0 reaches


@functools.lru_cache(maxsize=None)
def correct_inputs():
    """(phi, pts, rad): the sphere field with a NaN at one grid point and -0.0 at another; markers seeded by the statement's rule from
    the sphere shifted by 0.8 dx along x, then the planted ones: rad 0, NaN and inf, the special points of sample_ref, and the marker
    half a cell from the -0.0 with rad = dx / 2, whose candidate there is +0.0 exactly.  Read-only."""
    X, Y, Z = grid_coords()
    phi = np.array(small_fields()[0], order="F")
    shifted = np.asfortranarray(np.sqrt((X - CENTRE[0] - 0.8 * DX) ** 2 + (Y - CENTRE[1]) ** 2 + (Z - CENTRE[2]) ** 2) - RADIUS)
    pts, rad = P.seed_particles(shifted, DX, LO, per_cell=8, rmin=0.05, rmax=0.1, band=1.5, seed=3)  # (close to the surface, small radii: enough escape)
    pts, rad = np.array(pts), rad.copy()
    rad[5], rad[17], rad[29], rad[41] = 0.0, np.nan, np.inf, -np.inf
    sp = S.special_points(SHAPE, DX, LO)[0]
    pts[100:100 + len(sp)] = sp
    i, j, k = ZERO_AT
    phi[i, j, k], phi[i + 1, j, k] = -0.0, -0.5
    phi[NAN_AT] = np.nan
    pts[60] = [LO[0] + (i + 0.5) * DX, LO[1] + j * DX, LO[2] + k * DX]
    rad[60] = 0.5 * DX
    pts = np.asfortranarray(pts)
    for a in (phi, pts, rad):
        a.setflags(write=False)
    return phi, pts, rad


@functools.lru_cache(maxsize=None)
def correct_want(masked, slack):
    phi, pts, rad = correct_inputs()
    return P.correct_field(phi, DX, LO, pts, rad, mask=small_fields()[5] if masked else None, slack=slack)


# ------------------------------------------------------------------------------------- the vortex configuration
VN = 33
VDX = 1.0 / (VN - 1)
VLO = (0.0, 0.0, 0.0)
VDT = VDX / 4
VSTEPS = 64  # forward, then as many with the velocity negated


@functools.lru_cache(maxsize=None)
def vortex_fields():
    """(phi0, (u, v, w)): the sphere of radius 0.15 at (0.35, 0.35, 0.35) and LeVeque's deformation field on 33^3 points"""
    X, Y, Z = grid_coords((VN,) * 3, VDX, VLO)
    pi = np.pi
    u = 2. * np.sin(pi * X) ** 2 * np.sin(2 * pi * Y) * np.sin(2 * pi * Z)
    v = -np.sin(2 * pi * X) * np.sin(pi * Y) ** 2 * np.sin(2 * pi * Z)
    w = -np.sin(2 * pi * X) * np.sin(2 * pi * Y) * np.sin(pi * Z) ** 2
    phi0 = np.sqrt((X - 0.35) ** 2 + (Y - 0.35) ** 2 + (Z - 0.35) ** 2) - 0.15
    out = [np.asfortranarray(a) for a in (phi0, u, v, w)]
    for a in out:
        a.setflags(write=False)
    return out[0], tuple(out[1:])


def volume(phi):
    """the volume of phi < 0 by the statement of lsf_measure_band on the whole interior"""
    import measure_ref as M

    return float(M.measure_band(phi, np.ones(phi.shape, np.int32), VDX, VLO).M[1])


def band_error(phi, phi0):
    near = np.abs(phi0) < 1.5 * VDX
    return float(np.mean(np.abs(phi - phi0)[near])) / VDX


@functools.lru_cache(maxsize=None)
def vortex_run(markers: bool, defect=None):
    """The statement's loop: 128 x (advect_ref.step; advect_points, one cubic RK3 step; correct_field), the velocity negated after 64.
    Returns dict(phi, pts, rad, infos (per step: advect info, correct info), escapes)."""
    import advect_ref as A

    phi0, vel = vortex_fields()
    neg = tuple(np.asfortranarray(-a) for a in vel)
    phi = phi0.copy(order="F")
    pts = rad = None
    if markers:
        pts, rad = P.seed_particles(phi0, VDX, VLO)
    infos, escapes = [], 0
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(2 * VSTEPS):
            V = vel if n < VSTEPS else neg
            phi = A.step(phi, V, None, VDX, VDT)
            if markers:
                a = P.advect_points(pts, VDX, VLO, VDT, 1, velocity=V, order=P.CUBIC, scheme=P.RK3, defect=defect)
                pts = a.pts
                c = P.correct_field(phi, VDX, VLO, pts, rad, defect=defect)
                phi = c.phi
                infos.append((tuple(a.info), tuple(c.info)))
                escapes += c.info[1]
    phi.setflags(write=False)
    return dict(phi=phi, pts=pts, rad=rad, infos=infos, escapes=escapes)
