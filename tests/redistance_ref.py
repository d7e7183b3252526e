"""Serial restatement of lsf_redistance_band (include/lsf_redistance.h): closest-point redistancing of a cell list.

    LIST     the interior points (1..n-1 on each axis) with mask == 1 (advect_band_ref.list_of)
    FOOT     every list cell as the point (i*dx, j*dx, k*dx) of the grid with xLo = 0, sampled and projected by
             sample_ref.sample_points: CUBIC, the call's mask as the band, iso = 0, iters, tol.  dist = |x - foot|;
             FROZEN = status OK and dist < near*dx;  s = -1 where phi < 0 on entry, else +1
    FILL     magnitudes u = dist at frozen cells, +inf elsewhere; Jacobi passes of distance_fill_ref's visit over the non-frozen
             list cells, on whole arrays, every pass reading u as it was at its start.  Only list cells ever hold a finite u, so
             a neighbour that is not in the list counts as +inf by itself.
    RESULT   frozen: s*dist (dist == 0.0: the value on entry); reached: s*u; still +inf: the value on entry, counted

Every expression is evaluated as the header writes it, left to right, element by element on float64 arrays (numpy fuses nothing;
sqrt and / are IEEE), so the library's field, passes, trace, change and info are compared with `==`.  The arguments are left alone.
phi off the list is never read: the statement works on a copy in which every point off the list has been REPLACED BY A POISON VALUE
and put back at the end, so a result that equals the library's proves that neither reads it there.

Also here: the inputs the tests share.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple

import numpy as np

import sample_ref as S
from advect_band_ref import list_of

POISON = -1.2345e300  # what the statement sees off the list instead of the caller's phi
INFO_LEN = 9


class Invalid(ValueError):
    """LSF_ERR_INVALID"""


class RedistanceResult(NamedTuple):
    field: np.ndarray
    passes: int
    trace: List[int]
    change: float
    info: List[int]
    status: np.ndarray  # per list cell, in np.argwhere(LIST) order
    dist: np.ndarray  # |x - foot| per list cell, NaN where there is no foot
    frozen: np.ndarray  # boolean field


def visit(x, y, z, dx):
    """distance_fill_ref's update from the smaller neighbour magnitude of each axis, on arrays; meaningful where min(x, y, z) < inf"""
    dx2 = dx * dx
    with np.errstate(invalid="ignore"):
        a = np.minimum(np.minimum(x, y), z)
        c = np.maximum(np.maximum(x, y), z)
        b = np.maximum(np.minimum(x, y), np.minimum(np.maximum(x, y), z))
        t = a + dx
        two = t > b
        dd = a - b
        t2 = ((a + b) + np.sqrt(2 * dx2 - dd * dd)) * 0.5
        t = np.where(two, t2, t)
        three = two & (t > c)
        s3 = ((a - b) * (a - b) + (a - c) * (a - c)) + (b - c) * (b - c)
        t3 = (((a + b) + c) + np.sqrt(np.maximum(3 * dx2 - s3, 0))) / 3
        return np.where(three, t3, t)


def feet(phi, mask, dx, iters, tol):
    """(cells (nL, 3), status, dist) of the list cells in np.argwhere order; dist is NaN where the sample gave no foot"""
    lst = list_of(mask)
    at = np.argwhere(lst)
    pts = np.asfortranarray(at.astype(np.float64) * np.float64(dx))  # ((double)i*dx, (double)j*dx, (double)k*dx)
    r = S.sample_points(phi, dx, (0.0, 0.0, 0.0), pts, order=S.CUBIC, mask=np.asarray(mask), iso=0.0, iters=iters, tol=tol)
    with np.errstate(invalid="ignore"):
        d0, d1, d2 = pts[:, 0] - r.foot[:, 0], pts[:, 1] - r.foot[:, 1], pts[:, 2] - r.foot[:, 2]
        dist = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
    return at, r.status, dist


def redistance_band(phi, mask, dx, near=2.5, iters=8, tol=1e-9, max_passes=64) -> RedistanceResult:
    """lsf_redistance_band.  phi, mask: (nx+1, ny+1, nz+1)."""
    phi_in = np.asarray(phi, dtype=np.float64)
    dx, near, tol = np.float64(dx), np.float64(near), float(tol)
    if phi_in.ndim != 3 or min(phi_in.shape) < 3 or phi_in.size > 2 ** 31 - 1:
        raise Invalid("dimensions")
    if not (np.isfinite(dx) and dx > 0) or not (np.isfinite(near) and near > 0) or iters < 1 or not (np.isfinite(tol) and tol >= 0) or max_passes < 1:
        raise Invalid("dx, near, iters, tol or max_passes")
    lst = list_of(mask)
    if not lst.any():
        raise Invalid("the list is empty")
    bad = int((lst & ~np.isfinite(phi_in)).sum())
    if bad:
        raise Invalid(f"{bad} list cell(s) hold a non-finite phi")
    work = np.where(lst, phi_in, POISON)
    at, status, dist = feet(work, mask, dx, iters, tol)
    own = tuple(at.T)
    near_dx = near * dx  # computed once
    with np.errstate(invalid="ignore"):
        fz = (status == S.OK) & (dist < near_dx)
    if not fz.any():
        raise Invalid("no frozen cell")
    old = work[own]
    sgn = np.where(old < 0, -1.0, 1.0)

    U = np.full(tuple(s + 2 for s in work.shape), np.inf)  # a ring of +inf; a point off the list never leaves +inf either
    pad = tuple(c + 1 for c in own)
    U[pad] = np.where(fz, dist, np.inf)
    live = tuple(c[~fz] for c in pad)
    nbr = []
    for a in range(3):
        lo, hi = list(live), list(live)
        lo[a], hi[a] = live[a] - 1, live[a] + 1
        nbr.append((tuple(lo), tuple(hi)))
    trace = []
    while len(trace) < max_passes:
        x, y, z = (np.minimum(U[lo], U[hi]) for lo, hi in nbr)  # u as it was at the start of the pass
        t = visit(x, y, z, dx)
        low = (np.minimum(np.minimum(x, y), z) < np.inf) & (t < U[live])
        U[tuple(c[low] for c in live)] = t[low]
        trace.append(int(low.sum()))
        if trace[-1] == 0:
            break

    u = U[pad]
    reached = ~fz & (u < np.inf)
    unreached = ~fz & ~reached
    new = np.where(fz, np.where(dist == 0.0, old, sgn * np.where(fz, dist, 0.0)), np.where(reached, sgn * np.where(reached, u, 0.0), old))
    change = float(np.abs(new - old).max())
    out = np.array(phi_in, copy=True, order="K")
    out[own] = new
    frozen = np.zeros(work.shape, bool)
    frozen[own] = fz
    count = lambda st: int(np.count_nonzero(status == st))
    info = [int(lst.sum()), int(fz.sum()), int(reached.sum()), int(unreached.sum()), count(S.OFFBAND), count(S.OUTSIDE), count(S.FLAT),
            count(S.NOT_CONVERGED), int(((status == S.OK) & ~fz).sum())]
    return RedistanceResult(out, len(trace), trace, change, info, status, dist, frozen)


# ------------------------------------------------------------------------------------------------ the inputs the tests share
CENTRE, RADIUS, HALF = (0.013, -0.021, 0.034), 0.8, 1.5  # the sphere of the accuracy table: centre off the lattice, box [-HALF, HALF]^3
DISTORTIONS = {"exact": lambda x, y, z: 1.0 + 0.0 * x,
               "mild": lambda x, y, z: 1.0 + 0.1 * x + 0.05 * np.sin(3.0 * z),
               "strong": lambda x, y, z: 1.0 + 0.3 * x + 0.2 * y * y + 0.25 * np.sin(3.0 * z)}
SETTINGS = dict(near=2.5, iters=8, tol=1e-9, max_passes=64)
WIDTH = 8.1  # the mask of the accuracy table, |d| < WIDTH * dx


@functools.lru_cache(maxsize=None)
def sphere_case(n, kind):
    """(phi, mask, dx, d): phi = d * g on n^3 points, d = r - RADIUS the exact distance, the mask |d| < WIDTH*dx; read-only"""
    dx = 2.0 * HALF / (n - 1)
    ax = -HALF + dx * np.arange(n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2) - RADIUS
    phi = np.asfortranarray(d * DISTORTIONS[kind](x, y, z))
    mask = np.asfortranarray((np.abs(d) < WIDTH * dx).astype(np.int32))
    for a in (phi, mask, d):
        a.setflags(write=False)
    return phi, mask, dx, d


@functools.lru_cache(maxsize=None)
def sphere_want(n, kind):
    phi, mask, dx, _ = sphere_case(n, kind)
    r = redistance_band(phi, mask, dx, **SETTINGS)
    r.field.setflags(write=False)
    return r


def errors(n, kind):
    """(largest error in dx over the list cells with |d| < 1.5 dx, over the frozen cells, over the whole list) of sphere_want"""
    phi, mask, dx, d = sphere_case(n, kind)
    r = sphere_want(n, kind)
    lst = list_of(mask)
    e = np.abs(r.field - d) / dx
    return float(e[lst & (np.abs(d) < 1.5 * dx)].max()), float(e[r.frozen].max()), float(e[lst].max())
