"""lsf_sample_points restated in numpy: the statement of the contract in include/lsf.h, vectorised over the points.

    locate    per axis s = (x - xLo) / dx; INSIDE is s >= 0 && s <= n, decided in double before any integer is made;
              i0 = min(floor(s), n - 1), t = s - i0.
    stencil   cubic (Catmull-Rom, 4 x 4 x 4 at i0 - 1 .. i0 + 2) where 1 <= i0 <= n - 2 on all three axes, the 2 x 2 x 2 corners
              of the cell otherwise and always for LINEAR.
    band      with a mask every stencil point must be an interior point with mask == 1, else OFFBAND.
    value     contracted along x, then y, then z, each as ((w0*a0 + w1*a1) + w2*a2) + w3*a3; grad[A] the same with the derivative
              weights on axis A, divided by dx at the end.
    foot      Newton steps along the interpolant's gradient onto phi = iso, both signs.

Every expression is evaluated as the header writes it, left to right, element by element on float64 arrays (numpy never contracts
and no dot / einsum enters), so the library's result is compared with `==` on the bit patterns.  The arguments are left alone.

`defect` switches ONE deliberate error on (tests/test_sample_points_cpu.py shows each of them failing a test of the statement).
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

LINEAR, CUBIC = 0, 1
OK, OUTSIDE, OFFBAND, FLAT, NOT_CONVERGED = 0, 1, 2, 3, 4
INFO_LEN = 6
DEFECTS = ("swap_w1_w2", "d_is_w_on_y", "y_before_x", "no_min")


class SampleResult(NamedTuple):
    val: np.ndarray
    grad: np.ndarray  # (npts, 3), Fortran order
    qval: Optional[np.ndarray]
    foot: Optional[np.ndarray]  # (npts, 3), Fortran order
    status: np.ndarray  # int32
    info: list


class Invalid(ValueError):
    """LSF_ERR_INVALID"""


def weights(t, cubic, defect=None):
    """(w, d): the value and derivative weights of the header at offsets t, lists of arrays"""
    if cubic:
        w = [0.5 * (((2. - t) * t - 1.) * t), 0.5 * ((3. * t - 5.) * t * t + 2.), 0.5 * (((4. - 3. * t) * t + 1.) * t), 0.5 * ((t - 1.) * t * t)]
        d = [0.5 * ((4. - 3. * t) * t - 1.), 0.5 * ((9. * t - 10.) * t), 0.5 * ((8. - 9. * t) * t + 1.), 0.5 * ((3. * t - 2.) * t)]
        if defect == "swap_w1_w2":
            w[1], w[2] = w[2], w[1]
    else:
        w = [1. - t, t]
        d = [np.full(t.shape, -1.), np.full(t.shape, 1.)]
        if defect == "swap_w1_w2":
            w[0], w[1] = w[1], w[0]
    return w, d


def _contract(w, a):
    """((w0*a0 + w1*a1) + w2*a2) + w3*a3, or w0*a0 + w1*a1"""
    r = w[0] * a[0] + w[1] * a[1]
    for m in range(2, len(w)):
        r = r + w[m] * a[m]
    return r


def locate(pts, shape, dx, xLo, defect=None):
    """(inside, i0, t): i0 and t are (npts, 3), meaningful where inside"""
    npts = pts.shape[0]
    inside = np.ones(npts, bool)
    i0 = np.zeros((npts, 3), np.int64)
    t = np.zeros((npts, 3))
    with np.errstate(all="ignore"):
        for A in range(3):
            n = shape[A] - 1
            s = (pts[:, A] - xLo[A]) / dx
            ok = (s >= 0.) & (s <= float(n))  # in double, before any integer is made: NaN, inf and 1e300 fail it
            inside &= ok
            f = np.floor(np.where(ok, s, 0.)).astype(np.int64)
            i0[:, A] = f if defect == "no_min" else np.minimum(f, n - 1)
            t[:, A] = s - i0[:, A].astype(np.float64)
    return inside, i0, t


def _sample_group(field, i0, t, cubic, dx, want_grad, defect):
    """value (and gradient) of `field` at located points that all use one stencil; i0 (m,3), t (m,3)"""
    K = 4 if cubic else 2
    off = -1 if cubic else 0
    wd = [weights(t[:, A], cubic, defect) for A in range(3)]
    (wx, dx_), (wy, dy_), (wz, dz_) = wd
    if defect == "d_is_w_on_y":
        dy_ = wy
    ix = [i0[:, 0] + off + a for a in range(K)]
    iy = [i0[:, 1] + off + b for b in range(K)]
    iz = [i0[:, 2] + off + c for c in range(K)]
    if defect == "no_min":  # (the wild index of the defect is kept inside the array so that the test sees values, not a crash)
        ix = [np.minimum(v, field.shape[0] - 1) for v in ix]
        iy = [np.minimum(v, field.shape[1] - 1) for v in iy]
        iz = [np.minimum(v, field.shape[2] - 1) for v in iz]
    p, px, py = [], [], []
    with np.errstate(all="ignore"):
        for c in range(K):
            r, rd = [], []
            for b in range(K):
                a = [field[ix[m], iy[b], iz[c]] for m in range(K)]
                if defect == "y_before_x":  # the row runs along y, the rows are combined along x
                    a = [field[ix[b], iy[m], iz[c]] for m in range(K)]
                    r.append(_contract(wy, a))
                    if want_grad:
                        rd.append(_contract(dy_, a))
                    continue
                r.append(_contract(wx, a))
                if want_grad:
                    rd.append(_contract(dx_, a))
            if defect == "y_before_x":
                p.append(_contract(wx, r))
                if want_grad:
                    px.append(_contract(dx_, r))
                    py.append(_contract(wx, rd))
                continue
            p.append(_contract(wy, r))
            if want_grad:
                px.append(_contract(wy, rd))
                py.append(_contract(dy_, r))
        v = _contract(wz, p)
        if not want_grad:
            return v, None
        g = np.empty((len(v), 3))
        g[:, 0] = _contract(wz, px) / dx
        g[:, 1] = _contract(wz, py) / dx
        g[:, 2] = _contract(dz_, p) / dx
    return v, g


def _in_band(mask, i0, cubic):
    """every stencil point an interior point with mask == 1 (the LIST rule of lsf_reinit_band)"""
    K = 4 if cubic else 2
    off = -1 if cubic else 0
    ok = np.ones(i0.shape[0], bool)
    for A in range(3):
        lo, hi = i0[:, A] + off, i0[:, A] + off + K - 1
        ok &= (lo >= 1) & (hi <= mask.shape[A] - 2)
    for c in range(K):
        for b in range(K):
            for a in range(K):
                ok &= mask[i0[:, 0] + off + a, i0[:, 1] + off + b, i0[:, 2] + off + c] == 1
    return ok


def sample_once(phi, mask, q, dx, xLo, pts, order, defect=None):
    """One sample of every point by the rules of the header: (status, val, grad, qval, fallback).  status is OK, OUTSIDE or OFFBAND;
    val, grad and qval are NaN where it is not OK; fallback marks the sampled points of a cubic request served linearly."""
    npts = pts.shape[0]
    status = np.full(npts, OK, np.int32)
    val = np.full(npts, np.nan)
    grad = np.full((npts, 3), np.nan)
    qval = np.full(npts, np.nan) if q is not None else None
    inside, i0, t = locate(pts, phi.shape, dx, xLo, defect)
    status[~inside] = OUTSIDE
    cub = np.zeros(npts, bool)
    if order == CUBIC:
        cub = inside.copy()
        for A in range(3):
            cub &= (i0[:, A] >= 1) & (i0[:, A] <= phi.shape[A] - 3)  # 1 <= i0 <= n - 2 on all three axes
    for cubic in (False, True):
        sel = np.flatnonzero(inside & (cub == cubic))
        if mask is not None and sel.size:
            ok = _in_band(mask, i0[sel], cubic)
            status[sel[~ok]] = OFFBAND
            sel = sel[ok]
        if not sel.size:
            continue
        v, g = _sample_group(phi, i0[sel], t[sel], cubic, dx, True, defect)
        val[sel], grad[sel] = v, g
        if q is not None:
            qval[sel] = _sample_group(q, i0[sel], t[sel], cubic, dx, False, defect)[0]
    fallback = (status == OK) & ~cub if order == CUBIC else np.zeros(npts, bool)
    return status, val, grad, qval, fallback


def sample_points(phi, dx, xLo, pts, order=CUBIC, mask=None, q=None, iso=0.0, iters=0, tol=1e-6, defect=None) -> SampleResult:
    """lsf_sample_points.  phi, mask, q: (nx+1, ny+1, nz+1); pts: (npts, 3).  foot is None for iters == 0, qval without q."""
    phi = np.asarray(phi, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    xLo = np.asarray(xLo, dtype=np.float64)
    dx, iso, tol = float(dx), float(iso), float(tol)
    if phi.ndim != 3 or min(phi.shape) < 2 or phi.size > 2 ** 31 - 1:
        raise Invalid("dimensions")
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise Invalid("npts < 1")
    if not (np.isfinite(dx) and dx > 0.) or xLo.shape != (3,) or not np.all(np.isfinite(xLo)) or not np.isfinite(iso):
        raise Invalid("dx, xLo or iso")
    if order not in (LINEAR, CUBIC) or iters < 0 or (iters >= 1 and not (np.isfinite(tol) and tol >= 0.)):
        raise Invalid("order, iters or tol")
    if q is not None:
        q = np.asarray(q, dtype=np.float64)
    npts = pts.shape[0]
    status, val, grad, qval, fallback = sample_once(phi, mask, q, dx, xLo, pts, order, defect)
    foot = None
    if iters >= 1:
        foot = np.full((npts, 3), np.nan)
        act = np.flatnonzero(status == OK)  # points still moving
        y = pts[act].copy()
        tol_dx = tol * dx
        with np.errstate(all="ignore"):
            for it in range(iters + 1):  # `iters` moves, and one more sample for the convergence test after the last
                if not act.size:
                    break
                st, v, g, _, _ = sample_once(phi, mask, None, dx, xLo, y, order, defect)
                gone = st != OK
                status[act[gone]] = st[gone]
                e = v - iso
                conv = ~gone & ~(np.abs(e) > tol_dx)
                if it == iters:
                    status[act[~gone & ~conv]] = NOT_CONVERGED
                    foot[act] = y
                    break
                m = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
                flat = ~gone & ~conv & (m == 0.)
                status[act[flat]] = FLAT
                move = ~gone & ~conv & ~flat
                done = ~move
                foot[act[done]] = y[done]
                ynew = y[move] - (e[move, None] * g[move]) / m[move, None]
                act, y = act[move], ynew
    info = [int(np.count_nonzero(status == OK)), int(np.count_nonzero(status == OUTSIDE)), int(np.count_nonzero(status == OFFBAND)),
            int(np.count_nonzero(fallback)), int(np.count_nonzero(status == FLAT)), int(np.count_nonzero(status == NOT_CONVERGED))]
    return SampleResult(val, np.asfortranarray(grad), qval, None if foot is None else np.asfortranarray(foot), status, info)


# ---------------------------------------------------------------------------------- inputs shared by the tests
def special_points(shape, dx, lo):
    """(points, expected status of a maskless sample): just below the lower wall, exactly on the upper wall, one ulp above it, NaN,
    +inf, -inf and 1e300 on each axis in turn, the other coordinates in the middle of the grid"""
    pts, want = [], []
    mid = [lo[A] + 0.5 * (shape[A] - 1) * dx for A in range(3)]
    for A in range(3):
        n = shape[A] - 1
        for s, st in ((-1e-12, OUTSIDE), (float(n), OK), (n * (1 + 2.0 ** -52), OUTSIDE), (float("nan"), OUTSIDE), (float("inf"), OUTSIDE),
                      (float("-inf"), OUTSIDE), (1e300, OUTSIDE), (0.0, OK)):
            p = list(mid)
            p[A] = lo[A] + s * dx
            if s > n and not (p[A] - lo[A]) / dx > n:  # the coordinate rounded onto the wall: the next double is beyond it
                p[A] = float(np.nextafter(p[A], np.inf))
            pts.append(p)
            want.append(st)
    return np.array(pts), np.array(want, np.int32)


def ring_points(phi, mask, dx, lo):
    """(points, status of a cubic sample under the mask): a handful of points in cells whose eight corners are all on the list while a
    point of the outer ring of their 4 x 4 x 4 stencil is not -- OFFBAND by the ring alone -- and, beside each, a point in a
    neighbouring cell whose whole stencil is on the list.  The cells come from the mask itself: a hole next to the lower corner of
    the interior (mask[1, 1, 1] != 1) gives one.  Asserts that the statement reports at least one point of each kind."""
    shape, lo = phi.shape, np.asarray(lo, dtype=np.float64)
    listed = np.zeros(shape, bool)
    listed[1:-1, 1:-1, 1:-1] = mask[1:-1, 1:-1, 1:-1] == 1
    pts = []
    for i in range(2, shape[0] - 3):
        for j in range(2, shape[1] - 3):
            for k in range(2, shape[2] - 3):  # the cubic stencil is taken and lies in the interior: the mask's values decide
                corners, stencil = listed[i:i + 2, j:j + 2, k:k + 2].all(), listed[i - 1:i + 3, j - 1:j + 3, k - 1:k + 3].all()
                if corners and not stencil:
                    pts.extend(lo + (np.array([i, j, k]) + f) * dx for f in ((0.5, 0.5, 0.5), (0.0, 0.25, 0.875), (0.75, 0.125, 0.0)))
                    pts.extend(lo + (np.array([i + a, j + b, k + c]) + 0.5) * dx for a, b, c in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))
    pts = np.asfortranarray(np.array(pts))
    want = sample_points(phi, dx, lo, pts, order=CUBIC, mask=mask)
    ring_only = want.status == OFFBAND
    assert ring_only.any() and (want.status == OK).any(), want.info
    assert np.array_equal(sample_points(phi, dx, lo, pts[ring_only], order=LINEAR, mask=mask).status, np.zeros(ring_only.sum(), np.int32))
    return pts, want


def node_value_bound(phi, dx, xLo, X):
    """How far from iso the LINEAR sample at each node of lsf_extract_surface may lie, derived and not measured: (bound per node,
    whether the node lies on an edge along a grid axis).

    A node on an edge along axis A sits at x_A = fl(xLo + fl(fl(i + t) * dx)), t = fa / (fa - fb), where the trilinear interpolant
    along the edge is fa + t (fb - fa) = iso exactly.  Three roundings form x and two recover s = fl(fl(x - xLo) / dx), each half an
    ulp of a quantity no larger than |xLo| + |x|: per axis |s - (i + t)| <= 2.5 * 2^-52 * (|xLo| + |x|) / dx, rounded up to 4.  The
    interpolant changes by at most D = max|difference of adjacent grid values| per unit of s on each axis, and evaluating it (t, the
    weights, 7 products and sums) costs no more than 16 * 2^-52 * max|phi|:
        rounding = sum over the axes of 4 * 2^-52 * (|xLo| + max|x|) / dx * D  +  16 * 2^-52 * max|phi|.
    The Kuhn tetrahedra also cross the face and body diagonals of a cell, where the node is placed linearly but the trilinear
    interpolant is not linear: along the body diagonal it is c0 + t (cx+cy+cz) + t^2 (cxy+cxz+cyz) + t^3 cxyz with the mixed
    differences c of the cell's corners, and differs from the chord by (t^2 - t)(cxy+cxz+cyz) + (t^3 - t) cxyz, at most
    (|cxy|+|cxz|+|cyz|) / 4 + 0.385 |cxyz| (a face diagonal has one of the three and no cxyz).  For those nodes the bound is
        rounding + (Mxy + Mxz + Myz) / 4 + 0.385 Mxyz,    M the largest |mixed difference| over the cells."""
    eps = 2.0 ** -52
    D = max(np.abs(np.diff(phi, axis=A)).max() for A in range(3))
    ds = sum(4 * eps * (abs(xLo[A]) + np.abs(X[:, A]).max()) / dx for A in range(3))
    rounding = ds * D + 16 * eps * np.abs(phi).max()
    mixed = lambda *axes: np.abs(functools.reduce(lambda a, A: np.diff(a, axis=A), axes, phi)).max()
    curved = (mixed(0, 1) + mixed(0, 2) + mixed(1, 2)) / 4 + 0.385 * mixed(0, 1, 2)
    s = (np.asarray(X) - np.asarray(xLo)) / dx
    off_grid = np.abs(s - np.round(s)) > 1e-9
    axis_edge = off_grid.sum(axis=1) <= 1
    return np.where(axis_edge, rounding, rounding + curved), axis_edge
