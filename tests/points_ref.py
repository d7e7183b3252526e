"""lsf_advect_points and lsf_correct_field restated in numpy: the statement of the two contracts in include/lsf.h, vectorised over
the points.  Built on tests/sample_ref.py: `locate`, the joint stencil rule, the band rule, the weights and the contraction are that
file's own (sample_once for the linear value of the correction, its pieces for the value-only samples of the velocity).

    advect    x' = (u, v, w)(x) + speed(x) * grad phi(x) / |grad phi(x)| in fields frozen for the call, by TVD-RK3 or Euler:
                  k = K(x0); x1 = x0 + dt*k
                  k = K(x1); x2 = 0.75*x0 + 0.25*(x1 + dt*k)
                  k = K(x2); xn = (1./3.)*x0 + (2./3.)*(x2 + dt*k)
              A step completes when each sample was OK and xn is INSIDE; otherwise the point keeps the bits of x0 and stops with
              the status of what failed.
    correct   markers with rad = side * radius; an ESCAPED marker (s*val < -(slack*r)) offers cand = s*(r - d) to the 8 corners of
              its cell; plus = max, minus = min in the TOTAL order of the bit patterns; phi = |plus| <= |minus| ? plus : minus.

Every expression is evaluated as the header writes it, left to right, element by element on float64 arrays, so the library's result is
compared with `==` on the bit patterns.  The arguments are left alone.

`defect` switches ONE deliberate error on (tests/test_points_cpu.py shows each of them failing a named check of the statement).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import sample_ref as S

LINEAR, CUBIC = S.LINEAR, S.CUBIC
RK3, EULER = 0, 1
OK, OUTSIDE, OFFBAND, FLAT = 0, 1, 2, 3  # status of lsf_advect_points
INPLACE, ESCAPED, C_OUTSIDE, C_OFFBAND, NONFINITE, BADRADIUS = 0, 1, 2, 3, 4, 5  # status of lsf_correct_field
ADVECT_INFO_LEN, CORRECT_INFO_LEN = 6, 7
MAX_STEPS = 4096
DEFECTS = ("swap_025_075", "xn_not_tested", "escape_plus_r", "float_max", "prefer_minus")
Invalid = S.Invalid


class AdvectResult(NamedTuple):
    pts: np.ndarray  # (npts, 3), Fortran order
    status: np.ndarray  # int32
    cfl: float
    info: list


class CorrectResult(NamedTuple):
    phi: np.ndarray
    status: np.ndarray  # int32
    change: float
    info: list


# ---------------------------------------------------------------------------------------------------------- lsf_advect_points
def _sites(shape, mask, dx, xLo, pos, order):
    """locate, stencil and band of sample_once without any value: (status, i0, t, cub)"""
    m = pos.shape[0]
    status = np.full(m, OK, np.int32)
    inside, i0, t = S.locate(pos, shape, dx, xLo)
    status[~inside] = OUTSIDE
    cub = np.zeros(m, bool)
    if order == CUBIC:
        cub = inside.copy()
        for A in range(3):
            cub &= (i0[:, A] >= 1) & (i0[:, A] <= shape[A] - 3)  # 1 <= i0 <= n - 2 on all three axes
    if mask is not None:
        for cubic in (False, True):
            sel = np.flatnonzero(inside & (cub == cubic))
            if sel.size:
                status[sel[~S._in_band(mask, i0[sel], cubic)]] = OFFBAND
    return status, i0, t, cub


def _values(fields, i0, t, cubic):
    """the values of several fields at located points that all use one stencil, under one set of weights: what
    sample_ref._sample_group(field, ..., want_grad=False) gives for each -- the same products and sums in the same order (pinned by
    tests/test_points_cpu.py) -- with the stencil's point indices formed once for all of them"""
    K = 4 if cubic else 2
    off = -1 if cubic else 0
    wx, wy, wz = (S.weights(t[:, A], cubic)[0] for A in range(3))
    n0, n1 = fields[0].shape[0], fields[0].shape[1]
    flat = [f.reshape(-1, order="F") for f in fields]  # point index p = i + (nx+1) * (j + (ny+1) * k)
    base = (i0[:, 0] + off) + n0 * ((i0[:, 1] + off) + n1 * (i0[:, 2] + off))
    p = [[] for _ in fields]
    for c in range(K):
        r = [[] for _ in fields]
        for b in range(K):
            row = base + n0 * (b + n1 * c)
            idx = [row + m for m in range(K)]
            for q, f in enumerate(flat):
                r[q].append(S._contract(wx, [f[j] for j in idx]))
        for q in range(len(fields)):
            p[q].append(S._contract(wy, r[q]))
    return [S._contract(wz, pq) for pq in p]


def rhs(vel, speed, phi, mask, dx, xLo, pos, order):
    """K at the positions pos (m, 3): (status, k (m, 3), fallback).  status is OK, OUTSIDE, OFFBAND or FLAT; k is meaningful where OK;
    fallback marks the OK samples of a cubic request served linearly."""
    shape = (vel[0] if vel is not None else phi).shape
    m = pos.shape[0]
    status, i0, t, cub = _sites(shape, mask, dx, xLo, pos, order)
    k = np.full((m, 3), np.nan)
    with np.errstate(all="ignore"):
        for cubic in (False, True):
            sel = np.flatnonzero((status == OK) & (cub == cubic))
            if not sel.size:
                continue
            U = None
            if vel is not None:
                U = _values(vel, i0[sel], t[sel], cubic)
            if speed is None:
                for A in range(3):
                    k[sel, A] = U[A]
                continue
            _, g = S._sample_group(phi, i0[sel], t[sel], cubic, dx, True, None)
            f = S._sample_group(speed, i0[sel], t[sel], cubic, dx, False, None)[0]
            mm = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            nrm = np.sqrt(mm)
            for A in range(3):
                k[sel, A] = (f * g[:, A]) / nrm if U is None else U[A] + (f * g[:, A]) / nrm
            status[sel[mm == 0.]] = FLAT
    fallback = (status == OK) & ~cub if order == CUBIC else np.zeros(m, bool)
    # (a FLAT sample is not OK: it is no fallback either)
    return status, k, fallback


def _check_grid(f, what="dimensions"):
    if f.ndim != 3 or min(f.shape) < 2 or f.size > 2 ** 31 - 1:
        raise Invalid(what)


def advect_points(pts, dx, xLo, dt, nsteps, velocity=None, speed=None, phi=None, mask=None, order=CUBIC, scheme=RK3,
                  defect=None) -> AdvectResult:
    """lsf_advect_points.  velocity: (u, v, w) or None; fields (nx+1, ny+1, nz+1); pts (npts, 3)."""
    pts = np.asarray(pts, dtype=np.float64)
    xLo = np.asarray(xLo, dtype=np.float64)
    dx, dt = float(dx), float(dt)
    if velocity is not None:
        if len(velocity) != 3 or any(f is None for f in velocity):
            raise Invalid("u, v, w come together")
        velocity = [np.asarray(f, dtype=np.float64) for f in velocity]
    if velocity is None and speed is None:
        raise Invalid("no group at all")
    if (speed is None) != (phi is None):
        raise Invalid("speed and phi come together")
    if speed is not None:
        speed, phi = np.asarray(speed, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    first = velocity[0] if velocity is not None else phi
    _check_grid(first)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise Invalid("npts < 1")
    if not (np.isfinite(dx) and dx > 0.) or xLo.shape != (3,) or not np.all(np.isfinite(xLo)) or not np.isfinite(dt):
        raise Invalid("dx, xLo or dt")
    if order not in (LINEAR, CUBIC) or scheme not in (RK3, EULER) or not 1 <= nsteps <= MAX_STEPS:
        raise Invalid("order, scheme or nsteps")
    npts = pts.shape[0]
    shape = first.shape
    out = pts.copy()
    status = np.full(npts, OK, np.int32)
    inside = S.locate(pts, shape, dx, xLo)[0]
    status[~inside] = OUTSIDE
    act = np.flatnonzero(inside)  # points still moving
    cfl_key = np.uint64(0)
    steps_done = 0
    nfall = 0
    a1, a2 = (0.25, 0.75) if defect == "swap_025_075" else (0.75, 0.25)
    nstage = 3 if scheme == RK3 else 1
    with np.errstate(all="ignore"):
        for _ in range(nsteps):
            if not act.size:
                break
            x0 = out[act]
            y = x0
            alive = np.ones(act.size, bool)  # every sample of the step so far was OK
            why = np.full(act.size, OK, np.int32)
            cmax = np.zeros(act.size)
            for stage in range(nstage):
                idx = np.flatnonzero(alive)
                st, k, fb = rhs(velocity, speed, phi, mask, dx, xLo, y[idx], order)
                nfall += int(np.count_nonzero(fb))
                bad = st != OK
                why[idx[bad]] = st[bad]
                alive[idx[bad]] = False
                idx, k, yy, xx = idx[~bad], k[~bad], y[idx[~bad]], x0[idx[~bad]]
                dk = dt * k
                if stage == 0:
                    yn = xx + dk
                elif stage == 1:
                    yn = a1 * xx + a2 * (yy + dk)
                else:
                    yn = (1. / 3.) * xx + (2. / 3.) * (yy + dk)
                y = y.copy()
                y[idx] = yn
                c = (np.abs(dk) / dx).max(axis=1) if idx.size else np.zeros(0)
                cmax[idx] = np.maximum(cmax[idx], c)
            idx = np.flatnonzero(alive)
            if defect != "xn_not_tested":
                ins = S.locate(y[idx], shape, dx, xLo)[0]
                why[idx[~ins]] = OUTSIDE
                alive[idx[~ins]] = False
            done = np.flatnonzero(alive)
            out[act[done]] = y[done]
            steps_done += done.size
            if done.size:
                cfl_key = max(cfl_key, cmax[done].view(np.uint64).max())
            status[act[~alive]] = why[~alive]
            act = act[alive]
    info = [int(np.count_nonzero(status == s)) for s in (OK, OUTSIDE, OFFBAND, FLAT)] + [steps_done, nfall]
    return AdvectResult(np.asfortranarray(out), status, float(np.array([cfl_key], np.uint64).view(np.float64)[0]), info)


# ---------------------------------------------------------------------------------------------------------- lsf_correct_field
def to_key(x):
    """the order-preserving 64-bit key of a double: b ^ (b >> 63 ? ~0 : 1 << 63); -0.0 sorts below +0.0"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63))


def from_key(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    b = k ^ np.where(k >> np.uint64(63) != 0, np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF))
    return b.view(np.float64)


def correct_field(phi, dx, xLo, pts, rad, mask=None, slack=1.0, defect=None) -> CorrectResult:
    """lsf_correct_field.  phi, mask: (nx+1, ny+1, nz+1); pts (npts, 3); rad (npts).  Returns the corrected copy of phi."""
    phi = np.asarray(phi, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    rad = np.asarray(rad, dtype=np.float64)
    xLo = np.asarray(xLo, dtype=np.float64)
    dx, slack = float(dx), float(slack)
    _check_grid(phi)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1 or rad.shape != (pts.shape[0],):
        raise Invalid("npts < 1")
    if not (np.isfinite(dx) and dx > 0.) or xLo.shape != (3,) or not np.all(np.isfinite(xLo)):
        raise Invalid("dx or xLo")
    if not (np.isfinite(slack) and slack >= 0.):
        raise Invalid("slack")
    npts = pts.shape[0]
    st, val, _, _, _ = S.sample_once(phi, mask, None, dx, xLo, pts, LINEAR)
    status = np.full(npts, INPLACE, np.int32)
    r = np.abs(rad)
    s = np.where(rad > 0., 1., -1.)
    with np.errstate(all="ignore"):
        esc = s * val < (r if defect == "escape_plus_r" else -(slack * r))
    status[esc] = ESCAPED
    status[~np.isfinite(val)] = NONFINITE
    status[st == S.OFFBAND] = C_OFFBAND
    status[st == S.OUTSIDE] = C_OUTSIDE
    status[~np.isfinite(rad) | (rad == 0.)] = BADRADIUS
    shape = phi.shape
    flat_old = phi.reshape(-1, order="F").copy()  # point index p = i + (nx+1) * (j + (ny+1) * k)
    plus, minus = to_key(flat_old), to_key(flat_old)
    e = np.flatnonzero(status == ESCAPED)
    if e.size:
        i0 = S.locate(pts[e], shape, dx, xLo)[1]
        for oc in range(2):
            for ob in range(2):
                for oa in range(2):
                    I = [i0[:, 0] + oa, i0[:, 1] + ob, i0[:, 2] + oc]
                    ee = [(xLo[A] + I[A].astype(np.float64) * dx) - pts[e, A] for A in range(3)]
                    d = np.sqrt((ee[0] * ee[0] + ee[1] * ee[1]) + ee[2] * ee[2])
                    cand = s[e] * (r[e] - d)
                    p = I[0] + shape[0] * (I[1] + shape[1] * I[2])
                    pos = s[e] > 0.
                    np.maximum.at(plus, p[pos], to_key(cand[pos]))
                    np.minimum.at(minus, p[~pos], to_key(cand[~pos]))
    fp, fm = from_key(plus), from_key(minus)
    if defect == "float_max":  # a comparison of values: +0.0 does not beat -0.0
        fp = np.where(fp == flat_old, flat_old, fp)
        fm = np.where(fm == flat_old, flat_old, fm)
    with np.errstate(all="ignore"):
        take_plus = np.abs(fp) < np.abs(fm) if defect == "prefer_minus" else np.abs(fp) <= np.abs(fm)
    new = np.where(take_plus, fp, fm)
    if mask is not None:  # the list: interior points with mask == 1 (no candidate reaches any other point anyway)
        lst = np.zeros(shape, bool, order="F")
        lst[1:-1, 1:-1, 1:-1] = np.asarray(mask)[1:-1, 1:-1, 1:-1] == 1
        new = np.where(lst.reshape(-1, order="F"), new, flat_old)
    changed = new.view(np.uint64) != flat_old.view(np.uint64)
    with np.errstate(all="ignore"):
        diff = np.abs(new[changed] - flat_old[changed])
    change = float(diff.view(np.uint64).max().view(np.float64)) if diff.size else 0.0  # the maximum of the bit patterns
    info = [int(np.count_nonzero(status == c)) for c in range(6)] + [int(np.count_nonzero(changed))]
    return CorrectResult(np.asfortranarray(new.reshape(shape, order="F")), status, change, info)


# ---------------------------------------------------------------------------------------------------------- seeding, by the public rule
def seed_particles(phi, dx, xLo, mask=None, per_cell=16, rmin=0.1, rmax=0.5, band=3.0, seed=0):
    """seedParticles of the package restated on the statement's own sampler: (pts (npts, 3) Fortran order, rad)"""
    phi = np.asarray(phi, dtype=np.float64)
    near = np.abs(phi) < band * dx
    if mask is not None:
        lst = np.zeros(phi.shape, bool)
        lst[1:-1, 1:-1, 1:-1] = np.asarray(mask)[1:-1, 1:-1, 1:-1] == 1
        near &= lst
    c = near[:-1, :-1, :-1].copy()
    for oa in range(2):
        for ob in range(2):
            for oc in range(2):
                c &= near[oa:phi.shape[0] - 1 + oa, ob:phi.shape[1] - 1 + ob, oc:phi.shape[2] - 1 + oc]
    cells = np.argwhere(c)  # C order of (i, j, k)
    rng = np.random.default_rng(seed)
    off = rng.random((cells.shape[0], per_cell, 3))
    pts = (np.asarray(xLo, dtype=np.float64) + (cells[:, None, :] + off) * dx).reshape(-1, 3)
    if not pts.shape[0]:
        return np.zeros((0, 3), order="F"), np.zeros(0)
    val = S.sample_once(phi, mask, None, dx, np.asarray(xLo, dtype=np.float64), pts, LINEAR)[1]
    with np.errstate(invalid="ignore"):
        keep = (np.abs(val) >= rmin * dx) & (np.abs(val) <= band * dx)
    pts, val = pts[keep], val[keep]
    rad = np.sign(val) * np.clip(np.abs(val), rmin * dx, rmax * dx)
    return np.asfortranarray(pts), rad
