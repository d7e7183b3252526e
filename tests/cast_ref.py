"""lsf_cast_rays restated in numpy: the statement of the contract in include/lsf.h, vectorised over the rays with an active set.

    ray       a non-finite origin or direction, or a length L = sqrt((d0*d0 + d1*d1) + d2*d2) that is not finite and > 0: BAD.
              u = d / L; t is a length along the ray.
    clip      slabs: [t0, t1] = [tmin, tmax] cut by the grid box, axis by axis; empty: NOGRID.
    sample    the point o + t*u; per axis s = (p - xLo) / dx, refused as OUTSIDE unless s >= -1e-6 && s <= n + 1e-6 (in double, before
              any integer), then clamped into [0, n]; from there on the stencil, the band rule, the weights and the contraction of
              lsf_sample_points (tests/sample_ref.py: _in_band, _sample_group).
    march     from t0 in steps clamp(safety*|e|, smin*dx, smax*dx) off the last on-list sample (tr, er), e = v - iso; off the list
              (mask only) in strides of skip*dx with `gap` set; the last sample is at t1; more than max_steps steps: STEPS.
              A crossing is e == 0 or (e > 0) != (er > 0); behind a gap it is LOST.
    refine    `refine` bisections of [tr, tn] by the same sign rule, one secant step, clamped into the bracket, and one full sample
              there (with q): HIT.

fmax(a, b) and fmin(a, b) are the header's own: b where a is NaN, else a where b is NaN or a >= b (a <= b), else b -- the first
argument on a tie, so that the sign of a zero is decided.  Every expression is evaluated as the header writes it, left to right,
element by element on float64 arrays, so the library's result is compared with `==` on the bit patterns.  The arguments are left
alone.

`defect` switches ONE deliberate error on (tests/test_cast_rays_cpu.py shows each of them failing a check of the statement).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import sample_ref as S

LINEAR, CUBIC = S.LINEAR, S.CUBIC
HIT, MISS, NOGRID, BAD, LOST, STEPS = 0, 1, 2, 3, 4, 5
INFO_LEN = 9
TOL_S = 1e-6  # cells: the tolerance of the locate step
DEFECTS = ("no_zero_case", "gap_ignored", "no_clamp_to_t1", "no_tolerance")
_OK, _OUTSIDE, _OFFBAND = S.OK, S.OUTSIDE, S.OFFBAND


class CastResult(NamedTuple):
    thit: np.ndarray
    hit: np.ndarray  # (nrays, 3), Fortran order
    grad: np.ndarray  # (nrays, 3), Fortran order
    qval: Optional[np.ndarray]
    status: np.ndarray  # int32
    info: list


class Invalid(ValueError):
    """LSF_ERR_INVALID"""


def fmax(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return np.where(np.isnan(a), b, np.where(np.isnan(b) | (a >= b), a, b))


def fmin(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return np.where(np.isnan(a), b, np.where(np.isnan(b) | (a <= b), a, b))


def _crossing(e, er, defect=None):
    c = (e > 0.) != (er > 0.)  # NaN counts as not > 0
    return c if defect == "no_zero_case" else (e == 0.) | c


def ray_sample(phi, mask, q, dx, xLo, pts, order, defect=None):
    """One ray sample of every point: (code, val, grad, qval); code is sample_ref's OK, OUTSIDE or OFFBAND, the rest NaN where it is
    not OK."""
    npts = pts.shape[0]
    code = np.full(npts, _OK, np.int32)
    val = np.full(npts, np.nan)
    grad = np.full((npts, 3), np.nan)
    qval = np.full(npts, np.nan) if q is not None else None
    inside = np.ones(npts, bool)
    i0 = np.zeros((npts, 3), np.int64)
    t = np.zeros((npts, 3))
    tol = 0. if defect == "no_tolerance" else TOL_S
    with np.errstate(all="ignore"):
        for A in range(3):
            n = phi.shape[A] - 1
            s = (pts[:, A] - xLo[A]) / dx
            ok = (s >= -tol) & (s <= float(n) + tol)  # in double, before any integer is made
            inside &= ok
            s = fmin(fmax(np.where(ok, s, 0.), 0.), float(n))
            i0[:, A] = np.minimum(np.floor(s).astype(np.int64), n - 1)
            t[:, A] = s - i0[:, A].astype(np.float64)
    code[~inside] = _OUTSIDE
    cub = np.zeros(npts, bool)
    if order == CUBIC:
        cub = inside.copy()
        for A in range(3):
            cub &= (i0[:, A] >= 1) & (i0[:, A] <= phi.shape[A] - 3)
    for cubic in (False, True):
        sel = np.flatnonzero(inside & (cub == cubic))
        if mask is not None and sel.size:
            ok = S._in_band(mask, i0[sel], cubic)
            code[sel[~ok]] = _OFFBAND
            sel = sel[ok]
        if not sel.size:
            continue
        v, g = S._sample_group(phi, i0[sel], t[sel], cubic, dx, True, None)
        val[sel], grad[sel] = v, g
        if q is not None:
            qval[sel] = S._sample_group(q, i0[sel], t[sel], cubic, dx, False, None)[0]
    return code, val, grad, qval


def cast_rays(phi, dx, xLo, org, dir, order=CUBIC, mask=None, q=None, iso=0.0, tmin=0.0, tmax=1e30, safety=0.9, smin=0.05, smax=1.0,
              skip=1.0, refine=24, max_steps=1000, defect=None) -> CastResult:
    """lsf_cast_rays.  phi, mask, q: (nx+1, ny+1, nz+1); org, dir: (nrays, 3).  qval is None without q."""
    phi = np.asarray(phi, dtype=np.float64)
    org = np.asarray(org, dtype=np.float64)
    dir = np.asarray(dir, dtype=np.float64)
    xLo = np.asarray(xLo, dtype=np.float64)
    dx, iso, tmin, tmax, safety, smin, smax, skip = (float(v) for v in (dx, iso, tmin, tmax, safety, smin, smax, skip))
    if phi.ndim != 3 or min(phi.shape) < 2 or phi.size > 2 ** 31 - 1:
        raise Invalid("dimensions")
    if org.ndim != 2 or org.shape[1] != 3 or org.shape[0] < 1 or dir.shape != org.shape:
        raise Invalid("nrays < 1")
    if not (np.isfinite(dx) and dx > 0.) or xLo.shape != (3,) or not np.all(np.isfinite(xLo)) or not np.isfinite(iso):
        raise Invalid("dx, xLo or iso")
    if order not in (LINEAR, CUBIC):
        raise Invalid("order")
    if not (np.isfinite(tmin) and tmin >= 0. and np.isfinite(tmax) and tmax > tmin):
        raise Invalid("tmin or tmax")
    if not (safety > 0. and safety <= 1. and np.isfinite(smin) and smin > 0. and np.isfinite(smax) and smax >= smin and np.isfinite(skip) and skip > 0.):
        raise Invalid("safety, smin, smax or skip")
    if refine < 0 or max_steps < 1:
        raise Invalid("refine or max_steps")
    if q is not None:
        q = np.asarray(q, dtype=np.float64)
    n = org.shape[0]
    status = np.full(n, -1, np.int32)
    thit = np.full(n, np.nan)
    hit = np.full((n, 3), np.nan)
    grad = np.full((n, 3), np.nan)
    qval = np.full(n, np.nan) if q is not None else None
    nsamp = np.zeros(n, np.int64)
    nskip = np.zeros(n, np.int64)
    inner = np.zeros(n, bool)
    smin_dx, smax_dx, skip_dx = smin * dx, smax * dx, skip * dx
    with np.errstate(all="ignore"):
        # 1. the ray
        fin = np.all(np.isfinite(org), axis=1) & np.all(np.isfinite(dir), axis=1)
        L = np.sqrt((dir[:, 0] * dir[:, 0] + dir[:, 1] * dir[:, 1]) + dir[:, 2] * dir[:, 2])
        good = fin & (L > 0.) & np.isfinite(L)
        status[~good] = BAD
        u = dir / np.where(good, L, 1.)[:, None]
        # 2. the clip
        t0 = np.full(n, tmin)
        t1 = np.full(n, tmax)
        nogrid = np.zeros(n, bool)
        for A in range(3):
            lo, hi = xLo[A], xLo[A] + float(phi.shape[A] - 1) * dx
            par = u[:, A] == 0.
            nogrid |= par & ~((org[:, A] >= lo) & (org[:, A] <= hi))
            ua = np.where(par, 1., u[:, A])
            a, b = (lo - org[:, A]) / ua, (hi - org[:, A]) / ua
            t0 = np.where(par, t0, fmax(t0, fmin(a, b)))
            t1 = np.where(par, t1, fmin(t1, fmax(a, b)))
        nogrid |= ~(t0 <= t1)
        status[good & nogrid] = NOGRID

        def sample(idx, t, qq=None):
            p = org[idx] + t[:, None] * u[idx]
            return (p,) + ray_sample(phi, mask, qq, dx, xLo, p, order, defect)

        # 4. the march.  Per ray: t the position of the next sample, (tr, er) the reference, gap, last.
        act = np.flatnonzero(status < 0)
        t = t0[act].copy()
        tr = np.zeros(act.size)
        er = np.zeros(act.size)
        have = np.zeros(act.size, bool)
        gap = np.zeros(act.size, bool)
        last = np.zeros(act.size, bool)
        # the rays that go on to the refinement: index, bracket and its two values
        R_idx, R_ta, R_ea, R_tb, R_eb, R_bis = [], [], [], [], [], []

        def to_refine(sel, ta, ea, tb, eb, bisect):
            R_idx.append(act[sel]), R_ta.append(ta), R_ea.append(ea), R_tb.append(tb), R_eb.append(eb)
            R_bis.append(np.full(ta.shape, bisect))

        for k in range(max_steps + 1):  # the first sample and at most max_steps further ones
            if not act.size:
                break
            _, code, v, _, _ = sample(act, t)
            on = code == _OK
            nsamp[act[on]] += 1
            e = v - iso
            done = np.zeros(act.size, bool)
            out = code == _OUTSIDE
            status[act[out]] = MISS
            thit[act[out]] = t[out]
            done |= out
            off = code == _OFFBAND
            gap[off] = True
            nskip[act[off]] += 1
            first = on & ~have
            inner[act[first]] = e[first] < 0.
            zero = first & (e == 0.)  # a HIT at this t: the bracket is [t, t]
            to_refine(zero, t[zero], e[zero], t[zero], e[zero], False)  # (nothing to bisect)
            done |= zero
            cross = on & have & _crossing(e, er, defect)
            lost = cross & gap
            if defect == "gap_ignored":
                lost = np.zeros(act.size, bool)
            status[act[lost]] = LOST
            found = cross & ~lost
            to_refine(found, tr[found], er[found], t[found], e[found], True)
            done |= cross
            ref = on & ~done  # the sample becomes the reference
            tr[ref], er[ref] = t[ref], e[ref]
            gap[ref] = False
            have |= first
            step = np.where(off, skip_dx, fmin(fmax(safety * np.abs(er), smin_dx), smax_dx))
            end = ~done & last  # after the last sample without a crossing
            status[act[end]] = MISS
            thit[act[end]] = t[end]
            done |= end
            if k == max_steps:
                status[act[~done]] = STEPS
                break
            tn = t + step
            over = ~(tn < t1[act])
            if defect != "no_clamp_to_t1":
                tn = np.where(over, t1[act], tn)
            last = last | over
            keep = ~done
            act, t, tr, er, have, gap, last = act[keep], tn[keep], tr[keep], er[keep], have[keep], gap[keep], last[keep]

        # 5. the refinement
        idx = np.concatenate(R_idx) if R_idx else np.zeros(0, np.int64)
        ta, ea, tb, eb = (np.concatenate(a) if R_idx else np.zeros(0) for a in (R_ta, R_ea, R_tb, R_eb))
        bis = np.concatenate(R_bis) if R_idx else np.zeros(0, bool)
        for _ in range(refine):
            if not bis.any():
                break
            sel = np.flatnonzero(bis)
            tm = 0.5 * (ta[sel] + tb[sel])
            _, code, v, _, _ = sample(idx[sel], tm)
            okm = code == _OK
            nsamp[idx[sel[okm]]] += 1
            status[idx[sel[~okm]]] = LOST
            bis[sel[~okm]] = False
            em = v - iso
            left = okm & _crossing(em, ea[sel], defect)
            right = okm & ~left
            tb[sel[left]], eb[sel[left]] = tm[left], em[left]
            ta[sel[right]], ea[sel[right]] = tm[right], em[right]
        alive = status[idx] < 0
        idx, ta, ea, tb, eb = idx[alive], ta[alive], ea[alive], tb[alive], eb[alive]
        quo = (ea * (tb - ta)) / (eb - ea)
        th = np.where((eb != ea) & np.isfinite(quo), ta - quo, ta)
        th = fmin(fmax(th, ta), tb)
        p, code, v, g, qv = sample(idx, th, q)
        ok = code == _OK
        nsamp[idx[ok]] += 1
        status[idx[~ok]] = LOST
        h = idx[ok]
        status[h] = HIT
        thit[h], hit[h], grad[h] = th[ok], p[ok], g[ok]
        if q is not None:
            qval[h] = qv[ok]
    assert np.all(status >= 0)
    info = [int(np.count_nonzero(status == s)) for s in (HIT, MISS, NOGRID, BAD, LOST, STEPS)]
    info += [int(nsamp.sum()), int(nskip.sum()), int(np.count_nonzero(inner))]
    return CastResult(thit, np.asfortranarray(hit), np.asfortranarray(grad), qval, status, info)
