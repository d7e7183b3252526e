"""lsf_reseed_points restated in numpy: the statement of the contract in include/lsf.h, vectorised over the markers and candidates.
Built on tests/sample_ref.py: `locate`, the joint stencil rule, the band rule, the weights and the contraction are that file's own.

    old       BADRADIUS, OUTSIDE, OFFBAND, NONFINITE, FAR (fabs(val) > band*dx), else KEPT with
              rad' = s*fmin(fmax(s*val, rmin*dx), rmax*dx), s = rad < 0 ? -1 : 1, and count[cell] += 1.
    cells     ELIGIBLE: all 8 corners fabs(phi) < band*dx (and IN under a mask); need = max(per_cell - count, 0).
    draws     splitmix64 of ctr = (p*4096 + j)*4 + d in uint64; u = (z >> 11) * 2^-53; x_A = xLo[A] + ((double)c_A + u_A)*dx.
    attract   v0 in the caller's order; s = v0 < 0 ? -1 : 1; goal = s*((rmin + (band - rmin)*u3)*dx); the foot iteration of
              sample_points with iso = goal; the LINEAR value vl at the end decides and gives the radius.
    output    kept markers in the caller's order (src = 1-based input position), then accepted candidates in ascending (p, j), src 0.

Every expression is evaluated as the header writes it, left to right, element by element on float64 arrays, so the library's result is
compared with `==` on the bit patterns.  The arguments are left alone.

`defect` switches ONE deliberate error on (tests/test_reseed_cpu.py shows each of them failing a named check of the statement).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import sample_ref as S

LINEAR, CUBIC = S.LINEAR, S.CUBIC
KEPT, OUTSIDE, OFFBAND, NONFINITE, BADRADIUS, FAR = 0, 1, 2, 3, 4, 5
INFO_LEN, MAX_PER_CELL, MAX_ITERS = 14, 4096, 64
DEFECTS = ("goal_no_side", "final_on_order", "count_before_far", "ctr_no_j", "new_first")
Invalid = S.Invalid
_M64 = (1 << 64) - 1


class ReseedResult(NamedTuple):
    pts: np.ndarray  # (nout, 3), Fortran order
    rad: np.ndarray
    src: np.ndarray  # int32
    status: np.ndarray  # int32, (npts)
    info: list


def splitmix_int(seed: int, ctr: int) -> int:
    """the draw's 64-bit word with Python integers (the pin of tests/test_reseed_cpu.py)"""
    z = (seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(seed: int, p, j, d: int, defect=None):
    """u_d of the candidates (p, j): float64 in [0, 1); p, j integer arrays"""
    with np.errstate(over="ignore"):
        p = np.asarray(p).astype(np.uint64)
        j = np.asarray(j).astype(np.uint64)
        ctr = p * np.uint64(4096)
        if defect != "ctr_no_j":
            ctr = ctr + j
        ctr = ctr * np.uint64(4) + np.uint64(d)
        z = np.uint64(seed & _M64) + np.uint64(0x9E3779B97F4A7C15) * (ctr + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def eligible_cells(phi, mask, band_dx):
    """bool (nx, ny, nz): seedParticles' rule"""
    with np.errstate(invalid="ignore"):
        near = np.abs(phi) < band_dx
    if mask is not None:
        lst = np.zeros(phi.shape, bool)
        lst[1:-1, 1:-1, 1:-1] = np.asarray(mask)[1:-1, 1:-1, 1:-1] == 1
        near &= lst
    c = near[:-1, :-1, :-1].copy()
    for oa in range(2):
        for ob in range(2):
            for oc in range(2):
                c &= near[oa:phi.shape[0] - 1 + oa, ob:phi.shape[1] - 1 + ob, oc:phi.shape[2] - 1 + oc]
    return c


def attract(phi, mask, dx, xLo, x, goal, order, iters, tol):
    """the foot iteration of sample_ref.sample_points with a goal per point: (status, y).  status as sample_ref's."""
    m = x.shape[0]
    status = np.full(m, S.OK, np.int32)
    foot = x.copy()
    act = np.arange(m)
    y = x.copy()
    tol_dx = tol * dx
    with np.errstate(all="ignore"):
        for it in range(iters + 1):  # `iters` moves, and one more sample for the convergence test after the last
            if not act.size:
                break
            st, v, g, _, _ = S.sample_once(phi, mask, None, dx, xLo, y, order)
            gone = st != S.OK
            status[act[gone]] = st[gone]
            e = v - goal[act]
            conv = ~gone & ~(np.abs(e) > tol_dx)
            if it == iters:
                status[act[~gone & ~conv]] = S.NOT_CONVERGED
                foot[act] = y
                break
            mm = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            flat = ~gone & ~conv & (mm == 0.)
            status[act[flat]] = S.FLAT
            move = ~gone & ~conv & ~flat
            foot[act[~move]] = y[~move]
            ynew = y[move] - (e[move, None] * g[move]) / mm[move, None]
            act, y = act[move], ynew
    return status, foot


def reseed_points(phi, dx, xLo, pts=None, rad=None, mask=None, per_cell=16, rmin=0.1, rmax=0.5, band=3.0, order=CUBIC, iters=4, tol=1e-3,
                  seed=0, defect=None) -> ReseedResult:
    """lsf_reseed_points followed by lsf_reseed_get.  phi, mask: (nx+1, ny+1, nz+1); pts (npts, 3) and rad (npts), or None."""
    phi = np.asarray(phi, dtype=np.float64)
    xLo = np.asarray(xLo, dtype=np.float64)
    dx, rmin, rmax, band, tol = float(dx), float(rmin), float(rmax), float(band), float(tol)
    if phi.ndim != 3 or min(phi.shape) < 2 or phi.size > 2 ** 31 - 1:
        raise Invalid("dimensions")
    npts = 0 if pts is None else int(np.asarray(pts).shape[0])
    if npts:
        pts = np.asarray(pts, dtype=np.float64)
        rad = np.asarray(rad, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3 or rad.shape != (npts,):
            raise Invalid("pts or rad")
    if not (np.isfinite(dx) and dx > 0.) or xLo.shape != (3,) or not np.all(np.isfinite(xLo)):
        raise Invalid("dx or xLo")
    if not 1 <= per_cell <= MAX_PER_CELL:
        raise Invalid("per_cell")
    if not (np.isfinite(rmin) and np.isfinite(rmax) and np.isfinite(band)) or not 0. < rmin <= rmax or not rmin < band:
        raise Invalid("rmin, rmax or band")
    if order not in (LINEAR, CUBIC) or not 1 <= iters <= MAX_ITERS or not (np.isfinite(tol) and tol >= 0.):
        raise Invalid("order, iters or tol")
    shape = phi.shape
    rmin_dx, rmax_dx, band_dx = rmin * dx, rmax * dx, band * dx
    # ---- step 1: the old markers
    count = np.zeros(shape, np.int64)  # count of the cell whose lower corner the point is
    status = np.zeros(npts, np.int32)
    kept = np.zeros(npts, bool)
    radn = np.zeros(npts)
    wrong = 0
    if npts:
        st, val, _, _, _ = S.sample_once(phi, mask, None, dx, xLo, pts, LINEAR)
        status[:] = KEPT
        with np.errstate(invalid="ignore"):
            far = np.abs(val) > band_dx
        status[far] = FAR
        status[~np.isfinite(val)] = NONFINITE
        status[st == S.OFFBAND] = OFFBAND
        status[st == S.OUTSIDE] = OUTSIDE
        status[~np.isfinite(rad) | (rad == 0.)] = BADRADIUS
        kept = status == KEPT
        s = np.where(rad < 0., -1., 1.)
        with np.errstate(invalid="ignore"):
            sv = s * val
            radn = s * np.minimum(np.maximum(sv, rmin_dx), rmax_dx)
        wrong = int(np.count_nonzero(kept & (sv < 0.)))
        counted = kept | (status == FAR) if defect == "count_before_far" else kept
        if counted.any():
            i0 = S.locate(pts[counted], shape, dx, xLo)[1]
            np.add.at(count, (i0[:, 0], i0[:, 1], i0[:, 2]), 1)
    # ---- step 2: the cells
    elig = eligible_cells(phi, mask, band_dx)
    cnt_cells = count[:-1, :-1, :-1]
    need = np.where(elig, np.maximum(per_cell - cnt_cells, 0), 0)
    # ---- step 3: the candidates, in ascending (p, j): p ascends with i fastest, then j_c, then k
    ci, cj, ck = np.nonzero(need.transpose(2, 1, 0))[::-1]  # sorted by (k, j, i)
    nd = need[ci, cj, ck]
    ncand = int(nd.sum())
    if npts + ncand > 2 ** 31 - 1:
        raise Invalid("npts + candidates")
    cell = np.repeat(np.arange(ci.size), nd)
    jj = np.arange(ncand) - np.repeat(np.cumsum(nd) - nd, nd)
    c3 = np.stack([ci[cell], cj[cell], ck[cell]], axis=1).astype(np.int64)
    p = c3[:, 0] + shape[0] * (c3[:, 1] + shape[1] * c3[:, 2])
    u = [draw(seed, p, jj, d, defect) for d in range(4)]
    x = np.empty((ncand, 3))
    for A in range(3):
        x[:, A] = xLo[A] + (c3[:, A].astype(np.float64) + u[A]) * dx
    acc = np.zeros(ncand, bool)
    newrad = np.zeros(ncand)
    y = x.copy()
    early = late = 0
    if ncand:
        st0, v0, _, _, _ = S.sample_once(phi, mask, None, dx, xLo, x, order)
        live = (st0 == S.OK) & np.isfinite(v0)
        sg = np.where(v0 < 0., -1., 1.)
        goal = (rmin + (band - rmin) * u[3]) * dx
        if defect != "goal_no_side":
            goal = sg * goal
        idx = np.flatnonzero(live)
        ast, yy = attract(phi, mask, dx, xLo, x[idx], goal[idx], order, iters, tol)
        y[idx] = yy
        ok = idx[ast == S.OK]
        early = ncand - ok.size
        stl, vl, _, _, _ = S.sample_once(phi, mask, None, dx, xLo, y[ok], CUBIC if defect == "final_on_order" else LINEAR)
        with np.errstate(invalid="ignore"):
            av = np.abs(vl)
            good = (stl == S.OK) & (av >= rmin_dx) & (av <= band_dx) & (np.where(vl < 0., -1., 1.) == sg[ok])
            newrad[ok] = sg[ok] * np.minimum(np.maximum(av, rmin_dx), rmax_dx)
        acc[ok[good]] = True
        late = ok.size - int(np.count_nonzero(good))
    # ---- step 4: the output
    nk, na = int(np.count_nonzero(kept)), int(np.count_nonzero(acc))
    old = (pts[kept] if npts else np.zeros((0, 3)), radn[kept], (np.flatnonzero(kept) + 1).astype(np.int32))
    new = (y[acc], newrad[acc], np.zeros(na, np.int32))
    parts = (new, old) if defect == "new_first" else (old, new)
    out = np.asfortranarray(np.concatenate([parts[0][0], parts[1][0]], axis=0))
    info = [int(np.count_nonzero(status == c)) for c in range(6)] if npts else [0] * 6
    info += [int(np.count_nonzero(elig)), ncand, na, early, late, int(np.count_nonzero(cnt_cells > per_cell)), int(count.max()), wrong]
    return ReseedResult(out, np.concatenate([parts[0][1], parts[1][1]]), np.concatenate([parts[0][2], parts[1][2]]), status, info)
