"""lsf_advect_field_band restated in numpy: the serial statement of the contract in include/lsf.h, LSF_ARITH_STRICT, built on
tests/advect_ref.py (the operator, `stage`, is that file's; nothing of it is restated here).

    LIST   the interior points with mask == 1;  a stage is where(LIST, S(a), a): every stencil value comes from the stage's input
           field, whether the stencil point is in the list or not; nothing outside LIST is written, no boundary condition.

The input fields u, v, w, speed are REPLACED BY NaN OUTSIDE THE LIST before use: a result that equals the library's proves that
neither reads them there.  Everything is evaluated on whole arrays, as the header writes it, so the library's STRICT result is
compared with `==`.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple

import numpy as np

import advect_ref as R

INF_BITS = np.uint64(0x7FF0000000000000)


class BandResult(NamedTuple):
    field: np.ndarray
    steps: int
    change: List[float]
    cfl: float
    cells: int
    edge_cells: int
    edge_flips: int
    margin: float
    nan: bool  # the run ended on a NaN step (LSF_ERR_NAN): cells, edge_cells, edge_flips and margin are then not reported


def list_of(mask):
    """LIST as a boolean array: interior points (1..n-1 on each axis) with mask == 1; a 1 on a wall point is ignored."""
    lst = np.zeros(mask.shape, bool)
    I = R.interior(mask)
    lst[I] = np.asarray(mask)[I] == 1
    return lst


def edge_of(lst):
    """EDGE: the list cells with at least one of the six axis neighbours outside LIST (a wall point never is in LIST)."""
    inner = lst.copy()
    for a in range(3):
        for o in (-1, 1):
            nb = np.zeros_like(lst)  # nb[p] = lst[p + o along a]; beyond the field: not in the list (no list cell looks there)
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[a] = slice(1, None) if o == 1 else slice(None, -1)
            dst[a] = slice(None, -1) if o == 1 else slice(1, None)
            nb[tuple(dst)] = lst[tuple(src)]
            inner &= nb
    return lst & ~inner


def depth_of(lst, upto):
    """City-block distance of every list cell to the nearest point outside LIST (walls are outside), capped at upto + 1; 0 outside."""
    depth = np.zeros(lst.shape, np.int64)
    cur = lst.copy()
    for d in range(1, upto + 2):
        depth[cur] = d
        cur = cur & ~edge_of(cur)  # erosion by the six-neighbour cross: what remains lies deeper than d
    return depth


def masked_inputs(lst, vel, F):
    """The inputs with NaN outside the list (fresh arrays)."""
    hide = lambda a: np.asfortranarray(np.where(lst, a, np.nan))
    return (None if vel is None else tuple(hide(a) for a in vel)), (None if F is None else hide(F))


def nonfinite_at_list(lst, vel, F):
    """The count the library reports for non-finite inputs at list cells."""
    return int(sum(np.count_nonzero(~np.isfinite(a[lst])) for a in (list(vel or ()) + ([F] if F is not None else []))))


def cfl_number(lst, vel, F, dx, dt):
    """(dt * max over LIST cells of (|u| + |v| + |w| + |speed|)) / dx, added left to right; 0 for an empty list"""
    if not lst.any():
        return 0.0
    s = 0.0
    if vel is not None:
        s = (np.abs(vel[0][lst]) + np.abs(vel[1][lst])) + np.abs(vel[2][lst])
    if F is not None:
        s = s + np.abs(F[lst])
    return (dt * float(np.max(s))) / dx


def _S(a, lst, vel, F, dx, dt):
    """S(a) on the whole field: the interior of advect_ref.stage; only its list cells are ever used"""
    out = np.full(a.shape, np.nan, order="F")
    out[R.interior(a)] = R.stage(a, vel, F, dx, dt)
    return out


def step(phi, lst, vel, F, dx, dt, scheme="rk3"):
    a = np.asfortranarray(np.where(lst, _S(phi, lst, vel, F, dx, dt), phi))
    if scheme == "euler":
        return a
    b = np.asfortranarray(np.where(lst, 0.75 * phi + 0.25 * _S(a, lst, vel, F, dx, dt), phi))
    return np.asfortranarray(np.where(lst, (1. / 3.) * phi + (2. / 3.) * _S(b, lst, vel, F, dx, dt), phi))


def margin_of(field, edge):
    """the smallest |phi| over the edge cells as the minimum of bit patterns, at most +inf (and +inf without edge cells)"""
    bits = np.abs(field[edge]).view(np.uint64)
    m = min(INF_BITS, bits.min()) if bits.size else INF_BITS
    return float(np.array([m], np.uint64).view(np.float64)[0])


def advect_band(phi, mask, vel, F, dx, dt, steps, scheme="rk3") -> BandResult:
    """lsf_advect_field_band; the arguments are left alone.  Stops after a step whose change is NaN."""
    assert scheme in ("rk3", "euler") and (vel is not None or F is not None)
    lst = list_of(mask)
    cur = np.asfortranarray(phi, dtype=np.float64).copy(order="F")
    if not lst.any():
        return BandResult(cur, 0, [], 0.0, 0, 0, 0, math.inf, False)
    if nonfinite_at_list(lst, vel, F):
        raise ValueError(f"{nonfinite_at_list(lst, vel, F)} non-finite value(s) in u, v, w, speed at list cells")
    cfl = cfl_number(lst, vel, F, dx, dt)
    vel, F = masked_inputs(lst, vel, F)  # from here on nothing outside the list can reach the result unnoticed
    edge = edge_of(lst)
    neg0 = cur < 0
    change = []
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(steps):
            new = step(cur, lst, vel, F, dx, dt, scheme)
            change.append(float(np.max(np.abs(new[lst] - cur[lst]))))
            cur = new
            if math.isnan(change[-1]):
                return BandResult(cur, len(change), change, cfl, 0, 0, 0, math.nan, True)
    flips = int(np.count_nonzero((cur < 0)[edge] != neg0[edge]))
    return BandResult(cur, len(change), change, cfl, int(lst.sum()), int(edge.sum()), flips, margin_of(cur, edge), False)
