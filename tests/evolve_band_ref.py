"""lsf_evolve_band restated in numpy: the serial statement of the contract in include/lsf.h, LSF_ARITH_STRICT.  Composed from
tests/advect_band_ref.py (`step`, `list_of`, `edge_of`, `margin_of`: the transport on a list) and tests/band_emulator.py
(`band_sweep`: one sweep of lsf_reinit_band); nothing of either is restated here.  What is new is stated on whole arrays:

    OPEN EDGE  a list cell with an axis neighbour that is an INTERIOR point outside LIST (a wall neighbour opens nothing)
    CHECK      flips and margin over the open-edge cells; flips end the call, margin < core dx rebuilds
    REBUILD    CORE = list cells with |phi| < core dx; NEW = interior points within Chebyshev distance `ring` of a CORE cell;
               entering cells take -far / +far by (phi < 0); leaving cells keep their value; the sign reference is renewed

The library's STRICT result is compared with `==`.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

import numpy as np

import advect_band_ref as B
import advect_ref as R
import band_emulator as E


class EvolveResult(NamedTuple):
    field: np.ndarray
    mask: np.ndarray  # int32, 1 on the cells of the list on return, 0 elsewhere
    steps: int
    change: List[float]
    cfl: float
    cells: Optional[int]       # info[0] .. info[5] and margin: None when the run ended on a NaN step
    open_cells: Optional[int]
    flips: Optional[int]
    rebuilds: Optional[int]
    entered: Optional[int]
    near_wall: Optional[int]
    margin: Optional[float]
    nan: bool
    rebuilt_after: List[int]   # 1-based steps after which a rebuild took place (not part of the interface)
    margins: List[float]       # the margin of every check of the time loop (not part of the interface)


def interior_of(shape):
    inner = np.zeros(shape, bool)
    inner[R.interior(inner)] = True
    return inner


def open_edge_of(lst):
    """the list cells with an axis neighbour that is an interior point outside LIST"""
    # the walls count as members: what edge_of then still finds is open towards an interior point
    return B.edge_of(lst | ~interior_of(lst.shape)) & lst


def dilate(core, ring):
    """the interior points within Chebyshev distance `ring` of a cell of `core`"""
    out = core.copy()
    for a in range(3):
        acc = out.copy()
        for o in range(1, ring + 1):
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            src[a], dst[a] = slice(o, None), slice(None, -o)
            acc[tuple(dst)] |= out[tuple(src)]
            acc[tuple(src)] |= out[tuple(dst)]
        out = acc
    return out & interior_of(core.shape)


def entering_values(cur, entering, far):
    """-far where phi < 0, +far otherwise (-0.0 and every positive value)"""
    return np.asfortranarray(np.where(entering, np.where(cur < 0, -far, far), cur))


def near_wall_of(lst):
    """the list cells with a wall point among their axis neighbours"""
    inner2 = np.zeros(lst.shape, bool)
    inner2[tuple(slice(2, s - 2) for s in lst.shape)] = True
    return lst & ~inner2


def nonfinite(vel, F):
    return int(sum(np.count_nonzero(~np.isfinite(a)) for a in (list(vel or ()) + ([F] if F is not None else []))))


def evolve_band(phi, mask, vel, F, dx, dt, steps, scheme="rk3", core=3.0, ring=3, reinit_sweeps=2, h=None, check_every=1) -> EvolveResult:
    """lsf_evolve_band; the arguments are left alone."""
    assert scheme in ("rk3", "euler") and (vel is not None or F is not None)
    assert core > 0 and 1 <= ring <= 8 and reinit_sweeps >= 0 and check_every >= 1 and steps >= 0
    h = 0.5 * dx if h is None else h
    if nonfinite(vel, F):
        raise ValueError(f"{nonfinite(vel, F)} non-finite value(s) in u, v, w, speed")
    lst = B.list_of(mask)
    cur = np.asfortranarray(phi, dtype=np.float64).copy(order="F")
    nx, ny, nz = (s - 1 for s in cur.shape)
    if not lst.any():
        return EvolveResult(cur, np.zeros(cur.shape, np.int32, order="F"), 0, [], 0.0, 0, 0, 0, 0, 0, 0, math.inf, False, [], [])
    cfl = R.cfl_number(vel, F, dx, dt)
    far = (core + float(ring)) * dx
    neg_ref = cur < 0
    change, rebuilt_after, margins = [], [], []
    rebuilds = entered = flips = 0

    def check():
        op = open_edge_of(lst)
        return int(np.count_nonzero((cur < 0)[op] != neg_ref[op])), B.margin_of(cur, op), int(op.sum())

    as_mask = lambda: np.asfortranarray(lst.astype(np.int32))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(steps):
            new = B.step(cur, lst, vel, F, dx, dt, scheme)
            change.append(float(np.max(np.abs(new[lst] - cur[lst]))))
            cur = new
            if math.isnan(change[-1]):
                return EvolveResult(cur, as_mask(), len(change), change, cfl, None, None, None, None, None, None, None, True, rebuilt_after, margins)
            sgn = cur
            for _ in range(reinit_sweeps):
                cur, _ = E.band_sweep(cur, sgn, lst, nx, ny, nz, dx, h)
            if (s + 1) % check_every == 0 or s == steps - 1:
                flips, margin, _ = check()
                margins.append(margin)
                if flips > 0:
                    break
                if margin < core * dx:
                    new_lst = dilate(lst & (np.abs(cur) < core * dx), ring)
                    entering = new_lst & ~lst
                    cur = entering_values(cur, entering, far)
                    entered += int(entering.sum())
                    lst, neg_ref = new_lst, cur < 0
                    rebuilds += 1
                    rebuilt_after.append(s + 1)
    # of the list and the field on return: what the last check saw, or -- after a rebuild, where nothing has flipped yet -- the new list
    flips, margin, n_open = check()
    near = int(np.count_nonzero(near_wall_of(lst) & (np.abs(cur) < core * dx)))
    return EvolveResult(cur, as_mask(), len(change), change, cfl, int(lst.sum()), n_open, flips, rebuilds, entered, near, margin, False,
                        rebuilt_after, margins)
