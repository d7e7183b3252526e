"""lsf_evolve_band_curv restated in numpy: the serial statement of the contract in include/lsf.h, LSF_ARITH_STRICT.  Composed from
tests/evolve_band_ref.py (`evolve_band`: the list, the steps, the check and the rebuild), tests/advect_band_ref.py (`step`: the
blends on a list), tests/advect_ref.py (`stage`: t0 = a - dt R0) and tests/curvature_ref.py (`interior_values`: H and g); nothing of
them is restated here.  What is new:

    S(a)       t = t0 + dt * C,  C = bcurv * (H * g),  H and g evaluated on the stage's input field a (clamp applied to H);
               with neither a velocity nor a speed t0 = a
    diffusion  (bcurv * dt) / (dx * dx)

The loop of evolve_band_ref asks advect_band_ref for its stage operator `_S` by name at every stage; `evolve_band_curv` runs that loop
with `_S` bound to the S above for the length of the call.  Everything is evaluated on whole arrays, as the header writes it, so the
library's STRICT result is compared with `==`.
"""
from __future__ import annotations

import contextlib
from typing import List, NamedTuple, Optional

import numpy as np

import advect_band_ref as B
import advect_ref as R
import curvature_ref as C
import evolve_band_ref as E


class EvolveCurvResult(NamedTuple):
    """evolve_band_ref.EvolveResult with `diffusion` after `cfl`"""
    field: np.ndarray
    mask: np.ndarray
    steps: int
    change: List[float]
    cfl: float
    diffusion: float
    cells: Optional[int]
    open_cells: Optional[int]
    flips: Optional[int]
    rebuilds: Optional[int]
    entered: Optional[int]
    near_wall: Optional[int]
    margin: Optional[float]
    nan: bool
    rebuilt_after: List[int]
    margins: List[float]


def term(a, dx, bcurv, clamp):
    """(C, degenerate, clamped) on all interior cells of the stage's input field a"""
    H, _, g, deg, cH, _ = C.interior_values(a, dx, clamp)
    with np.errstate(all="ignore"):
        return bcurv * (H * g), deg, cH


def S_with_term(bcurv, clamp, log=None):
    """S(a) on the whole field, with the signature of advect_band_ref._S; log: a list that receives per stage the numbers of
    degenerate and clamped list cells"""
    def S(a, lst, vel, F, dx, dt):
        I = R.interior(a)
        with np.errstate(all="ignore"):
            t0 = a[I] if vel is None and F is None else R.stage(a, vel, F, dx, dt)
            c, deg, cl = term(a, dx, bcurv, clamp)
            out = np.full(a.shape, np.nan, order="F")
            out[I] = t0 + dt * c
        if log is not None:
            log.append((int(np.count_nonzero(deg & lst[I])), int(np.count_nonzero(cl & lst[I]))))
        return out
    return S


@contextlib.contextmanager
def stage_operator(S):
    """advect_band_ref.step with S as its stage operator, for the length of the block"""
    keep = B._S
    B._S = S
    try:
        yield
    finally:
        B._S = keep


def evolve_band_curv(phi, mask, vel, F, dx, dt, steps, bcurv, clamp=1.0, scheme="rk3", core=3.0, ring=3, reinit_sweeps=2, h=None,
                     check_every=1, log=None) -> EvolveCurvResult:
    """lsf_evolve_band_curv; the arguments are left alone.  bcurv = 0 is evolve_band_ref.evolve_band itself."""
    assert np.isfinite(bcurv) and bcurv >= 0 and np.isfinite(clamp) and clamp >= 0
    assert bcurv > 0 or vel is not None or F is not None
    diffusion = (bcurv * dt) / (dx * dx)
    args = (dx, dt, steps, scheme, core, ring, reinit_sweeps, h, check_every)
    if bcurv == 0:
        r = E.evolve_band(phi, mask, vel, F, *args)
    elif vel is None and F is None:
        # the loop wants an input to scan: a speed of 0 gives cfl = 0, and S above is handed the absent inputs, not this one
        S = S_with_term(bcurv, clamp, log)
        with stage_operator(lambda a, lst, _vel, _F, dx_, dt_: S(a, lst, None, None, dx_, dt_)):
            r = E.evolve_band(phi, mask, None, np.zeros(np.shape(phi), order="F"), *args)
    else:
        with stage_operator(S_with_term(bcurv, clamp, log)):
            r = E.evolve_band(phi, mask, vel, F, *args)
    return EvolveCurvResult(*r[:5], diffusion, *r[5:])
