"""The cases of lsf_evolve_band_curv shared by tests/test_evolve_band_curv_cpu.py (their properties, on the statement) and
tests/test_gpu_evolve_band_curv.py (the library against the statement).  Statement results are computed once and read-only.

Every case starts from a distance clamped to +-far, far = (core + ring) dx, with the mask |distance| < far.  dt comes from the CFL
number where a velocity or a speed exists; bcurv = lam dx^2 / dt (curvonly: bcurv = 1 and dt = lam dx^2).  A chunk is 256 list
entries (MB_CH in csrc/lsf_minmax_band.hpp).
  curvsmall  (14,13,12), u = (1,0,0), CFL 0.5, lam 0.15, core 1.5, ring 2, 1 sweep, 6 steps, clamp 1: wall-adjacent list cells, one
             rebuild, clamped cells in every step, degenerate cells (the placeholders) in the step after the rebuild
  curvonly   (24,22,20), no velocity and no speed, lam 0.2, core 2.5, ring 2, 2 sweeps, 12 steps: the instance without R0, cfl == 0,
             a ragged last chunk, no rebuild
  dumbbell   (40,33,27), two spheres, u = (1,.5,-.25) and speed 0.5, CFL 0.5, lam 0.15, core 3, ring 3, 2 sweeps, 12 steps: a
             concave kink, a rebuild that grows every workspace slot mid-call
  euler      (24,22,20), u = (1,.3,0), CFL 0.3, lam 0.1, Euler, 9 steps, clamp 0: no rebuild, an odd step count, no clamp
"""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import advect_ref as R
import evolve_band_curv_ref as VC

CHUNK = 256  # MB_CH


class Case(NamedTuple):
    npts: Tuple[int, int, int]
    spheres: Tuple[Tuple[Tuple[float, float, float], float], ...]  # (centre, radius) of each
    u: Optional[Tuple[float, float, float]]
    speed: Optional[float]
    cfl: Optional[float]
    lam: float
    core: float
    ring: int
    sweeps: int
    steps: int
    clamp: float = 1.0
    scheme: str = "rk3"


CASES = {
    "curvsmall": Case((14, 13, 12), (((-0.1, -0.2, -0.3), 0.45),), (1, 0, 0), None, 0.5, 0.15, 1.5, 2, 1, 6),
    "curvonly": Case((24, 22, 20), (((0, -0.1, -0.25), 0.3),), None, None, None, 0.2, 2.5, 2, 2, 12),
    "dumbbell": Case((40, 33, 27), (((-0.45, -0.3, -0.5), 0.35), ((0.1, -0.2, -0.4), 0.35)), (1, .5, -.25), 0.5, 0.5, 0.15, 3, 3, 2, 12),
    "euler": Case((24, 22, 20), (((-0.1, -0.1, -0.25), 0.4),), (1, .3, 0), None, 0.3, 0.1, 2, 3, 2, 9, 0.0, "euler"),
}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(phi0, mask, vel or None, F or None, (nx, ny, nz), dx, dt, bcurv, keywords of the call); shared and read-only"""
    c = CASES[case]
    dist = None
    for centre, radius in c.spheres:
        d, dx = R.sphere_distance(c.npts, centre, radius)
        dist = d if dist is None else np.minimum(dist, d)
    far = (c.core + float(c.ring)) * dx
    phi0 = np.asfortranarray(np.clip(dist, -far, far))
    mask = np.asfortranarray((np.abs(dist) < far).astype(np.int32))
    vel = None if c.u is None else tuple(np.asfortranarray(np.full(c.npts, float(x))) for x in c.u)
    F = None if c.speed is None else np.asfortranarray(np.full(c.npts, float(c.speed)))
    if c.cfl is None:
        bcurv = 1.0
        dt = c.lam * dx * dx / bcurv
    else:
        dt = c.cfl * dx / R.max_speed(vel, F)
        bcurv = c.lam * dx * dx / dt
    for a in (phi0, mask) + (vel or ()) + ((F,) if F is not None else ()):
        a.setflags(write=False)
    kw = dict(scheme=c.scheme, core=float(c.core), ring=c.ring, reinit_sweeps=c.sweeps, h=0.5 * dx, clamp=c.clamp)
    return phi0, mask, vel, F, tuple(n - 1 for n in c.npts), dx, dt, bcurv, kw


@functools.lru_cache(maxsize=None)
def want(case, steps=None, clamp=None):
    """(the statement's result, the log of (degenerate, clamped) list cells per stage)"""
    phi0, mask, vel, F, _, dx, dt, bcurv, kw = inputs(case)
    if clamp is not None:
        kw = dict(kw, clamp=clamp)
    log = []
    r = VC.evolve_band_curv(phi0, mask, vel, F, dx, dt, CASES[case].steps if steps is None else steps, bcurv, log=log, **kw)
    assert not r.nan
    r.field.setflags(write=False), r.mask.setflags(write=False)
    # FAST must take the same schedule: no margin of a check within 1e-6 dx of the threshold
    core_dx = CASES[case].core * dx
    assert all(abs(m - core_dx) >= 1e-6 * dx for m in r.margins), (case, [m / dx for m in r.margins])
    return r, tuple(log)


def per_step(case, log):
    """the log summed over the stages of each step: [(degenerate, clamped)]"""
    k = 1 if CASES[case].scheme == "euler" else 3
    return [tuple(sum(x[q] for x in log[s:s + k]) for q in range(2)) for s in range(0, len(log), k)]
