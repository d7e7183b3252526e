"""Input fields of the fp32 Jacobi tests (tests/test_reinit_f32_cpu.py, tests/test_gpu_f32_statement.py) and, computed once
per process and left unchanged, what every test compares against: the fp64 oracle and the float32 statement
(tests/reinit_f32_ref.py) on the same fp32-rounded input.  All fields come from formulas and seeds.

  two      fields.two_sphere_phi0: smooth, the three WENO stencils nearly agree
  cube     phi0 of tests/golden/cube40_62.npz (62^3): flat +-1 far field (first differences exactly 0), kinks
  box      max(|x|-0.7, |y|-0.5, |z|-0.9) on grid_axes, unsmeared: linear pieces that meet in kinks
  noisy    sphere_phi0 + 1e-3 * standard normal noise
  random   uniform in [-1, 1]
  scaled   box with phi, dx and h multiplied by s
"""
from __future__ import annotations

import functools
import os

import numpy as np

import reinit_f32_ref as stmt
from levelsetfortran_amd import fields

NPTS = (37, 30, 41)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SCALES_ASSERTED = (1e-8, 1e8)    # the full accuracy rule holds
SCALES_FINITE = (1e-13, 1e15)    # beyond the floor / towards the overflow of the unscaled q_k: finiteness only
ACCURACY_FIELDS = ("two", "cube", "box", "noisy", "random") + tuple(f"scaled{s:g}" for s in SCALES_ASSERTED)
FINITE_FIELDS = tuple(f"scaled{s:g}" for s in SCALES_FINITE)


def box_distance(npts):
    x, y, z, dx = fields.grid_axes(npts)
    d = np.maximum(np.maximum(np.abs(x)[:, None, None] - 0.7, np.abs(y)[None, :, None] - 0.5), np.abs(z)[None, None, :] - 0.9)
    return np.asfortranarray(d), float(dx)


def make(name, npts=NPTS):
    """(input rounded to float32, Fortran-ordered; dx; h) of the named field"""
    scale = 1.0
    if name == "two":
        phi, dx = fields.two_sphere_phi0(npts)
    elif name == "cube":
        z = np.load(os.path.join(GOLDEN, "cube40_62.npz"), allow_pickle=False)
        phi, dx = z["phi0"], float(z["dx"])
    elif name == "box":
        phi, dx = box_distance(npts)
    elif name == "noisy":
        phi, dx = fields.sphere_phi0(npts)
        phi = phi + 1e-3 * np.random.default_rng(20240519).standard_normal(phi.shape)
    elif name == "random":
        dx = fields.grid_axes(npts)[3]
        phi = np.random.default_rng(7315).uniform(-1.0, 1.0, npts)
    elif name.startswith("scaled"):
        scale = float(name[len("scaled"):])
        phi, dx = box_distance(npts)
    else:
        raise KeyError(name)
    h = fields.reinit_step(dx)
    return np.asfortranarray((phi * scale).astype(np.float32)), float(dx * scale), float(h * scale)


class Case:
    """One field and sweep count: input, the fp64 oracle's result and the float32 statement's, and their distance."""

    def __init__(self, name, sweeps, npts=NPTS):
        import oracle_lib

        self.name, self.sweeps = name, sweeps
        self.in32, self.dx, self.h = make(name, npts)
        self.nx, self.ny, self.nz = (v - 1 for v in self.in32.shape)
        self.ref = np.asfortranarray(self.in32.astype(np.float64))
        rc, n, self.ref_trace = oracle_lib.reinit(self.ref, self.nx, self.ny, self.nz, sweeps - 1, self.dx, self.h, tol=0.0,
                                                  order=oracle_lib.JACOBI)
        assert rc == 0 and n == sweeps
        self.stmt, n, self.stmt_trace = stmt.reinit(self.in32, self.nx, self.ny, self.nz, sweeps - 1, self.dx, self.h, tol=0.0,
                                                    dtype=np.float32)
        assert n == sweeps
        self.stmt_max, self.stmt_rms = stmt.distance(self.stmt, self.ref)
        for a in (self.in32, self.ref, self.stmt):
            a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def _case(name, sweeps, npts):
    return Case(name, sweeps, npts)


def case(name, sweeps, npts=NPTS):
    """the shared, read-only Case (cube has its own 62^3 shape)"""
    return _case(name, int(sweeps), NPTS if name == "cube" else tuple(npts))
