"""lsf_evolve_band_curv without a GPU: the interface through every layer, properties of the serial statement of the contract
(tests/evolve_band_curv_ref.py, composed from tests/evolve_band_ref.py, tests/advect_band_ref.py, tests/advect_ref.py and
tests/curvature_ref.py), the properties of the GPU cases (tests/evolve_band_curv_cases.py), argument validation before the library,
and no CPU fallback."""
import math
import os
import re

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R
import evolve_band_curv_cases as K
import evolve_band_curv_ref as VC
import evolve_band_ref as V
from conftest import ROOT

REPORT_FIELDS = ("steps", "cfl", "diffusion", "change", "cells", "open_cells", "flips", "rebuilds", "entered", "near_wall", "margin")


# ---------------------------------------------------------------------------------- the interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_evolve_band_curv", 28), ("lsf_evolve_band_curv_device", 29)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert callable(lsf.evolveBandCurv) and "evolveBandCurv" in levelset.__all__ and "EvolveBandCurvReport" in levelset.__all__
    assert lsf.EvolveBandCurvReport._fields == REPORT_FIELDS
    assert tuple(f for f in REPORT_FIELDS if f != "diffusion") == lsf.EvolveBandReport._fields
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_evolvebandcurv():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bevolveBandCurv\b", public)
    assert "BIND(C,NAME='lsf_evolve_band_curv')" in src
    assert re.search(r"^SUBROUTINE evolveBandCurv\(phi,mask,speed,nx,ny,nz,dx,dt,steps,b\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_evolve_band_curv',rc)" in src
    assert re.search(r"^!\s+evolveBandCurv\(phi,mask,speed,nx,ny,nz,dx,dt,steps,b\)", src, flags=re.M)  # the header comment's list of procedures


# ---------------------------------------------------------------------------------- the statement
def test_without_the_term_the_statement_is_evolve_band():
    """bcurv = 0 on the `small` case of tests/test_evolve_band_cpu.py: field, mask, trace and every count."""
    npts = (14, 13, 12)
    phi, dx = R.sphere_distance(npts, (-0.1, -0.2, -0.3), 0.45)
    far = 3.5 * dx
    phi0 = np.asfortranarray(np.clip(phi, -far, far))
    mask = np.asfortranarray((np.abs(phi) < far).astype(np.int32))
    vel = tuple(np.asfortranarray(np.full(npts, c)) for c in (1.0, 0.0, 0.0))
    kw = dict(core=1.5, ring=2, reinit_sweeps=1)
    want = V.evolve_band(phi0, mask, vel, None, dx, 0.5 * dx, 6, **kw)
    got = VC.evolve_band_curv(phi0, mask, vel, None, dx, 0.5 * dx, 6, 0.0, clamp=0.37, **kw)
    assert want.rebuilds == 1 and got.diffusion == 0.0
    assert np.array_equal(got.field, want.field) and np.array_equal(got.mask, want.mask)
    assert tuple(got[2:5]) == tuple(want[2:5]) and tuple(got[6:]) == tuple(want[5:])  # steps, change, cfl; every count, margin, the schedule
    assert B._S.__module__ == "advect_band_ref"  # the stage operator is back in place


def _sphere_run(t_end, lam, bcurv, N=33, R0=0.6):
    """The closed-form run of the header's guidance: (result, radius error in dx, exact radius, dx)"""
    npts = (N, N, N)
    dist, dx = R.sphere_distance(npts, (0.0, 0.0, 0.0), R0)
    phi0 = np.asfortranarray(np.clip(dist, -6 * dx, 6 * dx))
    mask = np.asfortranarray((np.abs(dist) < 6 * dx).astype(np.int32))
    steps = int(round(t_end / (lam * dx * dx)))
    dt = t_end / steps
    kw = dict(core=3.0, ring=3, reinit_sweeps=2, h=0.5 * dx)
    if bcurv > 0:
        r = VC.evolve_band_curv(phi0, mask, None, None, dx, dt, steps, bcurv, clamp=1.0, **kw)
    else:  # the term left out: a speed of 0 only
        r = V.evolve_band(phi0, mask, None, np.zeros(npts, order="F"), dx, dt, steps, **kw)
    exact = math.sqrt(R0 * R0 - 4.0 * t_end)
    return r, abs(radius_on_x(r.field, N, dx) - exact) / dx, exact, dx


def radius_on_x(field, N, dx):
    """the zero crossing on the +x axis from the centre outwards, by linear interpolation"""
    c = (N - 1) // 2
    line = field[c:, c, c]
    i = int(np.argmax(line >= 0))
    assert i > 0 and line[i - 1] < 0 <= line[i]
    return (i - 1 + line[i - 1] / (line[i - 1] - line[i])) * dx


MEASURED_RADIUS_ERROR_DX = 0.0481  # the statement's figure for the run below; the bound is twice this


def test_a_sphere_shrinks_by_its_mean_curvature():
    """Motion by mean curvature against the closed form sqrt(R0^2 - 4 b t): R0 = 0.6 on 33^3 points over [-1.5,1.5]^3, the distance
    clamped to +-6 dx, mask |phi| < 6 dx, core = 3, ring = 3, 2 sweeps, h = 0.5 dx, b = 1, clamp 1, RK3, no velocity and no speed,
    t = 0.07 at b dt/dx^2 = 0.15 (53 steps).  Measured with this statement: 1 rebuild (after step 41), no flips, the radius on the +x
    axis off by 0.0481 dx (the issue's prototype, not bit-true in its transport part: 0.048 dx).  With the term left out the radius
    stays R0, 3.4 dx from the closed form."""
    r, err, exact, dx = _sphere_run(0.07, 0.15, 1.0)
    print(f"t = 0.07: {r.steps} steps, diffusion {r.diffusion:.4f}, rebuilds {r.rebuilds} after {r.rebuilt_after}, flips {r.flips}, "
          f"radius error {err:.4f} dx (exact radius {exact / dx:.3f} dx)")
    assert r.cfl == 0.0 and abs(r.diffusion - 0.15) < 0.003
    assert r.rebuilds >= 1 and r.flips == 0 and not r.nan and np.isfinite(r.field).all()
    assert err < 2 * MEASURED_RADIUS_ERROR_DX
    r0, err0, _, _ = _sphere_run(0.07, 0.15, 0.0)
    print(f"without the term: radius error {err0:.4f} dx")
    assert err0 > 1.0


# ---------------------------------------------------------------------------------- the GPU cases keep exercising their paths
def test_the_gpu_cases_show_their_properties():
    cells0 = lambda case: int(B.list_of(K.inputs(case)[1]).sum())
    chunks = lambda n: -(-n // K.CHUNK)
    # curvsmall: wall-adjacent list cells, one rebuild, the clamp live in every stage, the placeholders degenerate after the rebuild
    r, log = K.want("curvsmall")
    lst0 = B.list_of(K.inputs("curvsmall")[1])
    assert cells0("curvsmall") == 668 and V.near_wall_of(lst0).sum() > 0
    assert (r.steps, r.rebuilt_after, r.flips) == (6, [5], 0) and r.cfl == 0.5 and abs(r.diffusion - 0.15) < 1e-12
    before = log[:15]  # the stages of the five steps before the rebuild
    assert all(d == 0 for d, _ in before) and min(c for _, c in before) == 33 and max(c for _, c in before) == 201
    assert log[15][0] == 75 and sum(d for d, _ in log[15:]) > 75 and all(c > 0 for _, c in log)
    # curvonly: the instance without R0
    r, log = K.want("curvonly")
    n0 = cells0("curvonly")
    assert K.inputs("curvonly")[2] is None and K.inputs("curvonly")[3] is None and K.inputs("curvonly")[7] == 1.0
    assert n0 == 1326 and n0 % K.CHUNK != 0 and (r.steps, r.rebuilds, r.flips, r.cfl) == (12, 0, 0, 0.0) and abs(r.diffusion - 0.2) < 1e-12
    assert all(c > 0 for _, c in log)
    # dumbbell: every workspace slot grows mid-call, a concave kink
    r, log = K.want("dumbbell")
    n0 = cells0("dumbbell")
    assert (n0, r.cells, r.rebuilt_after, r.flips, r.steps) == (7390, 11003, [8], 0, 12) and (chunks(n0), chunks(r.cells)) == (29, 43)
    assert n0 % K.CHUNK != 0 and r.cells % K.CHUNK != 0 and abs(r.cfl - 0.5) < 1e-12
    steps = K.per_step("dumbbell", log)
    assert all(c >= 200 for _, c in steps) and steps[8][0] > 0
    # euler: no clamp, and the clamp would have mattered
    r, log = K.want("euler")
    assert (r.steps, r.rebuilds, r.flips) == (9, 0, 0) and K.CASES["euler"].clamp == 0.0 and all(c == 0 for _, c in log)
    r1, log1 = K.want("euler", None, 1.0)
    assert any(c > 0 for _, c in log1) and not np.array_equal(r1.field, r.field)


# ---------------------------------------------------------------------------------- the Python layer
def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    u = np.ones((6, 6, 6), order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    nan, inf = float("nan"), float("inf")
    call = lambda *a, **k: lsf.evolveBandCurv(*a, 5, 5, 5, 0.1, 0.01, 1, **k)
    for kw in (dict(curvature=-1.0), dict(curvature=nan), dict(curvature=inf), dict(curvature=-inf, speed=u),  # a bad curvature
               dict(curvature=1.0, clamp=-0.5), dict(curvature=1.0, clamp=nan), dict(curvature=1.0, clamp=inf),  # a bad clamp
               dict(curvature=0.0), dict(curvature=0.0, clamp=0.0),  # neither inputs nor curvature
               dict(curvature=1.0, velocity=(u, u)), dict(curvature=1.0, scheme="rk4"), dict(curvature=1.0, arith="exact"),
               dict(curvature=1.0, core=0.0), dict(curvature=1.0, ring=9), dict(curvature=1.0, reinit_sweeps=-1), dict(curvature=1.0, h=0.0),
               dict(curvature=1.0, check_every=0)):
        with pytest.raises(ValueError):
            call(phi, m, **kw)
    with pytest.raises(TypeError):
        call(phi, m)  # curvature is required
    with pytest.raises(ValueError):
        call(phi, None, curvature=1.0)
    with pytest.raises(TypeError):
        call(phi.astype(np.float32), m, curvature=1.0)
    assert np.all(phi == 1.0) and np.all(u == 1.0) and np.all(m == 1)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    u = np.ones((6, 6, 6), order="F")
    m = np.full((6, 6, 6), 7, np.int32, order="F")
    for kw in (dict(curvature=1.0), dict(curvature=0.5, speed=u), dict(curvature=0.0, velocity=(u, u, u)),
               dict(curvature=2.0, velocity=(u, u, u), speed=u, scheme="euler", arith="fast", reinit_sweeps=0, clamp=0.0)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.evolveBandCurv(phi, m, 5, 5, 5, 0.1, 0.01, 1, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(phi == 1.0) and np.all(m == 7)
