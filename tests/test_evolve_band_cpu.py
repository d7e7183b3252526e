"""lsf_evolve_band without a GPU: the interface through every layer, properties of the serial statement of the contract
(tests/evolve_band_ref.py, composed from tests/advect_band_ref.py and tests/band_emulator.py), argument validation before the
library, and no CPU fallback."""
import functools
import math
import os
import re

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R
import evolve_band_ref as V
from conftest import ROOT


def _mask(cond):
    return np.asfortranarray(cond.astype(np.int32))


def _const(npts, c):
    return np.asfortranarray(np.full(npts, float(c)))


# ---------------------------------------------------------------------------------- the interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_evolve_band", 25), ("lsf_evolve_band_device", 26)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_EVOLVE_INFO_LEN\s+6\b", hdr) and _lib.LSF_EVOLVE_INFO_LEN == 6
    assert callable(lsf.evolveBand) and "evolveBand" in levelset.__all__ and "EvolveBandReport" in levelset.__all__
    assert lsf.EvolveBandReport._fields == ("steps", "cfl", "change", "cells", "open_cells", "flips", "rebuilds", "entered", "near_wall", "margin")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_evolveband():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bevolveBand\b", public)
    assert "BIND(C,NAME='lsf_evolve_band')" in src
    assert re.search(r"^SUBROUTINE evolveBand\(phi,mask,u,v,w,nx,ny,nz,dx,dt,steps\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_evolve_band',rc)" in src
    assert re.search(r"^!\s+evolveBand\(phi,mask,u,v,w,nx,ny,nz,dx,dt,steps\)", src, flags=re.M)  # the header comment's list of procedures


# ---------------------------------------------------------------------------------- the statement
def test_open_edge_rule_ignores_wall_neighbours():
    """Every interior point in the list: all the wall-adjacent cells are edge cells of lsf_advect_field_band, none is OPEN.  A gap at
    an interior point opens its six neighbours and nothing else."""
    m = np.ones((7, 6, 8), np.int32, order="F")
    lst = B.list_of(m)
    assert B.edge_of(lst).sum() == 5 * 4 * 6 - 3 * 2 * 4 and V.open_edge_of(lst).sum() == 0
    m[1, 2, 3] = 0  # a gap next to the wall i = 0
    op = V.open_edge_of(B.list_of(m))
    assert op.sum() == 5 and op[2, 2, 3] and op[1, 1, 3] and op[1, 3, 3] and op[1, 2, 2] and op[1, 2, 4] and not op[1, 2, 3]
    assert V.near_wall_of(lst).sum() == 5 * 4 * 6 - 3 * 2 * 4


def test_dilation_is_chebyshev_and_clipped_to_the_interior():
    core = np.zeros((9, 8, 7), bool, order="F")
    core[1, 4, 3] = True
    new = V.dilate(core, 2)
    assert new.sum() == 3 * 5 * 5 and new[1:4, 2:7, 1:6].all() and not new[0].any()  # the cube, cut at the wall i = 0
    assert new[3, 6, 5] and not new[4, 4, 3]  # corners belong (Chebyshev, not city-block)
    core[7, 6, 5] = True  # nx - 1, ny - 1, nz - 1
    new = V.dilate(core, 8)
    assert np.array_equal(new, V.interior_of(core.shape))
    assert not V.dilate(np.zeros((6, 6, 6), bool), 3).any()


def test_entering_values_and_their_sign_rule():
    cur = np.asfortranarray(np.array([[[-2.0, -0.0, 0.0, 3.0, -1e-300, np.inf]]]))
    ent = np.ones(cur.shape, bool)
    out = V.entering_values(cur, ent, 0.75)
    assert list(out.ravel()) == [-0.75, 0.75, 0.75, 0.75, -0.75, 0.75]  # -0.0 is not < 0
    ent[0, 0, 0] = False
    assert V.entering_values(cur, ent, 0.75)[0, 0, 0] == -2.0  # anything else keeps its value


@functools.lru_cache(maxsize=None)
def _small():
    """the `small` case of tests/test_gpu_evolve_band.py: (14,13,12), one rebuild, wall-adjacent list cells"""
    npts = (14, 13, 12)
    phi, dx = R.sphere_distance(npts, (-0.1, -0.2, -0.3), 0.45)
    far = 3.5 * dx
    phi0 = np.asfortranarray(np.clip(phi, -far, far))
    return phi0, _mask(np.abs(phi) < far), (_const(npts, 1), _const(npts, 0), _const(npts, 0)), dx, 0.5 * dx


def test_a_rebuild_moves_the_list_and_calls_compose():
    phi0, mask, vel, dx, dt = _small()
    kw = dict(core=1.5, ring=2, reinit_sweeps=1)
    keep = [a.copy() for a in (phi0, mask, *vel)]
    r = V.evolve_band(phi0, mask, vel, None, dx, dt, 6, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(keep, (phi0, mask, *vel)))  # the arguments are left alone
    lst0, lst1 = B.list_of(mask), r.mask == 1
    assert (r.steps, r.rebuilds, r.rebuilt_after, r.flips, r.entered) == (6, 1, [4], 0, 248) and lst0.sum() == 668
    assert r.cells == lst1.sum() == 838 and set(np.unique(r.mask)) == {0, 1} and not (lst1 & ~V.interior_of(lst1.shape)).any()
    assert (lst1 & ~lst0).sum() == 248 and (lst0 & ~lst1).sum() == 668 + 248 - 838  # cells entered in front and left behind
    assert B.edge_of(lst1).sum() > r.open_cells == V.open_edge_of(lst1).sum() > 0  # wall-adjacent list cells: the open-edge rule matters
    never = ~lst0 & ~lst1
    assert np.array_equal(r.field[never], phi0[never]) and r.cfl == 0.5
    # 6 steps = 3 + 3 for phi, mask and trace (check_every = 1 divides 3)
    a = V.evolve_band(phi0, mask, vel, None, dx, dt, 3, **kw)
    b = V.evolve_band(a.field, a.mask, vel, None, dx, dt, 3, **kw)
    assert np.array_equal(b.field, r.field) and np.array_equal(b.mask, r.mask) and a.change + b.change == r.change
    assert a.rebuilds + b.rebuilds == 1 and b.margin == r.margin and b.cells == r.cells
    # a non-finite input anywhere is an error, off the list too
    bad = vel[0].copy(order="F")
    bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="1 non-finite"):
        V.evolve_band(phi0, mask, (bad, vel[1], vel[2]), None, dx, dt, 1, **kw)


def test_the_flip_ending_empty_list_zero_steps_and_a_nan():
    npts = (20, 20, 20)
    phi0, dx = R.sphere_distance(npts, (-0.1, 0.0, 0.0), 0.5)
    vel = (_const(npts, 1), _const(npts, 0), _const(npts, 0))
    thin = _mask(np.abs(phi0) < 0.6 * dx)
    r = V.evolve_band(phi0, thin, vel, None, dx, 0.5 * dx, 4, core=0.25, ring=1, reinit_sweeps=0)
    assert (r.steps, r.flips, r.rebuilds, len(r.change)) == (1, 44, 0, 1) and r.cells == B.list_of(thin).sum()  # the loud ending
    late = V.evolve_band(phi0, thin, vel, None, dx, 0.5 * dx, 4, core=0.25, ring=1, reinit_sweeps=0, check_every=3)
    assert late.steps == 3 and late.flips > 44  # seen at the first check only
    walls = np.zeros(npts, np.int32, order="F")
    walls[0], walls[:, :, -1] = 1, 1
    e = V.evolve_band(phi0, walls, vel, None, dx, 0.5 * dx, 3)
    assert (e.steps, e.change, e.cfl, e.cells, e.open_cells, e.flips, e.rebuilds, e.entered, e.near_wall, e.margin) == (0, [], 0.0, 0, 0, 0, 0, 0, 0, math.inf)
    assert np.array_equal(e.field, phi0) and not e.mask.any()
    wide = _mask(np.abs(phi0) < 6 * dx)
    wide[3, 3, 3], wide[0] = 7, 1  # normalised away
    z = V.evolve_band(phi0, wide, vel, None, dx, 0.5 * dx, 0)
    op = V.open_edge_of(B.list_of(wide))
    assert z.steps == 0 and z.cfl == 0.5 and (z.flips, z.rebuilds, z.entered) == (0, 0, 0) and z.open_cells == op.sum()
    assert z.margin == np.abs(phi0[op]).min() and np.array_equal(z.field, phi0) and np.array_equal(z.mask == 1, B.list_of(wide))
    bad = phi0.copy(order="F")
    bad[tuple(np.argwhere(B.list_of(wide))[40])] = np.nan
    n = V.evolve_band(bad, wide, vel, None, dx, 0.5 * dx, 3)
    assert n.nan and n.steps == 1 and math.isnan(n.change[0]) and n.cells is None and np.array_equal(n.mask == 1, B.list_of(wide))


def test_the_list_tracks_a_sphere_over_three_times_its_half_width():
    """The distance to a sphere of radius 0.5 clamped to +-6 dx on 49^3 points, mask |phi| < 6 dx, u = (1,0,0) at CFL 0.5, 36 steps:
    the surface moves 18 cells.  core = 3, ring = 3, h = 0.5 dx.  Measured with the statement: 2 sweeps per step: 6 rebuilds (after
    steps 5, 10, 16, 22, 28, 34), no flips, largest error over |exact| < 2 dx 0.029 dx (the full-grid lsf_advect_field statement
    alone: 0.014 dx); reinit_sweeps = 0: 5 rebuilds, 3.3 dx off."""
    npts = (49, 49, 49)
    centre = (-0.6, -0.1, 0.05)
    phi, dx = R.sphere_distance(npts, centre, R.RADIUS)
    phi0 = np.asfortranarray(np.clip(phi, -6 * dx, 6 * dx))
    mask = _mask(np.abs(phi) < 6 * dx)
    vel = (_const(npts, 1), _const(npts, 0), _const(npts, 0))
    dt, steps = 0.5 * dx, 36
    exact, _ = R.sphere_distance(npts, (centre[0] + steps * dt, centre[1], centre[2]), R.RADIUS)
    near = np.abs(exact) < 2 * dx
    assert steps * dt == 18 * dx and not (near & ~V.interior_of(npts)).any()
    r = V.evolve_band(phi0, mask, vel, None, dx, dt, steps, core=3.0, ring=3, reinit_sweeps=2)
    err = float(np.abs(r.field - exact)[near].max()) / dx
    print(f"2 sweeps: {r.rebuilds} rebuilds after steps {r.rebuilt_after}, flips {r.flips}, {r.cells} cells, error {err:.4f} dx")
    assert r.steps == steps and r.rebuilds >= 3 and r.flips == 0
    assert (r.mask[near] == 1).all()
    assert err < 0.1
    r0 = V.evolve_band(phi0, mask, vel, None, dx, dt, steps, core=3.0, ring=3, reinit_sweeps=0)
    err0 = float(np.abs(r0.field - exact)[near].max()) / dx
    print(f"0 sweeps: {r0.rebuilds} rebuilds, flips {r0.flips}, error {err0:.4f} dx")
    assert err0 > 1.0  # the placeholders are corrected by the sweeps and by nothing else


# ---------------------------------------------------------------------------------- the Python layer
def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    u = np.ones((6, 6, 6), order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    ok = dict(velocity=(u, u, u))
    call = lambda *a, **k: lsf.evolveBand(*a, 5, 5, 5, 0.1, 0.01, 1, **k)
    for kw in (dict(), dict(velocity=(u, u)), dict(velocity=(u, None, u)), dict(ok, scheme="rk4"), dict(ok, arith="exact"),
               dict(velocity=(u, u, np.ones((6, 5, 6), order="F"))), dict(speed=np.ones((5, 6, 6), order="F")),
               dict(ok, core=0.0), dict(ok, core=-1.0), dict(ok, core=float("nan")), dict(ok, core=float("inf")),
               dict(ok, ring=0), dict(ok, ring=9), dict(ok, ring=2.5), dict(ok, reinit_sweeps=-1), dict(ok, h=0.0), dict(ok, h=float("inf")),
               dict(ok, h=float("nan")), dict(ok, check_every=0)):
        with pytest.raises(ValueError):
            call(phi, m, **kw)
    with pytest.raises(ValueError):
        call(np.ones((6, 6, 5), order="F"), m, **ok)
    with pytest.raises(ValueError):
        call(np.ones((6, 6, 6), order="C"), m, **ok)
    with pytest.raises(ValueError):
        call(phi, None, **ok)
    with pytest.raises(ValueError):
        call(phi, np.ones((6, 5, 6), np.int32, order="F"), **ok)
    with pytest.raises(ValueError):
        call(phi, np.ones((6, 6, 6), np.int32, order="C"), **ok)
    for bad_phi, bad_m, kw in ((phi.astype(np.float32), m, ok), (phi, m.astype(np.int64), ok), (phi, m.astype(bool), ok),
                               (phi, m, dict(speed=u.astype(np.float32))), (phi, m, dict(velocity=(u, u, [[1.0]])))):
        with pytest.raises(TypeError):
            call(bad_phi, bad_m, **kw)
    assert np.all(phi == 1.0) and np.all(u == 1.0) and np.all(m == 1)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    u = np.ones((6, 6, 6), order="F")
    m = np.full((6, 6, 6), 7, np.int32, order="F")
    for kw in (dict(velocity=(u, u, u)), dict(speed=u), dict(velocity=(u, u, u), speed=u, scheme="euler", arith="fast", reinit_sweeps=0)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.evolveBand(phi, m, 5, 5, 5, 0.1, 0.01, 1, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(phi == 1.0) and np.all(m == 7)
