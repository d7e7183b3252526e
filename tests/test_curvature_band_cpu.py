"""lsf_curvature_band without a GPU: the interface through every layer, properties of the serial statement of the contract
(tests/curvature_ref.py), argument validation before the library, and no CPU fallback."""
import os
import re

import numpy as np
import pytest

import advect_ref as R
import curvature_ref as C
from advect_band_ref import list_of
from conftest import ROOT

CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6  # the sphere of the other band tests


def _mask(cond):
    return np.asfortranarray(cond.astype(np.int32))


def _outs(npts, k=3):
    return [np.full(npts, np.nan, order="F") for _ in range(k)]


# ---------------------------------------------------------------------------------- the interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_curvature_band", 12), ("lsf_curvature_band_device", 13)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_CURV_INFO_LEN\s+4\b", hdr) and _lib.LSF_CURV_INFO_LEN == 4
    assert callable(lsf.curvatureBand) and "curvatureBand" in levelset.__all__ and "CurvatureReport" in levelset.__all__
    assert lsf.CurvatureReport._fields == ("cells", "degenerate", "clamped", "kappa_max")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_curvatureband():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bcurvatureBand\b", public)
    assert "BIND(C,NAME='lsf_curvature_band')" in src
    assert re.search(r"^SUBROUTINE curvatureBand\(phi,mask,kappa,nx,ny,nz,dx,clamp\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_curvature_band',rc)" in src
    assert re.search(r"^!\s+curvatureBand\(phi,mask,kappa,nx,ny,nz,dx,clamp\)", src, flags=re.M)  # the header comment's list of procedures


# ---------------------------------------------------------------------------------- the statement
def _sphere_errors(N):
    """(list cells, largest |kappa - 2/r| over the surface's 2/R, largest |K - 1/r^2| over 1/R^2) on the cells with |phi| < 2.1 dx:
    each cell is compared with the level set through it, the error is stated in units of the surface's curvature"""
    npts = (N, N, N)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.1 * dx)
    k, g, _ = _outs(npts)
    res = C.curvature_band(phi, mask, dx, k, g)
    L = list_of(mask)
    r = phi[L] + RADIUS
    assert res.nonfinite == 0 and res.degenerate == 0 and res.clamped == 0 and res.cells == L.sum()
    return res.cells, float(np.max(np.abs(res.kappa[L] - 2. / r)) / (2. / RADIUS)), float(np.max(np.abs(res.gauss[L] - 1. / r ** 2)) * RADIUS ** 2)


def test_sphere_is_second_order():
    n25, k25, g25 = _sphere_errors(25)
    n49, k49, g49 = _sphere_errors(49)
    print(f"sphere 25^3: {n25} cells, kappa error {k25:.4g}, K error {g25:.4g};  49^3: {n49} cells, kappa {k49:.4g}, K {g49:.4g}")
    assert n25 == 1286
    assert k49 <= k25 / 4 and g49 <= g25 / 4  # second order
    assert abs(k25 - 0.0499) < 5e-5 and abs(g25 - 0.168) < 5e-4
    assert abs(k49 - 0.00532) < 5e-6 and abs(g49 - 0.0134) < 5e-5


def test_signs_and_gmag_on_the_sphere():
    npts = (25, 25, 25)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.1 * dx)
    res = C.curvature_band(phi, mask, dx, *_outs(npts))
    L = list_of(mask)
    assert np.all(res.kappa[L] > 0) and np.all(res.gauss[L] > 0)  # phi < 0 inside: +2/r, 1/r^2
    assert np.max(np.abs(res.gmag[L] - 1.0)) < 0.05
    assert res.kappa_max == np.abs(res.kappa[L]).max()
    # -phi: kappa changes sign bit for bit, K and |grad| do not change
    neg = C.curvature_band(-phi, mask, dx, *_outs(npts))
    assert np.array_equal(neg.kappa[L], -res.kappa[L]) and np.array_equal(neg.gauss[L], res.gauss[L]) and np.array_equal(neg.gmag[L], res.gmag[L])


def test_plane_has_no_curvature():
    from levelsetfortran_amd import fields

    npts = (49, 49, 49)
    x, y, z, dx = fields.grid_axes(npts)
    n = np.array((0.3, -0.5, 0.8))
    n /= np.linalg.norm(n)
    phi = np.asfortranarray(n[0] * x[:, None, None] + n[1] * y[None, :, None] + n[2] * z[None, None, :] - 0.05)
    res = C.curvature_band(phi, np.ones(npts, np.int32, order="F"), dx, *_outs(npts))
    L = list_of(np.ones(npts, np.int32))
    print(f"plane 49^3: max |kappa| {np.abs(res.kappa[L]).max():.3e}, max |K| {np.abs(res.gauss[L]).max():.3e}")
    assert res.cells == 47 ** 3 and res.degenerate == 0
    assert np.abs(res.kappa[L]).max() < 1e-11  # roundoff of the second differences, which scales with 1/dx^2
    assert np.abs(res.gauss[L]).max() < 1e-22
    assert np.max(np.abs(res.gmag[L] - 1.0)) < 1e-13


def _cylinder_error(N):
    from levelsetfortran_amd import fields

    npts = (N, N, N)
    x, y, z, dx = fields.grid_axes(npts)
    r = np.sqrt((x[:, None, None] - CENTRE[0]) ** 2 + (y[None, :, None] - CENTRE[1]) ** 2 + 0. * z[None, None, :])
    phi = np.asfortranarray(r - RADIUS)
    mask = _mask(np.abs(phi) < 2.1 * dx)
    res = C.curvature_band(phi, mask, dx, *_outs(npts))
    L = list_of(mask)
    assert res.nonfinite == 0 and np.all(res.gauss[L] == 0.0)  # every z derivative is an exact zero
    return float(np.max(np.abs(res.kappa[L] - 1. / r[L])) * RADIUS)


def test_cylinder_along_z_has_zero_gaussian_curvature():
    e25, e49 = _cylinder_error(25), _cylinder_error(49)
    print(f"cylinder: kappa error over the surface's 1/R {e25:.4g} at 25^3, {e49:.4g} at 49^3")
    assert e49 <= e25 / 4
    assert abs(e25 - 0.0514) < 5e-5 and abs(e49 - 0.00542) < 5e-6


def _flat_case():
    """the sphere on 25^3 with a constant 3x3x3 block planted at (11..13)^3: its centre (12,12,12) is degenerate"""
    npts = (25, 25, 25)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    phi = phi.copy(order="F")
    phi[11:14, 11:14, 11:14] = 0.25
    return phi, dx, npts


def test_degenerate_cell_gets_zero_and_is_counted():
    phi, dx, npts = _flat_case()
    ones = np.ones(npts, np.int32, order="F")
    res = C.curvature_band(phi, ones, dx, *_outs(npts))
    assert res.nonfinite == 0 and res.degenerate == 1 and res.cells == 23 ** 3
    assert res.kappa[12, 12, 12] == 0.0 and res.gauss[12, 12, 12] == 0.0 and res.gmag[12, 12, 12] == 0.0
    assert res.gmag[11, 12, 12] > 0.0  # its neighbours see the rim of the block: not degenerate
    one = np.zeros(npts, np.int32, order="F")
    one[12, 12, 12] = 1
    assert C.curvature_band(phi, one, dx, *_outs(npts))[3:] == (1, 1, 0, 0.0, 0)


def test_clamp_limits_every_value_and_is_counted():
    npts = (25, 25, 25)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    ones = np.ones(npts, np.int32, order="F")
    L = list_of(ones)
    free = C.curvature_band(phi, ones, dx, *_outs(npts))
    print(f"unclamped: largest |kappa| dx = {free.kappa_max * dx:.4g}")
    assert free.clamped == 0 and abs(free.kappa_max * dx - 10.8) < 0.05  # next to the centre of the sphere
    res = C.curvature_band(phi, ones, dx, *_outs(npts), clamp=1.0)
    lim = 1.0 / dx
    assert res.clamped > 0 and np.all(np.abs(res.kappa[L]) <= lim) and res.kappa_max == lim
    assert np.all(np.abs(res.gauss[L]) <= lim * lim) and np.array_equal(res.gmag, free.gmag, equal_nan=True)  # gmag is never clamped
    changed = (res.kappa != free.kappa) | (res.gauss != free.gauss)
    assert res.clamped == np.count_nonzero(changed[L])
    # without gauss only kappa counts
    konly = C.curvature_band(phi, ones, dx, _outs(npts)[0], clamp=1.0)
    assert konly.clamped == np.count_nonzero((res.kappa != free.kappa)[L]) <= res.clamped
    assert np.array_equal(konly.kappa, res.kappa, equal_nan=True)


def test_arguments_and_non_list_points_are_left_alone():
    npts = (14, 12, 13)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.6 * dx)
    mask[0, :, :] = 1  # a wall: ignored
    mask[5, 5, 5] = 7
    L = list_of(mask)
    outs = _outs(npts)
    outs[1][::2] = -7.0
    keep = [a.copy() for a in (phi, mask, *outs)]
    res = C.curvature_band(phi, mask, dx, *outs, clamp=1.0)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, (phi, mask, *outs)))  # the arguments are left alone
    for got, was in zip(res[:3], outs):
        assert np.array_equal(got[~L], was[~L], equal_nan=True) and np.all(np.isfinite(got[L]))
    assert res.cells == L.sum() and not L[5, 5, 5] and not L[0].any()
    assert res.gauss is not None and C.curvature_band(phi, mask, dx, outs[0]).gauss is None
    # an empty list: nothing written, everything zero
    walls = np.zeros(npts, np.int32, order="F")
    walls[0, :, :], walls[:, :, -1] = 1, 1
    e = C.curvature_band(phi, walls, dx, *outs)
    assert e[3:] == (0, 0, 0, 0.0, 0) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(e[:3], outs))


def test_nan_on_a_stencil_point_is_reported_with_its_count():
    npts = (14, 12, 13)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    only = np.zeros(npts, np.int32, order="F")
    only[6, 6, 6] = only[9, 6, 6] = 1
    bad = phi.copy(order="F")
    bad[7, 7, 6] = np.nan  # an edge diagonal of (6,6,6), no stencil point of (9,6,6)
    res = C.curvature_band(bad, only, dx, *_outs(npts))
    assert res.nonfinite == 1 and np.isnan(res.kappa[6, 6, 6]) and np.isnan(res.gauss[6, 6, 6])
    assert np.isfinite(res.gmag[6, 6, 6])  # |grad| has no mixed difference in it
    assert np.isfinite(res.kappa[9, 6, 6])
    # the clamp leaves a NaN a NaN; an infinite kappa is clamped to a finite one and is no error
    assert C.curvature_band(bad, only, dx, *_outs(npts), clamp=1.0).nonfinite == 1
    everywhere = C.curvature_band(bad, np.ones(npts, np.int32, order="F"), dx, _outs(npts)[0])
    assert everywhere.nonfinite == 19  # the cells whose 19-point stencil holds (7,7,6), itself included


# ---------------------------------------------------------------------------------- the Python layer
def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    k = np.full((6, 6, 6), -7.0, order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, None, 5, 5, 5, 0.1, k)
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, None)
    with pytest.raises(ValueError):
        lsf.curvatureBand(np.ones((6, 6, 5), order="F"), m, 5, 5, 5, 0.1, k)
    with pytest.raises(ValueError):
        lsf.curvatureBand(np.ones((6, 6, 6), order="C"), m, 5, 5, 5, 0.1, k)
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, np.ones((6, 5, 6), order="F"))
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k, gauss=np.ones((5, 6, 6), order="F"))
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k, gmag=np.ones((6, 6, 6), order="C"))
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, np.ones((6, 5, 6), np.int32, order="F"), 5, 5, 5, 0.1, k)
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k, clamp=-1.0)
    with pytest.raises(ValueError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k, clamp=float("nan"))
    with pytest.raises(TypeError):
        lsf.curvatureBand(phi.astype(np.float32), m, 5, 5, 5, 0.1, k)
    with pytest.raises(TypeError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k.astype(np.float32))
    with pytest.raises(TypeError):
        lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k, gauss=[[1.0]])
    with pytest.raises(TypeError):
        lsf.curvatureBand(phi, m.astype(np.int64), 5, 5, 5, 0.1, k)
    with pytest.raises(TypeError):
        lsf.curvatureBand(phi, m.astype(bool), 5, 5, 5, 0.1, k)
    assert np.all(phi == 1.0) and np.all(k == -7.0) and np.all(m == 1)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    k, g, a = (np.full((6, 6, 6), -7.0, order="F") for _ in range(3))
    for kw in (dict(), dict(gauss=g), dict(gauss=g, gmag=a, clamp=1.0)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.curvatureBand(phi, m, 5, 5, 5, 0.1, k, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(k == -7.0) and np.all(g == -7.0) and np.all(a == -7.0) and np.all(phi == 1.0)
