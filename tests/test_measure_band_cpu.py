"""lsf_measure_band without a GPU: the interface through every layer, properties of the serial statement of the contract
(tests/measure_ref.py), argument validation before the library, and no CPU fallback."""
import math
import os
import re

import numpy as np
import pytest

import advect_ref as R
import curvature_ref as C
import extract_ref as X
import measure_ref as MR
from advect_band_ref import list_of
from conftest import ROOT

CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6  # the sphere of tests/test_gpu_curvature_band.py, grid over [-1.5, 1.5]^3
LO = (-1.5, -1.5, -1.5)
AREA, VOLUME = 4. * math.pi * RADIUS ** 2, 4. / 3. * math.pi * RADIUS ** 3


def _mask(cond):
    return np.asfortranarray(cond.astype(np.int32))


def _ones(npts):
    return np.ones(npts, np.int32, order="F")


# ---------------------------------------------------------------------------------- the interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_measure_band", 12), ("lsf_measure_band_device", 13)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_MEASURE_LEN\s+9\b", hdr) and _lib.LSF_MEASURE_LEN == 9
    assert re.search(r"#define\s+LSF_MEASURE_INFO_LEN\s+5\b", hdr) and _lib.LSF_MEASURE_INFO_LEN == 5
    assert callable(lsf.measureBand) and "measureBand" in levelset.__all__ and "MeasureReport" in levelset.__all__
    assert lsf.MeasureReport._fields == ("area", "volume", "centroid", "surface_centroid", "q_integral", "cells", "crossed", "triangles", "open",
                                         "degenerate")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_measureband():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bmeasureBand\b", public)
    assert "BIND(C,NAME='lsf_measure_band')" in src
    assert re.search(r"^SUBROUTINE measureBand\(phi,mask,nx,ny,nz,dx,xLo,iso,M\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_measure_band',rc)" in src
    assert re.search(r"^!\s+measureBand\(phi,mask,nx,ny,nz,dx,xLo,iso,M\)", src, flags=re.M)  # the header comment's list of procedures


# ---------------------------------------------------------------------------------- the statement against the extraction statement
def test_statement_measures_the_triangles_the_extraction_emits():
    """every interior point listed: the same crossed cells and triangles as extract_ref.extract, and area and signed volume of that
    mesh, computed by whole-array numpy from its nodes and connectivity, to the accuracy of the sums"""
    npts = (19, 17, 15)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    phi = np.asfortranarray(phi + X.wavy(npts, dx))  # all seven edge types, every tetrahedron pattern
    res = MR.measure_band(phi, _ones(npts), dx, LO)
    Xn, E, info = X.extract(phi, dx, LO)
    assert res.crossed == info[2] > 0 and res.triangles == info[1] and res.open == 0 and res.degenerate == 0
    P = [Xn[E[:, v].astype(np.int64) - 1] for v in range(3)]
    n = np.cross(P[1] - P[0], P[2] - P[0])
    a = 0.5 * np.sqrt((n * n).sum(axis=1))
    v = (P[0] * np.cross(P[1], P[2])).sum(axis=1) / 6.
    # the cell sums round once per triangle, the products of the mesh formulas a few times more: 8 u per term is generous
    for k, terms in ((0, a), (1, v)):
        tol = 8 * len(E) * 2. ** -53 * math.fsum(np.abs(terms))
        print(f"quantity {k}: statement {res.M[k]!r}, mesh {math.fsum(terms)!r}, tolerance {tol:.3g}")
        assert abs(res.M[k] - math.fsum(terms)) <= tol
    assert res.M[1] > 0  # the normals point outward
    am, vm, _ = MR.mesh_measures(Xn, E)
    assert abs(am - res.M[0]) <= MR.summation_bound(res, 0) + res.triangles * 2. ** -53 * res.abs_sum[0]
    assert abs(vm - res.M[1]) <= MR.summation_bound(res, 1) + res.triangles * 2. ** -53 * res.abs_sum[1]


def _sphere(N, mask_of=None, **kw):
    npts = (N, N, N)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _ones(npts) if mask_of is None else _mask(mask_of(phi, dx))
    return MR.measure_band(phi, mask, dx, LO, **kw), phi, mask, dx


def test_sphere_is_second_order():
    """The figures the extraction statement gives on this sphere: area 1.12 % low at 25^3 and 0.28 % at 49^3, volume 2.17 % and 0.54 %,
    the surface centroid 1.45e-5 and 1.50e-6 from the centre (the polyhedron is inscribed: both measures come out low)."""
    r25, r49 = _sphere(25)[0], _sphere(49)[0]
    low = lambda got, exact: 100. * (1. - got / exact)
    a25, a49, v25, v49 = low(r25.M[0], AREA), low(r49.M[0], AREA), low(r25.M[1], VOLUME), low(r49.M[1], VOLUME)
    off = lambda r: max(abs(r.M[5 + A] / r.M[0] - CENTRE[A]) for A in range(3))
    voff = lambda r: max(abs(r.M[2 + A] / r.M[1] - CENTRE[A]) for A in range(3))
    print(f"area low {a25:.4f} % / {a49:.4f} %, volume low {v25:.4f} % / {v49:.4f} %, surface centroid off {off(r25):.3e} / {off(r49):.3e}, "
          f"body centroid off {voff(r25):.3e} / {voff(r49):.3e}")
    assert abs(a25 - 1.12) < 0.005 and abs(a49 - 0.28) < 0.005
    assert abs(v25 - 2.17) < 0.005 and abs(v49 - 0.54) < 0.005
    assert a25 / a49 >= 3.9 and v25 / v49 >= 3.9
    assert off(r25) < 1.55e-5 and off(r49) < 1.55e-6  # 1.5e-5 and 1.5e-6 to the two digits quoted
    assert voff(r25) < 1.55e-5 and voff(r49) < 1.55e-6
    assert r25.open == r49.open == 0 and r25.degenerate == r49.degenerate == 0
    assert (r25.cells, r25.crossed, r25.triangles) == (23 ** 3, 420, 2508)


def test_a_band_mask_gives_the_same_cells_as_every_interior_point():
    full, phi, _, dx = _sphere(25)
    band = MR.measure_band(phi, _mask(np.abs(phi) < 2.1 * dx), dx, LO)
    assert np.array_equal(band.cells_c0, full.cells_c0) and np.array_equal(band.contrib, full.contrib) and band.M == full.M
    assert band.cells == 1286 and band.triangles == full.triangles
    assert band.open > 0  # crossed cells next to the rim of a band this thin: the flag is about the list, not about the surface


def test_half_space_cut_is_open_and_smaller():
    full, phi, _, dx = _sphere(25)
    half = np.zeros(phi.shape, bool)
    half[:13] = True  # a half-space through the sphere
    cut = MR.measure_band(phi, _mask(half), dx, LO)
    assert cut.open > 0 and 0 < cut.crossed < full.crossed and 0 < cut.M[0] < full.M[0]
    assert abs(cut.M[0] / full.M[0] - 0.5) < 0.1


def test_exact_zeros_on_grid_points_give_zero_area_triangles():
    from levelsetfortran_amd import fields

    npts = (9, 8, 7)
    x, y, z, dx = fields.grid_axes(npts)
    phi = np.asfortranarray(np.broadcast_to((x - x[4])[:, None, None], npts))  # phi == 0 on the grid plane i = 4
    assert np.count_nonzero(phi == 0.0) == npts[1] * npts[2]
    res = MR.measure_band(phi, _ones(npts), dx, (x[0], y[0], z[0]))
    ncell = (npts[1] - 2) * (npts[2] - 2)  # the measured cells i = 3 whose upper face is the plane
    assert res.crossed == ncell and res.degenerate > 0 and res.triangles > res.degenerate
    assert abs(res.M[0] - ncell * dx * dx) < 1e-12  # the zero-area triangles add nothing
    out = np.full(npts, np.nan, order="F")
    got = MR.measure_band(phi, _ones(npts), dx, (x[0], y[0], z[0]), cell_area=out).cell_area
    assert np.all(np.abs(got[3, 1:-1, 1:-1] - dx * dx) < 1e-15) and np.count_nonzero(got[1:-1, 1:-1, 1:-1]) == ncell


def test_iso_selects_the_level():
    npts = (25, 25, 25)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    iso = 0.125
    a = MR.measure_band(phi, _ones(npts), dx, LO, iso=iso)
    b = MR.measure_band(np.asfortranarray(phi - iso), _ones(npts), dx, LO)  # the same f, bit for bit
    assert a.M == b.M and a.info == b.info and np.array_equal(a.contrib, b.contrib)
    zero = MR.measure_band(phi, _ones(npts), dx, LO)
    exact = 4. * math.pi * (RADIUS + iso) ** 2
    assert a.M[0] > zero.M[0] and abs(a.M[0] / exact - 1.) < 0.012


def test_q_equal_one_integrates_to_the_area_bit_for_bit():
    npts = (25, 25, 25)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    phi = np.asfortranarray(phi + X.wavy(npts, dx))
    res = MR.measure_band(phi, _ones(npts), dx, LO, q=np.ones(npts, order="F"))
    assert res.crossed > 0 and np.array_equal(res.contrib[:, 8], res.contrib[:, 0]) and res.M[8] == res.M[0]
    none = MR.measure_band(phi, _ones(npts), dx, LO)
    assert np.all(none.contrib[:, 8] == 0.0) and none.M[8] == 0.0 and np.array_equal(none.contrib[:, :8], res.contrib[:, :8])


def test_linear_q_against_the_closed_form():
    """a linear q is interpolated exactly along an edge, and the mean of its vertex values is its value at a triangle's centroid:
    the integral is c0 * area + c . (surface moments); on the sphere that is q(centre) * area"""
    from levelsetfortran_amd import fields

    res0, phi, mask, dx = _sphere(25)
    x, y, z, _ = fields.grid_axes(phi.shape)
    c0, c = 0.7, (0.3, -1.1, 0.45)
    q = np.asfortranarray(c0 + c[0] * x[:, None, None] + c[1] * y[None, :, None] + c[2] * z[None, None, :])
    res = MR.measure_band(phi, mask, dx, (x[0], y[0], z[0]), q=q)
    want = c0 * res.M[0] + sum(c[A] * res.M[5 + A] for A in range(3))
    assert abs(res.M[8] - want) < 1e-13 * res.abs_sum[8]
    at_centre = c0 + sum(c[A] * CENTRE[A] for A in range(3))
    assert abs(res.M[8] / (at_centre * AREA) - 1.) < 0.0115  # the area's own 1.12 %


def _gauss_bonnet(N):
    npts = (N, N, N)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.1 * dx)
    nan = lambda: np.full(npts, np.nan, order="F")
    K = C.curvature_band(phi, mask, dx, nan(), nan()).gauss  # NaN off the list
    assert np.isnan(K[~list_of(mask)]).all()
    return MR.measure_band(phi, mask, dx, LO, q=K).M[8] / (4. * math.pi)


def test_gauss_bonnet_on_the_sphere():
    """the integral of the Gaussian curvature of lsf_curvature_band over the surface, / 4 pi = chi / 2 = 1 for a sphere: 1.00893 at 25^3 and
    1.00200 at 49^3 (the two statements composed), second order"""
    g25, g49 = _gauss_bonnet(25), _gauss_bonnet(49)
    print(f"Gauss-Bonnet: {g25:.6f} at 25^3, {g49:.6f} at 49^3, factor {(g25 - 1.) / (g49 - 1.):.3f}")
    assert abs(g25 - 1.00893) < 5e-6 and abs(g49 - 1.00200) < 5e-6
    assert (g25 - 1.) / (g49 - 1.) >= 4.4


def test_cell_area_is_written_at_list_points_only_and_arguments_are_left_alone():
    npts = (14, 12, 13)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.6 * dx)
    mask[0, :, :] = 1  # a wall: ignored
    mask[5, 5, 5] = 7
    L = list_of(mask)
    out = np.full(npts, np.nan, order="F")
    out[::2] = -7.0
    q = np.asfortranarray(np.where(np.abs(phi) < 2.6 * dx, 1.5, np.nan))  # NaN away from the crossed edges, wall points included
    keep = [a.copy() for a in (phi, mask, q, out)]
    res = MR.measure_band(phi, mask, dx, LO, q=q, cell_area=out)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, (phi, mask, q, out)))
    assert np.array_equal(res.cell_area[~L], out[~L], equal_nan=True) and np.all(res.cell_area[L] >= 0.0)
    assert np.count_nonzero(res.cell_area[L]) == res.crossed and math.fsum(res.cell_area[L]) == res.M[0]
    assert res.cells == L.sum() and not L[5, 5, 5] and not L[0].any()
    assert MR.measure_band(phi, mask, dx, LO).cell_area is None
    # an empty list, and a list without a crossed cell: zeros
    walls = np.zeros(npts, np.int32, order="F")
    walls[0, :, :], walls[:, :, -1] = 1, 1
    e = MR.measure_band(phi, walls, dx, LO, cell_area=out)
    assert e.M == (0.0,) * 9 and e.info == [0] * 5 and np.array_equal(e.cell_area, out, equal_nan=True)
    one = np.zeros(npts, np.int32, order="F")
    one[1, 1, 1] = 1
    f = MR.measure_band(phi, one, dx, LO, cell_area=out)
    assert f.M == (0.0,) * 9 and f.info == [1, 0, 0, 0, 0] and f.cell_area[1, 1, 1] == 0.0


def test_every_rule_of_the_statement_that_refuses():
    npts = (14, 12, 13)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.6 * dx)
    q = np.ones(npts, order="F")
    ok = dict(phi=phi, mask=mask, dx=dx, xLo=LO, iso=0.0, q=q, cell_area=np.zeros(npts, order="F"))
    MR.measure_band(**ok)
    bad = {
        "dx = 0": dict(dx=0.0), "dx < 0": dict(dx=-dx), "dx NaN": dict(dx=float("nan")), "dx inf": dict(dx=float("inf")),
        "iso NaN": dict(iso=float("nan")), "iso inf": dict(iso=float("inf")),
        "xLo NaN": dict(xLo=(0.0, float("nan"), 0.0)), "xLo inf": dict(xLo=(float("inf"), 0.0, 0.0)),
        "nx < 2": dict(phi=phi[:2], mask=mask[:2], q=q[:2], cell_area=np.zeros((2,) + npts[1:], order="F")),
        "cell_area is phi": dict(cell_area=phi), "cell_area is q": dict(cell_area=q), "cell_area overlaps phi": dict(cell_area=phi[:, :, ::-1][:, :, ::-1]),
    }
    for name, change in bad.items():
        with pytest.raises(MR.Invalid):
            MR.measure_band(**dict(ok, **change))
    # non-finite values: refused on an endpoint of a crossed edge of a measured cell, with the count; legal anywhere else
    res = MR.measure_band(phi, mask, dx, LO)
    c0 = tuple(res.cells_c0[len(res.cells_c0) // 2])
    far = tuple(np.argwhere(np.abs(phi[1:-1, 1:-1, 1:-1]) > 4.5 * dx)[0] + 1)  # an interior point, a corner of no measured cell
    for name in ("phi", "q"):
        for val in (np.nan, np.inf, -np.inf):
            a = ok[name].copy(order="F")
            a[far] = val
            MR.measure_band(**dict(ok, **{name: a}))  # on no crossed edge of a measured cell
            a[c0] = val
            with pytest.raises(MR.Invalid) as e:
                MR.measure_band(**dict(ok, **{name: a}))
            assert e.value.count >= 1 and str(e.value).startswith(f"{e.value.count} crossed edge") and ("phi - iso" if name == "phi" else " q ") in str(e.value)
    # q off the list may be NaN: what lsf_curvature_band leaves
    qn = np.asfortranarray(np.where(np.abs(phi) < 2.6 * dx, 1.0, np.nan))
    assert MR.measure_band(phi, mask, dx, LO, q=qn).M[8] == res.M[0]
    # both non-finite: phi is reported
    a, b = phi.copy(order="F"), q.copy(order="F")
    a[c0] = b[c0] = np.nan
    with pytest.raises(MR.Invalid, match="phi - iso"):
        MR.measure_band(a, mask, dx, LO, q=b)


# ---------------------------------------------------------------------------------- the Python layer
def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    a = np.full((6, 6, 6), -7.0, order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    lo = (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        lsf.measureBand(phi, None, 5, 5, 5, 0.1, lo)
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, (0.0, 0.0))
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, (0.0, float("nan"), 0.0))
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.0, lo)
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, float("inf"), lo)
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, lo, iso=float("nan"))
    with pytest.raises(ValueError):
        lsf.measureBand(np.ones((6, 6, 5), order="F"), m, 5, 5, 5, 0.1, lo)
    with pytest.raises(ValueError):
        lsf.measureBand(np.ones((6, 6, 6), order="C"), m, 5, 5, 5, 0.1, lo)
    with pytest.raises(ValueError):
        lsf.measureBand(phi, np.ones((6, 5, 6), np.int32, order="F"), 5, 5, 5, 0.1, lo)
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, lo, q=np.ones((6, 5, 6), order="F"))
    with pytest.raises(ValueError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, lo, cell_area=np.ones((6, 6, 6), order="C"))
    with pytest.raises(TypeError):
        lsf.measureBand(phi.astype(np.float32), m, 5, 5, 5, 0.1, lo)
    with pytest.raises(TypeError):
        lsf.measureBand(phi, m.astype(np.int64), 5, 5, 5, 0.1, lo)
    with pytest.raises(TypeError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, lo, q=a.astype(np.float32))
    with pytest.raises(TypeError):
        lsf.measureBand(phi, m, 5, 5, 5, 0.1, lo, cell_area=[[1.0]])
    assert np.all(phi == 1.0) and np.all(a == -7.0) and np.all(m == 1)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    q, a = (np.full((6, 6, 6), -7.0, order="F") for _ in range(2))
    for kw in (dict(), dict(q=q), dict(q=q, cell_area=a, iso=0.5)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.measureBand(phi, m, 5, 5, 5, 0.1, (0.0, 0.0, 0.0), **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(q == -7.0) and np.all(a == -7.0) and np.all(phi == 1.0) and np.all(m == 1)
