"""lsf_cut_cells_band without a GPU: the interface through every layer, properties of the serial statement of the contract
(tests/cut_cells_ref.py), argument validation before the library, and no CPU fallback.

The cap on a cell's own rounding, 64 * 2^-53 (cut_cells_ref.CAP), is derived: at most 18 triangles with a handful of roundings each
on magnitudes <= 1.  What the statement shows on the `general` input (printed by the tests): closedness 2 * 2^-53, the fraction
against the per-tetrahedron closed forms 2 * 2^-53, the summed volume against measure_ref's 1.3e-16 relative."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import advect_ref as R
import cut_cells_ref as CC
import extract_ref as X
import measure_ref as MR
from advect_band_ref import list_of
from conftest import ROOT

CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6  # the sphere of tests/test_measure_band_cpu.py, grid over [-1.5, 1.5]^3
LO = (-1.5, -1.5, -1.5)
VOLUME = 4. / 3. * math.pi * RADIUS ** 3
U = CC.U


def _mask(cond):
    return np.asfortranarray(cond.astype(np.int32))


def _ones(npts):
    return np.ones(npts, np.int32, order="F")


def _corners(f, c0):
    return [float(f[c0[0] + (o & 1), c0[1] + (o >> 1 & 1), c0[2] + (o >> 2 & 1)]) for o in range(8)]


def _general():
    npts = (19, 17, 15)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    return np.asfortranarray(phi + X.wavy(npts, dx)), dx, npts


def _fields(npts, n, fill=np.nan):
    return tuple(np.full(npts, fill, order="F") for _ in range(n))


# ---------------------------------------------------------------------------------- the interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_cut_cells_band", 17), ("lsf_cut_cells_band_device", 18)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_CUT_INFO_LEN\s+5\b", hdr) and _lib.LSF_CUT_INFO_LEN == 5
    assert callable(lsf.cutCellsBand) and "cutCellsBand" in levelset.__all__ and "CutCellsReport" in levelset.__all__
    assert lsf.CutCellsReport._fields == ("volume", "vof_min", "cells", "cut", "full", "open", "clamped")
    csrc = os.path.join(ROOT, "levelsetfortran_amd", "csrc")
    for h in ("lsf_cut_cells_band.hpp", "lsf_host_cut_cells_band.hpp", "lsf_host_args_cut.hpp"):
        assert os.path.exists(os.path.join(csrc, h)), h


def test_versions_do_not_move():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_cutcellsband():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bcutCellsBand\b", public)
    assert "BIND(C,NAME='lsf_cut_cells_band')" in src
    assert re.search(r"^SUBROUTINE cutCellsBand\(phi,mask,nx,ny,nz,dx,iso,vof,ax,ay,az,volume\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_cut_cells_band',rc)" in src
    assert re.search(r"^!\s+cutCellsBand\(phi,mask,nx,ny,nz,dx,iso,vof,ax,ay,az,volume\)", src, flags=re.M)  # the list of procedures


# ---------------------------------------------------------------------------------- the input
def test_the_general_input_has_every_edge_type_and_tetrahedron_pattern():
    """all seven edge types at either level; of the 6 x 14 crossed tetrahedron patterns the level 0 lacks one, (4, 9), and the level
    0.0625 of the GPU matrix another, (5, 9): between them every pattern occurs"""
    phi, dx, npts = _general()
    missing = {}
    for iso in (0.0, 0.0625):
        types, codes = X.census(phi, iso)
        assert all(n > 0 for n in types), types
        missing[iso] = {(t, code) for t in range(6) for code in range(1, 15) if codes[t][code] == 0}
    assert missing == {0.0: {(4, 9)}, 0.0625: {(5, 9)}}, missing
    res = CC.cut_cells_band(phi, _ones(npts), dx)
    assert res.info == [17 * 15 * 13, 250, 96, 0, 0]


# ---------------------------------------------------------------------------------- properties of the statement
def test_the_inside_part_of_a_cell_is_closed():
    """per cut cell and axis the surface's area vector balances the apertures: b_A = lower_A - upper_A within the cap"""
    phi, dx, npts = _general()
    res = CC.cut_cells_band(phi, _ones(npts), dx)
    worst = max(abs(c.b[A] - (c.low[A] - c.up[A])) for c in res.cut_cells for A in range(3))
    print(f"closedness: largest |b_A - (lower_A - upper_A)| over {res.cut} cut cells = {worst / U:.3g} * 2^-53 (cap 64)")
    assert res.cut == 250 and worst <= CC.CAP


def test_the_divergence_form_equals_the_closed_forms_per_tetrahedron():
    phi, dx, npts = _general()
    res = CC.cut_cells_band(phi, _ones(npts), dx)
    worst = max(abs(CC.tetrahedra_fraction(_corners(phi, c0)) - c.raw) for c0, c in zip(res.cells_c0, res.cut_cells))
    print(f"cross-check: largest |raw - closed forms| over {res.cut} cut cells = {worst / U:.3g} * 2^-53 (cap 64)")
    assert worst <= CC.CAP
    assert all(0.0 < c.raw < 1.0 and not c.clamped for c in res.cut_cells)
    # an uncut cell through the same closed forms
    assert CC.tetrahedra_fraction([1.0] * 8) == 0.0 and CC.tetrahedra_fraction([-1.0] * 8) == 1.0


def test_upper_face_of_a_cell_is_the_lower_face_of_its_neighbour_bit_for_bit():
    phi, dx, npts = _general()
    ap = _fields(npts, 3)
    res = CC.cut_cells_band(phi, _ones(npts), dx, aperture=ap)
    lst = list_of(_ones(npts))
    seen = 0
    for c0, c in zip(res.cells_c0, res.cut_cells):
        for A in range(3):
            nb = tuple(int(c0[B]) + (B == A) for B in range(3))
            if lst[nb]:  # (the neighbour may be uncut: 0.0 or 1.0 then, through the same function)
                assert res.aperture[A][nb] == c.up[A], (c0, A)
                seen += 1
    assert seen > 700


def test_the_summed_fractions_are_the_volume_measure_band_reports():
    """the same polyhedron, once as a sum over cells in cell units and once as a surface integral about the frame's origin: the
    difference lies within 8 u per term of each side's own absolute sum, plus the cap per cut cell"""
    phi, dx, npts = _general()
    res = CC.cut_cells_band(phi, _ones(npts), dx)
    mr = MR.measure_band(phi, _ones(npts), dx, LO)
    Xn, E, _ = X.extract(phi, dx, LO)
    P = [Xn[E[:, v].astype(np.int64) - 1] for v in range(3)]
    terms = (P[0] * np.cross(P[1], P[2])).sum(axis=1) / 6.
    d3 = (dx * dx) * dx
    tol = 8 * len(E) * U * math.fsum(np.abs(terms)) + (8 * np.count_nonzero(res.stored) * U * res.abs_sum + res.cut * CC.CAP) * d3
    err = abs(res.volume - mr.M[1])
    print(f"sum vof dx^3 {res.volume!r}, measure_ref M[1] {mr.M[1]!r}, relative difference {err / mr.M[1]:.3g}, tolerance {tol:.3g}")
    assert mr.triangles == len(E) and res.cut == mr.crossed and err <= tol


def test_sphere_is_second_order_and_the_polyhedron_of_measure_band():
    low = {}
    for N in (25, 49):
        npts = (N, N, N)
        phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
        res = CC.cut_cells_band(phi, _ones(npts), dx)
        low[N] = 100. * (1. - res.volume / VOLUME)
        assert res.open == 0 and res.clamped == 0
    print(f"volume low {low[25]:.4f} % / {low[49]:.4f} %")
    assert abs(low[25] - 2.17) < 0.005 and abs(low[49] - 0.54) < 0.005 and low[25] / low[49] >= 3.9


def _box_fraction(a, d):
    """the fraction of the unit box in len(a) dimensions with a . x < d, every a_i > 0"""
    k = len(a)
    if d >= sum(a):  # the whole box (the alternating sum below would cancel powers of a large d)
        return 1.0
    tot = 0.0
    for S in itertools.product((0, 1), repeat=k):
        r = d - sum(ai for ai, s in zip(a, S) if s)
        if r > 0.0:
            tot += (-1) ** sum(S) * r ** k
    return tot / (math.factorial(k) * math.prod(a))


def test_an_oblique_plane_gives_the_analytic_plane_cube_fractions():
    """f = n . (x - x0), n = (1,2,3)/sqrt(14): linear, so the interpolant is exact and vof and the apertures are the plane-cube and
    plane-square fractions.  Tolerance: a corner value carries an error of about u F (F the largest |f|), an edge fraction divides
    it by an edge's own change of f, at least n_min dx, and the fractions are polynomials of degree <= 3 in those with coefficient
    sums of a few units: 64 u F / (n_min dx), plus the cap."""
    from levelsetfortran_amd import fields

    npts = (12, 11, 10)
    x, y, z, dx = fields.grid_axes(npts)
    n = tuple(v / math.sqrt(14.) for v in (1., 2., 3.))
    x0 = (0.013, -0.021, 0.017)
    phi = np.asfortranarray(n[0] * (x[:, None, None] - x0[0]) + n[1] * (y[None, :, None] - x0[1]) + n[2] * (z[None, None, :] - x0[2]))
    ap = _fields(npts, 3)
    vof = _fields(npts, 1)[0]
    res = CC.cut_cells_band(phi, _ones(npts), dx, vof=vof, aperture=ap)
    tol = 64 * U * float(np.abs(phi).max()) / (min(n) * dx) + CC.CAP
    ax = (x, y, z)
    worst = 0.0
    lst = list_of(_ones(npts))
    for c0 in np.argwhere(lst):
        c0 = tuple(int(v) for v in c0)
        d = -sum(n[A] * (ax[A][c0[A]] - x0[A]) for A in range(3)) / dx  # in cell units: n . xi < d
        worst = max(worst, abs(res.vof[c0] - _box_fraction(n, d)))
        for A in range(3):
            others = [n[B] for B in range(3) if B != A]
            worst = max(worst, abs(res.aperture[A][c0] - _box_fraction(others, d)))
    print(f"oblique plane: {res.cut} cut cells, largest difference from the analytic fractions {worst:.3g}, tolerance {tol:.3g}")
    assert res.cut > 100 and res.full > 100 and worst <= tol


def test_complement():
    """-f swaps inside and outside (no exact zeros): a(-f) = 1 - a(f) and vof(-f) = 1 - vof(f) within the cap"""
    phi, dx, npts = _general()
    assert np.count_nonzero(phi == 0.0) == 0
    res = CC.cut_cells_band(phi, _ones(npts), dx)
    worst = 0.0
    for c0, c in zip(res.cells_c0, res.cut_cells):
        m = CC.cell([-v for v in _corners(phi, c0)])
        assert m.byte == 255 - c.byte
        worst = max([worst, abs(m.raw - (1.0 - c.raw))] + [abs(m.low[A] - (1.0 - c.low[A])) for A in range(3)]
                    + [abs(m.up[A] - (1.0 - c.up[A])) for A in range(3)] + [abs(m.b[A] + c.b[A]) for A in range(3)])
    print(f"complement: largest difference {worst / U:.3g} * 2^-53 (cap 64)")
    assert worst <= CC.CAP


# ---------------------------------------------------------------------------------- coverage
def test_exact_zeros_on_a_grid_plane():
    from levelsetfortran_amd import fields

    npts = (9, 8, 7)
    x, y, z, dx = fields.grid_axes(npts)
    phi = np.asfortranarray(np.broadcast_to((x - x[4])[:, None, None], npts))  # phi == 0 on the grid plane i = 4: outside
    assert np.count_nonzero(phi == 0.0) == npts[1] * npts[2]
    vof = _fields(npts, 1)[0]
    ap, bv = _fields(npts, 3), _fields(npts, 3)
    res = CC.cut_cells_band(phi, _ones(npts), dx, vof=vof, aperture=ap, area_vector=bv)
    ncell = (npts[1] - 2) * (npts[2] - 2)
    assert res.cut == ncell and res.full == 2 * ncell and res.clamped == 0  # the cells i = 3 are cut by their own upper face
    inner = (slice(1, -1),) * 2
    assert np.all(res.vof[3][inner] == 1.0) and res.vof_min == 1.0  # ... and wholly inside
    assert np.all(res.aperture[0][3][inner] == 1.0) and np.all(res.aperture[0][4][inner] == 0.0)  # the plane itself is closed
    assert np.all(res.area_vector[0][3][inner] == 1.0) and np.all(res.area_vector[1][3][inner] == 0.0)
    assert np.all(res.vof[4:-1, 1:-1, 1:-1] == 0.0)
    assert abs(res.volume - 3 * ncell * dx ** 3) < 1e-15


def _sliver(npts=(7, 6, 6)):
    dx = 0.25
    phi = np.full(npts, 0.3 * dx, order="F")
    phi[3, 3, 3] = -1e-12 * dx  # one grid point inside by 1e-12 dx: a corner of eight cells
    return phi, dx, npts


def test_a_sliver_gives_a_tiny_non_negative_fraction_and_reports_its_clamps():
    phi, dx, npts = _sliver()
    res = CC.cut_cells_band(phi, _ones(npts), dx)
    raws = [c.raw for c in res.cut_cells]
    print(f"sliver: raw fractions {raws}, clamped {res.clamped}, vof_min {res.vof_min!r}")
    assert res.cut == 8 and res.full == 0
    assert res.clamped == sum(r < 0.0 or r > 1.0 for r in raws)
    assert 0.0 <= res.vof_min < 1e-30 and all(0.0 <= c.vof < 1e-20 for c in res.cut_cells)
    assert any(c.vof > 0.0 for c in res.cut_cells)  # the cell whose own lower corner is inside keeps its fraction
    assert 0.0 <= res.volume < 1e-20


def test_iso_is_the_shifted_field_bit_for_bit():
    phi, dx, npts = _general()
    iso = 0.0625
    out = lambda: dict(vof=_fields(npts, 1)[0], aperture=_fields(npts, 3), area_vector=_fields(npts, 3))
    a = CC.cut_cells_band(phi, _ones(npts), dx, iso=iso, **out())
    b = CC.cut_cells_band(np.asfortranarray(phi - iso), _ones(npts), dx, **out())
    same = lambda p, q: np.array_equal(p.view(np.uint64), q.view(np.uint64))
    assert a.info == b.info and a.volume == b.volume and a.vof_min == b.vof_min and same(a.vof, b.vof)
    assert all(same(p, q) for p, q in zip(a.aperture + a.area_vector, b.aperture + b.area_vector))
    zero = CC.cut_cells_band(phi, _ones(npts), dx)
    assert a.volume > zero.volume and a.cut != zero.cut


def test_outputs_are_written_at_list_points_only_and_arguments_are_left_alone():
    npts = (14, 12, 13)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(phi < 2.1 * dx)
    mask[0, :, :] = 1  # a wall: ignored
    mask[7, 6, 6] = 7
    L = list_of(mask)
    outs = _fields(npts, 7)
    for a in outs:
        a[::2] = -7.0
    keep = [a.copy() for a in (phi, mask) + outs]
    res = CC.cut_cells_band(phi, mask, dx, vof=outs[0], aperture=outs[1:4], area_vector=outs[4:7])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, (phi, mask) + outs))
    got = (res.vof,) + res.aperture + res.area_vector
    for g, o in zip(got, outs):
        assert np.array_equal(g[~L], o[~L], equal_nan=True) and np.isfinite(g[L]).all()
    assert np.all((res.vof[L] >= 0.0) & (res.vof[L] <= 1.0)) and res.cells == L.sum() and not L[7, 6, 6] and not L[0].any()
    assert res.volume == math.fsum(res.vof[L]) * ((dx * dx) * dx) and res.full == np.count_nonzero(res.vof[L] == 1.0)
    assert res.open > 0  # some cut cell has a face neighbour outside the list
    none = CC.cut_cells_band(phi, mask, dx)
    assert none.vof is None and none.aperture is None and none.area_vector is None and none.volume == res.volume
    # an empty list
    walls = np.zeros(npts, np.int32, order="F")
    walls[0, :, :], walls[:, :, -1] = 1, 1
    e = CC.cut_cells_band(phi, walls, dx, vof=outs[0])
    assert e.info == [0] * 5 and e.volume == 0.0 and e.vof_min == math.inf and np.array_equal(e.vof, outs[0], equal_nan=True)


def test_every_rule_of_the_statement_that_refuses():
    npts = (14, 12, 13)
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = _mask(np.abs(phi) < 2.6 * dx)
    o = _fields(npts, 7, 0.0)
    ok = dict(phi=phi, mask=mask, dx=dx, iso=0.0, vof=o[0], aperture=o[1:4], area_vector=o[4:7])
    res = CC.cut_cells_band(**ok)
    bad = {
        "dx = 0": dict(dx=0.0), "dx < 0": dict(dx=-dx), "dx NaN": dict(dx=float("nan")), "dx inf": dict(dx=float("inf")),
        "iso NaN": dict(iso=float("nan")), "iso inf": dict(iso=float("inf")),
        "nx < 2": dict(phi=phi[:2], mask=mask[:2], vof=None, aperture=None, area_vector=None),
        "aperture 2 of 3": dict(aperture=(o[1], None, o[3])), "area vector 1 of 3": dict(area_vector=(o[4], None, None)),
        "vof is phi": dict(vof=phi), "ax is vof": dict(aperture=(o[0], o[2], o[3])), "by is bx": dict(area_vector=(o[4], o[4], o[6])),
        "bz overlaps phi": dict(area_vector=(o[4], o[5], phi[:, :, ::-1][:, :, ::-1])),
    }
    for name, change in bad.items():
        with pytest.raises(MR.Invalid):
            CC.cut_cells_band(**dict(ok, **change))
    # non-finite values: refused on an endpoint of a crossed edge of a listed cell, with the count; legal anywhere else
    c0 = tuple(res.cells_c0[len(res.cells_c0) // 2])
    far = tuple(np.argwhere(np.abs(phi[1:-1, 1:-1, 1:-1]) > 4.5 * dx)[0] + 1)  # an interior point, a corner of no listed cell
    for val in (np.nan, np.inf, -np.inf):
        a = phi.copy(order="F")
        a[far] = val
        assert CC.cut_cells_band(**dict(ok, phi=a)).info == res.info
        a[c0] = val
        with pytest.raises(MR.Invalid) as e:
            CC.cut_cells_band(**dict(ok, phi=a))
        assert e.value.count >= 1 and str(e.value).startswith(f"{e.value.count} crossed edge") and "phi - iso" in str(e.value)
        with pytest.raises(MR.Invalid) as m:  # the count is lsf_measure_band's
            MR.measure_band(a, mask, dx, LO)
        assert m.value.count == e.value.count


# ---------------------------------------------------------------------------------- the Python layer
def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    a, b, c = (np.full((6, 6, 6), -7.0, order="F") for _ in range(3))
    m = np.ones((6, 6, 6), np.int32, order="F")
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, None, 5, 5, 5, 0.1)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.0, vof=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, float("inf"), vof=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, iso=float("nan"), vof=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(np.ones((6, 6, 5), order="F"), m, 5, 5, 5, 0.1, vof=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(np.ones((6, 6, 6), order="C"), m, 5, 5, 5, 0.1, vof=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, np.ones((6, 5, 6), np.int32, order="F"), 5, 5, 5, 0.1, vof=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, vof=np.ones((6, 5, 6), order="F"))
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, aperture=(a, b))
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, aperture=(a, b, None))
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, area_vector=a)
    with pytest.raises(ValueError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, area_vector=(a, b, np.ones((6, 6, 6), order="C")))
    with pytest.raises(TypeError):
        lsf.cutCellsBand(phi.astype(np.float32), m, 5, 5, 5, 0.1, vof=a)
    with pytest.raises(TypeError):
        lsf.cutCellsBand(phi, m.astype(np.int64), 5, 5, 5, 0.1, vof=a)
    with pytest.raises(TypeError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, vof=a.astype(np.float32))
    with pytest.raises(TypeError):
        lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, aperture=(a, b, [[1.0]]))
    assert np.all(phi == 1.0) and all(np.all(v == -7.0) for v in (a, b, c)) and np.all(m == 1)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    o = [np.full((6, 6, 6), -7.0, order="F") for _ in range(7)]
    for kw in (dict(), dict(vof=o[0]), dict(vof=o[0], aperture=o[1:4], area_vector=o[4:7], iso=0.5)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.cutCellsBand(phi, m, 5, 5, 5, 0.1, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    # the C call: the scalars keep their sentinels too
    lib = _lib.load()
    tot, info = np.full(2, -7.0), np.full(5, -7, np.int64)
    rc = lib.lsf_cut_cells_band(phi.ctypes.data, m.ctypes.data, 5, 5, 5, 0.1, 0.0, *(a.ctypes.data for a in o), tot.ctypes.data,
                                tot.ctypes.data + 8, info.ctypes.data)
    assert rc == _lib.LSF_ERR_NO_DEVICE and np.all(tot == -7.0) and np.all(info == -7)
    assert all(np.all(a == -7.0) for a in o) and np.all(phi == 1.0) and np.all(m == 1)
