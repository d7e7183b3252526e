"""lsf_extract_surface / lsf_stl_write without a GPU: the interface through every layer (header, bindings, Python, Fortran shim),
argument validation before the library, no CPU fallback, lsf_stl_write against both STL readers, and the sanity of the numpy statement
(tests/extract_ref.py) that the GPU tests compare with.

The fields.  fields.sphere_phi0 returns the SMEARED sign d / sqrt(d^2 + dx^2) of the distance d (its docstring), whose linear
interpolant along an edge misses the zero of d by O(dx), not O(dx^2): measured on the statement, the largest node error of the
radius-0.7 sphere is 0.026 / 0.014 / 0.0071 at 17 / 33 / 65 points per axis, halving with dx.  The node bound below "follows from
linear interpolation of an exact distance", so the tests recover that distance, d = dx * phi / sqrt(1 - phi^2), from the field
(`distance_of`); the zero level set is the same.  two_sphere_phi0 is taken at 65 points per axis: its bodies are 0.2 apart, and the
bound's premise -- both endpoints of a crossed edge measure their distance to the same sphere -- needs sqrt(3) dx < 0.1.
"""
import os
import re

import numpy as np
import pytest

import extract_ref as R
import stl_io
from conftest import ROOT
from levelsetfortran_amd import fields

LO = (-1.5, -1.5, -1.5)
CENTRE, RADIUS = (0.13, -0.08, 0.21), 0.7


def distance_of(phi, dx):
    """The distance d that fields.sphere_phi0 smeared into phi = d / sqrt(d^2 + dx^2)."""
    return np.asfortranarray(dx * phi / np.sqrt(1.0 - phi * phi))


def sphere(n, radius=RADIUS, centre=CENTRE):
    phi, dx = fields.sphere_phi0((n, n, n), centers=(centre,), radius=radius)
    return distance_of(phi, dx), dx


def node_bound(dx, r):
    """| |p - c| - r | of a node: linear interpolation of an exact distance along an edge no longer than sqrt(3) dx."""
    return 3.0 * dx * dx / (8.0 * (r - np.sqrt(3.0) * dx)) + 1e-12


def signed_volume(X, E):
    a, b, c = (X[E[:, q] - 1] for q in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


@pytest.fixture(scope="module")
def sphere33():
    phi, dx = sphere(33)
    X, E, info = R.extract(phi, dx, LO)
    return phi, dx, X, E, info


def _header():
    txt = open(os.path.join(ROOT, "include", "lsf.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


# ---------------------------------------------------------------------------------- interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = _header()
    for name, nargs in (("lsf_extract_surface", 10), ("lsf_extract_surface_device", 11), ("lsf_extract_get", 2), ("lsf_extract_get_device", 3),
                        ("lsf_stl_write", 5)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_SURF_INFO_LEN\s+4\b", hdr) and _lib.LSF_SURF_INFO_LEN == 4
    for name in ("extractSurface", "stlWrite", "SurfaceInfo"):
        assert hasattr(lsf, name) and name in levelset.__all__
    assert callable(lsf.extractSurface) and callable(lsf.stlWrite)
    assert lsf.SurfaceInfo._fields == ("nodes", "triangles", "cells_crossed", "nodes_on_grid_points")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_extractsurface_and_stlwrite():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bextractSurface\b", public) and re.search(r"\bstlWrite\b", public)
    for name in ("lsf_extract_surface", "lsf_extract_get", "lsf_stl_write"):
        assert "BIND(C,NAME='%s')" % name in src
        assert "CALL lsf_fail('%s',rc)" % name in src
    assert re.search(r"^SUBROUTINE extractSurface\(phi,nx,ny,nz,dx,xLo,iso,surfX,nSurfNode,surfElem,nSurfElem\)", src, flags=re.M)
    assert re.search(r"^SUBROUTINE stlWrite\(", src, flags=re.M)
    body = src[src.index("SUBROUTINE extractSurface("):src.index("END SUBROUTINE extractSurface")]
    assert re.search(r"REAL,ALLOCATABLE,DIMENSION\(:,:\),INTENT\(OUT\) :: surfX", body)
    assert re.search(r"INTEGER\*4,ALLOCATABLE,DIMENSION\(:,:\),INTENT\(OUT\) :: surfElem", body)


def test_argument_validation_happens_before_the_library(tmp_path):
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    for dx in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lsf.extractSurface(phi, 5, 5, 5, dx, LO)
    for iso in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lsf.extractSurface(phi, 5, 5, 5, 0.1, LO, iso=iso)
    with pytest.raises(ValueError):
        lsf.extractSurface(phi, 5, 5, 5, 0.1, (0.0, 0.0))
    with pytest.raises(ValueError):
        lsf.extractSurface(np.ones((6, 6, 5), order="F"), 5, 5, 5, 0.1, LO)
    with pytest.raises(ValueError):
        lsf.extractSurface(np.ones((6, 6, 6)), 5, 5, 5, 0.1, LO)  # C-ordered
    with pytest.raises(ValueError):
        lsf.extractSurface(np.ones((1, 6, 6), order="F"), 0, 5, 5, 0.1, LO)
    with pytest.raises(TypeError):
        lsf.extractSurface(phi.astype(np.float32), 5, 5, 5, 0.1, LO)
    X = np.zeros((3, 3))
    E = np.array([[1, 2, 3]], dtype=np.int32)
    out = str(tmp_path / "never.stl")
    with pytest.raises(ValueError):
        lsf.stlWrite(out, X[:, :2], E)
    with pytest.raises(ValueError):
        lsf.stlWrite(out, X, E[:0])
    with pytest.raises(TypeError):
        lsf.stlWrite(out, X, E.astype(np.float64))
    assert not os.path.exists(out) and np.all(phi == 1.0)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi, dx = sphere(9)
    with pytest.raises(lsf.LsfError) as e:
        lsf.extractSurface(phi, 8, 8, 8, dx, LO)
    assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert _lib.load().lsf_extract_get(None, None) == _lib.LSF_ERR_INVALID  # nothing was kept


# ---------------------------------------------------------------------------------- lsf_stl_write
def test_stl_write_against_both_readers(sphere33, tmp_path):
    import ctypes

    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    _, _, X, E, _ = sphere33
    path = str(tmp_path / "sphere.stl")
    lsf.stlWrite(path, X, E)
    X32 = X.astype(np.float32)
    assert len(np.unique(X32, axis=0)) == len(X)  # no two nodes round to the same REAL*4 triple: the readers merge nothing
    # what a reader must return: the rounded nodes renumbered in the order of their first use
    order = E.ravel()  # C order of (nTri,3): triangle by triangle, vertex by vertex
    _, first = np.unique(order, return_index=True)
    old_of_new = order[np.sort(first)]
    new_of_old = np.zeros(len(X) + 1, dtype=np.int32)
    new_of_old[old_of_new] = np.arange(1, len(old_of_new) + 1)
    assert len(old_of_new) == len(X)
    wantX, wantE = X32[old_of_new - 1].astype(np.float64), new_of_old[E]

    lib = _lib.load()
    ne, nn = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.lsf_stl_read(os.fsencode(path), ctypes.byref(ne), ctypes.byref(nn)))
    assert (ne.value, nn.value) == (len(E), len(X))
    gX, gE = np.zeros((nn.value, 3), order="F"), np.zeros((ne.value, 3), dtype=np.int32, order="F")
    _lib.check(lib.lsf_stl_get(gX.ctypes.data, gE.ctypes.data))
    pX, pE = stl_io.stl_read(path)
    assert len(pX) == len(gX) == len(X)
    assert np.array_equal(gE, wantE) and np.array_equal(pE, wantE)
    assert np.array_equal(gX, wantX) and np.array_equal(pX, wantX)  # the float32 rounding, exactly

    raw = open(path, "rb").read()
    assert len(raw) == 84 + 50 * len(E) and not raw.startswith(b"solid")
    assert int(np.frombuffer(raw, dtype="<i4", count=1, offset=80)[0]) == len(E)
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("pad", "<i2")]), offset=84)
    assert np.array_equal(rec["v"], X32[E - 1]) and np.all(rec["pad"] == 0)
    v = rec["v"].astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    assert np.array_equal(rec["n"], nrm.astype(np.float32))  # computed in double from the rounded vertices
    assert np.abs(np.linalg.norm(rec["n"].astype(np.float64), axis=1) - 1.0).max() < 2e-7  # unit, to REAL*4
    outward = v.mean(axis=1) - np.asarray(CENTRE)
    assert ((rec["n"] * outward).sum(axis=1) > 0).all()


def test_stl_write_zero_area_triangle_and_errors(tmp_path):
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    X = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]])
    E = np.array([[1, 2, 3], [1, 2, 4], [1, 1, 2]], dtype=np.int32)  # the last two have no area
    path = str(tmp_path / "flat.stl")
    lsf.stlWrite(path, X, E)
    rec = np.frombuffer(open(path, "rb").read(), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("pad", "<i2")]), offset=84)
    assert np.array_equal(rec["n"], np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0]], dtype=np.float32))

    lib = _lib.load()
    Xf, Ef = np.asfortranarray(X), np.asfortranarray(E)
    bad = str(tmp_path / "bad.stl")

    def call(p, x, nn, e, ne):
        return lib.lsf_stl_write(p, x.ctypes.data if x is not None else None, nn, e.ctypes.data if e is not None else None, ne)

    cases = [(None, Xf, 4, Ef, 3), (os.fsencode(bad), None, 4, Ef, 3), (os.fsencode(bad), Xf, 4, None, 3),
             (os.fsencode(bad), Xf, 4, Ef, 0), (os.fsencode(bad), Xf, 0, Ef, 3),
             (os.fsencode(bad), Xf, 4, np.asfortranarray(np.where(E == 4, 5, E)), 3),  # an index above nSurfNode
             (os.fsencode(bad), Xf, 4, np.asfortranarray(np.where(E == 3, 0, E)), 3),  # an index below 1
             (os.fsencode(bad), np.asfortranarray(np.where(X == 2.0, np.nan, X)), 4, Ef, 3),
             (os.fsencode(bad), np.asfortranarray(np.where(X == 2.0, np.inf, X)), 4, Ef, 3)]
    for c in cases:
        assert call(*c) == _lib.LSF_ERR_INVALID, c[2:]
        assert not os.path.exists(bad)  # refused before the file is opened
    assert call(os.fsencode(str(tmp_path / "no_such_dir" / "x.stl")), Xf, 4, Ef, 3) == _lib.LSF_ERR_INVALID  # an unwritable path
    assert b"no_such_dir" in lib.lsf_last_error()
    with pytest.raises(lsf.LsfError):
        lsf.stlWrite(bad, X, np.where(E == 4, 7, E))


# ---------------------------------------------------------------------------------- the statement itself
def _closed_outward(X, E):
    import levelsetfortran_amd as lsf

    assert len(R.open_edges(E)) == 0  # every edge: two triangles, opposite directions
    c = lsf.meshCheck(X, E)
    assert (c.degenerate_triangles, c.defective_edges) == (0, 0) and c.signed_volume > 0
    assert abs(c.signed_volume - signed_volume(X, E)) <= 1e-12
    return c.signed_volume


def test_statement_on_the_off_centre_sphere(sphere33):
    phi, dx, X, E, info = sphere33
    assert not (phi == 0.0).any()
    assert info[:2] == [len(X), len(E)] and info[3] == 0 and info[2] > 0
    assert X.flags.f_contiguous and E.flags.f_contiguous and E.dtype == np.int32 and E.min() == 1 and E.max() == len(X)
    assert len(X) - 3 * len(E) // 2 + len(E) == 2  # Euler: one sphere
    _closed_outward(X, E)
    err = np.abs(np.linalg.norm(X - np.asarray(CENTRE), axis=1) - RADIUS)
    assert err.max() <= node_bound(dx, RADIUS), (err.max(), node_bound(dx, RADIUS))


def test_statement_on_two_spheres():
    phi, dx = fields.two_sphere_phi0((65, 65, 65))
    phi = distance_of(phi, dx)
    assert not (phi == 0.0).any()
    X, E, info = R.extract(phi, dx, LO)
    vol = _closed_outward(X, E)
    assert R.components(len(X), E) == 2 and abs(vol - 2 * 4.0 / 3.0 * np.pi * 0.5 ** 3) < 0.01
    err = np.minimum(*(np.abs(np.linalg.norm(X - np.array((cx, 0.0, 0.0)), axis=1) - 0.5) for cx in (-0.6, 0.6)))
    assert err.max() <= node_bound(dx, 0.5), (err.max(), node_bound(dx, 0.5))


def test_statement_volume_converges_at_second_order():
    # measured on the statement: errors 5.135e-2, 1.288e-2, 3.219e-3 at 17, 33, 65 points per axis,
    # ratios 3.986 and 4.002.  The floor: one quarter below the smaller measured ratio (and no lower than 2).
    floor = max(3.986 - 0.25, 2.0)
    exact = 4.0 / 3.0 * np.pi * RADIUS ** 3
    errs = []
    for n in (17, 33, 65):
        phi, dx = sphere(n)
        assert not (phi == 0.0).any()
        X, E, _ = R.extract(phi, dx, LO)
        errs.append(exact - signed_volume(X, E))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("volume errors", errs, "ratios", ratios)
    assert all(e > 0 for e in errs) and min(ratios) >= floor, (errs, ratios)


def test_statement_iso_level(sphere33):
    phi, dx, *_ = sphere33
    assert not (phi == 0.1).any()
    X, E, info = R.extract(phi, dx, LO, iso=0.1)
    _closed_outward(X, E)
    err = np.abs(np.linalg.norm(X - np.asarray(CENTRE), axis=1) - (RADIUS + 0.1))
    assert err.max() <= node_bound(dx, RADIUS + 0.1), (err.max(), node_bound(dx, RADIUS + 0.1))


def tilted_plane(shape, dx):
    x, y, z = (LO[a] + dx * np.arange(shape[a]) for a in range(3))
    return np.asfortranarray(0.31 * x[:, None, None] - 0.52 * y[None, :, None] + 0.8 * z[None, None, :] + 0.0123)


def test_statement_open_plane_has_its_boundary_in_the_walls():
    shape, dx = (14, 11, 12), 0.25
    phi = tilted_plane(shape, dx)
    assert not (phi == 0.0).any()
    X, E, info = R.extract(phi, dx, LO)
    lo_hi, use = R.edge_use(E)
    assert (use.sum(axis=1) <= 2).all() and (use.max(axis=1) <= 1).all()  # never more than two triangles, never twice the same way
    rim = R.open_edges(E)
    assert len(rim) > 0
    hi = np.asarray(LO) + dx * (np.asarray(shape) - 1)
    a, b = X[rim[:, 0] - 1], X[rim[:, 1] - 1]
    on_wall = ((a == np.asarray(LO)) & (b == np.asarray(LO))) | ((a == hi) & (b == hi))  # both ends in the same wall face
    assert on_wall.any(axis=1).all()
    assert R.components(len(X), E) == 1


def test_statement_empty_and_exact_zero(sphere33):
    X, E, info = R.extract(np.ones((5, 4, 6), order="F"), 0.1, LO)
    assert X.shape == (0, 3) and E.shape == (0, 3) and info == [0, 0, 0, 0]
    phi, dx, *_ = sphere33
    planted = phi.copy(order="F")
    # an outside point next to the surface becomes an exact zero; the last such point has inside neighbours BELOW it, whose edges
    # end on it with t == 1 (seen from the zero itself an edge starts with t == 0, which info[3] does not count)
    i, j, k = np.argwhere((phi > 0) & (phi < 0.5 * dx))[-1]
    planted[i, j, k] = 0.0
    X, E, info = R.extract(planted, dx, LO)
    assert info[3] >= 1 and len(R.open_edges(E)) == 0  # coincident nodes, zero-area triangles, the connectivity still closed
    import levelsetfortran_amd as lsf

    c = lsf.meshCheck(X, E)
    assert c.degenerate_triangles >= 1  # lsf_mesh_check skips them: it may then report their neighbours' edges
    with pytest.raises(R.NonFinite) as e:
        bad = phi.copy(order="F")
        bad[i, j, k] = np.nan
        R.extract(bad, dx, LO)
    assert e.value.count >= 1
