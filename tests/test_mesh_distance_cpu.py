"""lsf_mesh_distance / lsf_mesh_check without a GPU: the interface through every layer (header, bindings, Python, Fortran shim),
the host-only mesh check on the fixtures, argument validation before the library, no CPU fallback, and the sanity of the numpy
reference (tests/mesh_distance_ref.py) that the GPU tests compare with."""
import os
import re

import numpy as np
import pytest

import mesh_distance_ref as R
from conftest import GOLDEN, ROOT


def _header():
    txt = open(os.path.join(ROOT, "include", "lsf.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.fixture(scope="module")
def surfaces():
    s = np.load(os.path.join(GOLDEN, "surfaces.npz"))
    return {tag: (s[tag + "_surfX"].astype(np.float64), s[tag + "_surfElem"]) for tag in ("cube40", "twocube10")}


def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = _header()
    for name, nargs in (("lsf_mesh_check", 6), ("lsf_mesh_distance", 13), ("lsf_mesh_distance_device", 14)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_MESH_UNSIGNED\s+1\b", hdr) and re.search(r"#define\s+LSF_MESH_INFO_LEN\s+4\b", hdr)
    for name in ("meshDistance", "meshCheck"):
        assert callable(getattr(lsf, name)) and name in levelset.__all__
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_meshdistance():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bmeshDistance\b", public)
    assert "BIND(C,NAME='lsf_mesh_distance')" in src
    assert re.search(r"^SUBROUTINE meshDistance\(phi,nx,ny,nz,dx,xLo,surfX,nSurfNode,surfElem,nSurfElem,width\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_mesh_distance',rc)" in src


def test_mesh_check_on_the_fixtures(surfaces):
    import levelsetfortran_amd as lsf

    for tag, vol in (("cube40", 8.0), ("twocube10", 1.9999999404)):
        X, E = surfaces[tag]
        c = lsf.meshCheck(X, E)
        assert (c.degenerate_triangles, c.defective_edges) == (0, 0), tag
        assert abs(c.signed_volume - vol) <= 1e-9, (tag, c.signed_volume)
        assert abs(c.signed_volume - R.signed_volume(X, E)) <= 1e-12
    X, E = surfaces["twocube10"]
    assert lsf.meshCheck(X, np.delete(E, 5, axis=0)).defective_edges == 3  # a hole: its three sides have one triangle each
    flipped = E.copy()
    flipped[7] = flipped[7, [1, 0, 2]]
    c = lsf.meshCheck(X, flipped)
    assert (c.degenerate_triangles, c.defective_edges) == (0, 3)  # two triangles, but the same direction
    a, b = int(E[0, 0]), int(E[0, 1])
    c = lsf.meshCheck(X, np.vstack([E, [[a, a, b]]]))
    assert (c.degenerate_triangles, c.defective_edges) == (1, 0)  # skipped: part of no edge
    assert c.tube_points == 0 and c.triangles_off_grid == 0


def test_mesh_check_refuses_bad_input(surfaces):
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    X, E = surfaces["twocube10"]
    for Xb, Eb in ((X, np.where(E == 3, 0, E)), (X, np.where(E == 3, len(X) + 1, E)), (np.where(X == 12.0, np.inf, X), E)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.meshCheck(Xb, Eb)
        assert e.value.code == _lib.LSF_ERR_INVALID


def test_argument_validation_happens_before_the_library(surfaces):
    import levelsetfortran_amd as lsf

    X, E = surfaces["twocube10"]
    phi = np.ones((6, 6, 6), order="F")
    lo = (0.0, 0.0, 0.0)
    for kw in (dict(width=1.0), dict(width=float("nan")), dict(width=float("inf"))):
        with pytest.raises(ValueError):
            lsf.meshDistance(phi, 5, 5, 5, 0.1, lo, X, E, **kw)
    for dx in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            lsf.meshDistance(phi, 5, 5, 5, dx, lo, X, E)
    with pytest.raises(ValueError):
        lsf.meshDistance(np.ones((6, 6, 5), order="F"), 5, 5, 5, 0.1, lo, X, E)
    with pytest.raises(TypeError):
        lsf.meshDistance(phi.astype(np.float32), 5, 5, 5, 0.1, lo, X, E)
    with pytest.raises(ValueError):
        lsf.meshDistance(phi, 5, 5, 5, 0.1, (0.0, 0.0), X, E)
    with pytest.raises(ValueError):
        lsf.meshDistance(phi, 5, 5, 5, 0.1, lo, X[:, :2], E)
    with pytest.raises(ValueError):
        lsf.meshDistance(phi, 5, 5, 5, 0.1, lo, X, E[:0])
    with pytest.raises(TypeError):
        lsf.meshDistance(phi, 5, 5, 5, 0.1, lo, X, E.astype(np.float64))
    with pytest.raises(ValueError):
        lsf.meshCheck(X.T, E)
    assert np.all(phi == 1.0)


def test_no_cpu_fallback_without_device(surfaces):
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    X, E = surfaces["twocube10"]
    phi = np.ones((6, 6, 6), order="F")
    for signed in (True, False):
        with pytest.raises(lsf.LsfError) as e:
            lsf.meshDistance(phi, 5, 5, 5, 0.1, (0.0, 0.0, 0.0), X, E, signed=signed)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(phi == 1.0)


# ---------------------------------------------------------------------------------- the numpy reference itself
def _cube12(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    X = np.array([[(lo, hi)[(m >> a) & 1][a] for a in range(3)] for m in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]  # outward
    E = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32) + 1
    return X, E


def test_reference_against_the_closed_form_box():
    lo, hi = (-0.31, 0.12, -0.5), (0.52, 0.77, 0.245)
    X, E = _cube12(lo, hi)
    assert len(E) == 12 and abs(R.signed_volume(X, E) - np.prod(np.subtract(hi, lo))) < 1e-15
    n, dx, xLo = (23, 19, 21), 0.06, np.array((-0.71, -0.33, -0.93))
    P = R.grid_points(n, dx, xLo)
    sd = R.signed_distance(P, X, E)
    want = R.box_distance(P, lo, hi)
    assert (want < 0).sum() > 500 and np.abs(sd - want).max() < 1e-14
    assert np.array_equal(R.signed_distance(P, X, E, signed=False), np.abs(sd))
    # points exactly on faces, edges and corners (zero distance is positive), and the flipped cube
    Q = np.array([[0.0, 0.3, 0.0], [lo[0], 0.3, 0.0], [lo[0], lo[1], 0.0], list(lo), [lo[0] - 0.1, lo[1] - 0.1, lo[2] - 0.1]])
    assert np.allclose(R.signed_distance(Q, X, E), [R.box_distance(Q[0], lo, hi), 0, 0, 0, np.sqrt(0.03)], atol=1e-15)
    assert np.array_equal(R.signed_distance(P, X, E[:, [1, 0, 2]]), -sd)
    # clamp + column fill: the contract's field from the exact one
    far = 3.5 * dx
    f, tube = R.clamp_columns(sd, far)
    assert np.array_equal(f[tube], sd[tube]) and np.array_equal(f[~tube], np.where(want[~tube] < 0, -far, far))
    assert (f[~tube] < 0).sum() > 10  # interior far points exist and came out negative through the column rule


def test_reference_icosphere_within_the_sagitta_of_the_sphere():
    c, rad, dx = np.array((0.33, -0.27, 0.071)), 0.61, 0.07
    X, E = R.icosphere(2, rad, c)
    assert len(E) == 320 and len(X) == 162
    import levelsetfortran_amd as lsf

    chk = lsf.meshCheck(X, E)
    assert (chk.degenerate_triangles, chk.defective_edges) == (0, 0) and 0.9 < chk.signed_volume < 4.0 / 3.0 * np.pi * rad ** 3
    P = R.grid_points((27, 24, 29), dx, np.array((-1.02, -0.5, -0.93)))[::2, ::2, ::2]
    sd = R.signed_distance(P, X, E)
    gap = sd - (np.linalg.norm(P - c, axis=-1) - rad)  # the polyhedron is inscribed: never closer to the sphere's outside
    assert gap.min() > -1e-12 and gap.max() < 0.16 * dx  # (prototype: 0.155 dx on the full grid)
