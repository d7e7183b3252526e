"""lsf_mesh_distance on the GPU: the exact, clamped signed distance from the triangle mesh (include/lsf.h) against closed forms
(boxes) and the all-pairs numpy reference (tests/mesh_distance_ref.py).

Tolerance: the distance is about 50 well-conditioned fp64 operations on coordinates of magnitude L (the largest |coordinate| of
mesh and grid), a bound of about 1e-14 L; the tests use 1e-12 L absolute.  Tube membership is compared exactly; a point may be
left out of that comparison only where the REFERENCE value is within 1e-9 of the tube's edge, the references of these inputs have
no such point, and that is asserted too."""
import os

import numpy as np
import pytest

import mesh_distance_ref as R
import stl_io
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DX = 0.05
EDGE = 1.0e-9


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@pytest.fixture(scope="module")
def surfaces():
    s = np.load(os.path.join(GOLDEN, "surfaces.npz"))
    return {tag: (s[tag + "_surfX"].astype(np.float64), s[tag + "_surfElem"]) for tag in ("cube40", "twocube10")}


def _scale(X, n, dx, xLo):
    hi = np.asarray(xLo) + np.asarray(n) * dx
    return float(max(np.abs(X).max(), np.abs(xLo).max(), np.abs(hi).max()))


def _run(lsf, n, dx, xLo, X, E, width, **kw):
    phi = np.full(tuple(v + 1 for v in n), 7.0, order="F")
    info = lsf.meshDistance(phi, n[0], n[1], n[2], dx, xLo, X, E, width=width, **kw)
    return phi, info


def _check(phi, info, ref, far, tol, count):
    """The contract against an exact signed distance `ref` on the same grid."""
    edge = np.abs(np.abs(ref) - far) < EDGE
    assert edge.sum() == 0  # (the cap would be 0.1 % of the tube; these references have none at all)
    want, tube = R.clamp_columns(ref, far)
    assert np.array_equal(np.abs(phi) < far, tube)  # (a tube point could hold exactly far only on the edge, which is empty)
    err = float(np.abs(phi - want)[tube].max())
    print("tube", int(tube.sum()), "max abs error", err, "tolerance", tol)
    assert err <= tol
    assert np.array_equal(phi[~tube], want[~tube])  # exactly +-far, the sign of the reference (column rule == true sign here)
    assert np.array_equal(want[~tube], np.where(ref[~tube] < 0, -far, far))
    assert info.tube_points == int(tube.sum()) == count
    return tube


@pytest.fixture(scope="module")
def cube40_case(lsf, surfaces):
    X, E = surfaces["cube40"]
    n, xLo, mn, mx = stl_io.grid_from_surface(X)
    ref = R.box_distance(R.grid_points(n, DX, xLo), mn, mx)
    phi, info = _run(lsf, n, DX, xLo, X, E, 3.5)
    return X, E, n, xLo, ref, phi, info


def test_cube40_against_the_closed_form_box(cube40_case, cube40):
    X, E, n, xLo, ref, phi, info = cube40_case
    assert tuple(v + 1 for v in n) == (62, 62, 62)
    tube = _check(phi, info, ref, 3.5 * DX, 1e-12 * _scale(X, n, DX, xLo), 66282)
    assert info.degenerate_triangles == info.defective_edges == info.triangles_off_grid == 0
    sel = tube & (np.abs(ref) > EDGE)
    assert sel.sum() == 56680
    assert np.array_equal(phi[sel] < 0, cube40["phi0"][sel] < 0)  # the centroid test is right on this fixture


def test_twocube10_chunked_triangles_and_column_fill(lsf, surfaces):
    X, E = surfaces["twocube10"]
    n, xLo, mn, mx = stl_io.grid_from_surface(X)
    assert tuple(v + 1 for v in n) == (262, 42, 42)
    P = R.grid_points(n, DX, xLo)
    left, right = X[X[:, 0] < 5.0], X[X[:, 0] > 5.0]
    assert left[:, 0].max() == np.float64(np.float32(0.99999994))
    ref = np.minimum(R.box_distance(P, left.min(axis=0), left.max(axis=0)), R.box_distance(P, right.min(axis=0), right.max(axis=0)))
    phi, info = _run(lsf, n, DX, xLo, X, E, 3.5)
    tube = _check(phi, info, ref, 3.5 * DX, 1e-12 * _scale(X, n, DX, xLo), 33204)
    inner = ~tube & (ref < 0)
    assert inner.sum() == 4394 and np.all(phi[inner] == -3.5 * DX)


ICO = dict(n=(27, 24, 29), dx=0.07, xLo=np.array((-1.02, -0.5, -0.93)))


@pytest.fixture(scope="module")
def ico():
    X, E = R.icosphere(2, 0.61, (0.33, -0.27, 0.071))
    assert len(E) == 320
    P = R.grid_points(ICO["n"], ICO["dx"], ICO["xLo"])
    assert P.shape[:3] == (28, 25, 30)
    ref = R.signed_distance(P, X, E)
    assert X[:, 0].max() > P[-1, 0, 0, 0] and X[:, 1].min() < P[0, 0, 0, 1] and ref[:, :, 0].min() > 5.5 * ICO["dx"]
    return X, E, ref


@pytest.mark.parametrize("width,count", [(3.5, 4469), (1.5, 1953), (6.0, 7777)])
def test_icosphere_off_grid_through_two_walls(lsf, ico, width, count):
    X, E, ref = ico
    n, dx, xLo = ICO["n"], ICO["dx"], ICO["xLo"]
    phi, info = _run(lsf, n, dx, xLo, X, E, width)
    _check(phi, info, ref, width * dx, 1e-12 * _scale(X, n, dx, xLo), count)


def test_seams_reproducibility_and_unsigned(lsf, ico):
    import torch

    X, E, _ = ico
    n, dx, xLo = ICO["n"], ICO["dx"], ICO["xLo"]
    host, info = _run(lsf, n, dx, xLo, X, E, 3.5)
    again, _ = _run(lsf, n, dx, xLo, X, E, 3.5)
    assert np.array_equal(host, again)
    t = torch.full((host.size,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        info_d = lsf.meshDistance(t, n[0], n[1], n[2], dx, xLo, X, E, width=3.5)
    assert np.array_equal(t.cpu().numpy().reshape(host.shape, order="F"), host) and info_d == info
    uns, info_u = _run(lsf, n, dx, xLo, X, E, 3.5, signed=False)
    assert np.array_equal(uns, np.abs(host)) and info_u.tube_points == info.tube_points


def test_triangles_off_the_grid_and_degenerate_ones_change_nothing(lsf, ico):
    X, E, _ = ico
    n, dx, xLo = ICO["n"], ICO["dx"], ICO["xLo"]
    base, info = _run(lsf, n, dx, xLo, X, E, 3.5, signed=False)
    X2 = np.vstack([X, [[50.0, 50.0, 50.0], [51.0, 50.0, 50.0], [50.0, 51.0, 50.0]]])
    m = len(X)
    E2 = np.vstack([E, [[m + 1, m + 2, m + 3]], [[1, 1, 2]]]).astype(np.int32)
    got, info2 = _run(lsf, n, dx, xLo, X2, E2, 3.5, signed=False)
    assert np.array_equal(got, base)
    assert info2.degenerate_triangles == 1 and info2.triangles_off_grid == 1 and info2.tube_points == info.tube_points
    assert info2.defective_edges == 3  # the lone triangle's sides


def test_open_mesh_signed_refused_unsigned_exact(lsf, surfaces):
    from levelsetfortran_amd import _lib

    X, E = surfaces["cube40"]
    n, xLo, mn, mx = stl_io.grid_from_surface(X)
    hole = X[E[0] - 1].mean(axis=0)
    Eo = np.ascontiguousarray(E[1:])
    phi = np.full(tuple(v + 1 for v in n), 7.0, order="F")
    with pytest.raises(lsf.LsfError) as e:
        lsf.meshDistance(phi, n[0], n[1], n[2], DX, xLo, X, Eo, width=3.5)
    assert e.value.code == _lib.LSF_ERR_INVALID and "3 defective" in str(e.value) and np.all(phi == 7.0)
    info = lsf.meshDistance(phi, n[0], n[1], n[2], DX, xLo, X, Eo, width=3.5, signed=False)
    assert info.defective_edges == 3
    lo = np.clip(np.rint((hole - xLo) / DX).astype(int) - 10, 0, np.array(n) + 1 - 20)
    sub = tuple(slice(int(a), int(a) + 20) for a in lo)
    far = 3.5 * DX
    ref = R.signed_distance(R.grid_points(n, DX, xLo)[sub], X, Eo, signed=False, within=far)
    assert (np.abs(ref - far) < EDGE).sum() == 0
    want = np.minimum(ref, far)
    assert np.array_equal(phi[sub] < far, ref <= far) and (ref <= far).sum() > 1000
    err = float(np.abs(phi[sub] - want).max())
    print("open mesh, 20^3 around the hole: max abs error", err)
    assert err <= 1e-12 * _scale(X, n, DX, xLo)


def test_flipped_winding_negates_the_field(lsf, cube40_case):
    X, E, n, xLo, ref, phi, info = cube40_case
    flipped, info_f = _run(lsf, n, DX, xLo, X, np.ascontiguousarray(E[:, [1, 0, 2]]), 3.5)
    assert info_f.tube_points == info.tube_points
    err = float(np.abs(flipped + phi).max())  # (a point ON the surface may come out as 0 one way and as a rounding error the other)
    print("flipped winding: max |f + phi|", err)
    assert err <= 1e-12 * _scale(X, n, DX, xLo)
    far = ~(np.abs(phi) < 3.5 * DX)
    assert np.array_equal(flipped[far], -phi[far])  # the exterior sign follows the signed volume


def test_reinit_from_the_exact_distance_needs_far_fewer_sweeps(lsf, cube40_case, cube40):
    """The point of it.  Golden run from phi0 (the smeared centroid sign): 2155 sweeps.  The oracle started from the prototype's
    clamped exact distance stopped after 565.  Bound: at most half of the golden count."""
    X, E, n, xLo, ref, phi, info = cube40_case
    dx, h = float(cube40["dx"]), float(cube40["h"])
    golden = int(cube40["sweeps_reinit"])
    assert golden == 2155 and dx == DX
    f = np.array(phi, order="F")
    rep = lsf.reinit(f, None, None, n[0], n[1], n[2], 10000, dx, h, order="gs", arith="strict")
    print("reinit from meshDistance(width=3.5):", rep.count, "sweeps; from phi0:", golden)
    assert rep.converged and 2 * rep.count <= golden


def test_errors_on_the_device_path_leave_phi_alone(lsf, ico):
    import torch

    from levelsetfortran_amd import _lib

    X, E, _ = ico
    n, dx, xLo = ICO["n"], ICO["dx"], ICO["xLo"]
    lib = _lib.load()
    sX, sE = np.asfortranarray(X), np.asfortranarray(E, dtype=np.int32)
    lo = np.ascontiguousarray(xLo)
    t = torch.full(((n[0] + 1) * (n[1] + 1) * (n[2] + 1),), 7.0, dtype=torch.float64, device="cuda")

    def call(dx_=dx, width=3.5, sX_=sX, sE_=sE):
        return lib.lsf_mesh_distance_device(t.data_ptr(), n[0], n[1], n[2], dx_, lo.ctypes.data, sX_.ctypes.data, sX_.shape[0],
                                            sE_.ctypes.data, sE_.shape[0], width, 0, None, None)

    bad0, badn, nanX = sE.copy(order="F"), sE.copy(order="F"), sX.copy(order="F")
    bad0[5, 1], badn[7, 2], nanX[3, 0] = 0, len(X) + 1, np.nan
    for kw in (dict(width=1.0), dict(width=float("nan")), dict(dx_=0.0), dict(dx_=-0.1), dict(sE_=bad0), dict(sE_=badn), dict(sX_=nanX)):
        assert call(**kw) == _lib.LSF_ERR_INVALID, kw
        assert bool((t == 7.0).all()), kw
    assert call() == _lib.LSF_OK and not bool((t == 7.0).any())
