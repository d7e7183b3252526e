"""lsf_distance_fill without a GPU: the interface through every layer, the serial restatement of the contract
(tests/distance_fill_ref.py: its three forms against each other, and the scheme against closed forms), argument validation before
the library, and no CPU fallback."""
import os
import re

import numpy as np
import pytest

import distance_fill_ref as R
from conftest import ROOT


def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_distance_fill", 12), ("lsf_distance_fill_device", 13)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert callable(lsf.distanceFill) and "distanceFill" in levelset.__all__ and "FillReport" in levelset.__all__
    assert lsf.FillReport._fields == ("rounds", "changed", "frozen_points", "converged")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_distancefill():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bdistanceFill\b", public)
    assert "BIND(C,NAME='lsf_distance_fill')" in src
    assert re.search(r"^SUBROUTINE distanceFill\(phi,nx,ny,nz,dx,band\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_distance_fill',rc)" in src


def _sphere_input(shape):
    ref = R.sphere_distance(R.grid_points(shape, 0.1, (-0.5, -0.4, -0.3)), (0.1, 0.05, 0.0), 0.3)
    return R.clamp(ref, 0.1, 1.5)


@pytest.mark.parametrize("shape", [(12, 9, 7), (8, 7, 3)])
def test_the_two_forms_agree_bit_for_bit(shape):
    f = _sphere_input(shape)
    keep = f.copy()
    for cap in (1, 64):
        a, ra, ta, na = R.fill_loops(f, 0.1, band=1.5, max_rounds=cap)
        b, rb, tb, nb = R.fill(f, 0.1, band=1.5, max_rounds=cap)
        assert np.array_equal(a, b) and ra == rb and ta == tb and na == nb
        assert np.isfinite(a).all() and ta[0] > 0  # after round 1 every point is finite
    assert ta[-1] == 0 and np.array_equal(f, keep)
    # the mask form of the same frozen set, the other points holding anything of the right sign
    m = (np.abs(f) < 1.5 * 0.1).astype(np.int32)
    g = np.where(m == 1, f, np.where(f < 0, -7.0, 7.0))
    c, rc, tc, nc = R.fill(g, 0.1, mask=m)
    assert np.array_equal(c, b) and (rc, tc, nc) == (rb, tb, nb)


@pytest.mark.parametrize("case,tile", [("tiny", (32, 8, 8)), ("thin", (32, 8, 8)), ("long", (32, 8, 8)), ("tiny", (4, 2, 2))])
def test_tile_plane_schedule_equals_the_raster_order(case, tile):
    """Tiles in hyperplane order, each on a private copy with the halo snapshot of its plane's start: the kernel's schedule.  One
    round pins the order (the fixed point would not); the small tile makes 2 x 4 x 2 tiles with partial ones out of the tiny input."""
    inp, width = R.CASES[case]
    ref, dx = R.exact(inp)
    f = R.clamp(ref, dx, width)
    a, ra, ta, _ = R.fill_tiles(f, dx, band=width, max_rounds=1, tile=tile)
    b, rb, tb, _ = R.fill(f, dx, band=width, max_rounds=1)
    assert ta == tb and ra == rb == 1 and np.array_equal(a, b)


# (case, rounds, max error in dx): the figures of the restatement, which are also those of the prototype the issue quotes
FIGURES = [("box35", 3, 0.98), ("box15", 3, 1.31), ("sphere35", 2, 1.40), ("sphere15", 2, 1.65)]


@pytest.mark.parametrize("case,rounds,err_dx", FIGURES)
def test_scheme_against_the_closed_forms(case, rounds, err_dx):
    inp, width = R.CASES[case]
    ref, dx = R.exact(inp)
    f = R.clamp(ref, dx, width)
    frozen = R.frozen_set(f, dx, band=width)
    assert R.check(f, frozen)[1:] == (0, 0)
    out, nr, trace, nfz = R.fill(f, dx, band=width)
    err = float(np.abs(out - ref).max() / dx)
    print(case, "rounds", nr, "trace", trace, "frozen", nfz, "max error", err, "dx")
    assert trace[-1] == 0 and nr == len(trace)
    assert np.array_equal(out < 0, ref < 0)
    assert np.array_equal(out[frozen], f[frozen]) and np.array_equal(out[frozen], ref[frozen]) and nfz == int(frozen.sum())
    assert err < 2.0  # a sanity bound on the scheme
    assert nr == rounds and abs(err - err_dx) < 0.006  # the recorded figures (rounded to 0.01)
    if case == "box35":
        assert nfz == 66282  # the tube of meshDistance(cube40, width 3.5)


def test_check_counts_what_the_library_refuses():
    f = _sphere_input((12, 9, 7))
    fz = R.frozen_set(f, 0.1, band=1.5)
    assert R.check(f, fz) == (int(fz.sum()), 0, 0)
    g = f.copy()
    i = tuple(np.argwhere(~fz & (f > 0))[0])
    g[i] = -g[i]  # a lone negative value among positive non-frozen neighbours
    assert R.check(g, fz)[2] >= 3
    g = f.copy()
    g[tuple(np.argwhere(fz)[0])] = np.nan
    assert R.check(g, fz)[1] == 1


def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    mask = np.ones((6, 6, 6), dtype=np.int32, order="F")
    with pytest.raises(ValueError):
        lsf.distanceFill(phi, 5, 5, 5, 0.1)
    with pytest.raises(ValueError):
        lsf.distanceFill(phi, 5, 5, 5, 0.1, band=2.0, mask=mask)
    with pytest.raises(ValueError):
        lsf.distanceFill(np.ones((6, 6, 5), order="F"), 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(ValueError):
        lsf.distanceFill(np.ones((6, 6, 6), order="C"), 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(ValueError):
        lsf.distanceFill(phi, 5, 5, 5, 0.1, mask=np.ones((6, 5, 6), dtype=np.int32, order="F"))
    with pytest.raises(TypeError):
        lsf.distanceFill(phi.astype(np.float32), 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(TypeError):
        lsf.distanceFill(phi, 5, 5, 5, 0.1, mask=mask.astype(np.int64))
    assert np.all(phi == 1.0)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    mask = np.ones((6, 6, 6), dtype=np.int32, order="F")
    for kw in (dict(band=2.0), dict(mask=mask)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.distanceFill(phi, 5, 5, 5, 0.1, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(phi == 1.0)
