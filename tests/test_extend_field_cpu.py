"""lsf_extend_field without a GPU: the interface through every layer, the serial restatement of the contract (tests/extend_ref.py:
its three forms against each other, the scheme against a closed form and on a clamped field), argument validation before the
library, and no CPU fallback."""
import os
import re

import numpy as np
import pytest

import distance_fill_ref as D
import extend_ref as E
from conftest import ROOT


def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_extend_field", 13), ("lsf_extend_field_device", 14)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_EXTEND_INFO_LEN\s+3\b", hdr) and _lib.LSF_EXTEND_INFO_LEN == 3
    assert callable(lsf.extendField) and "extendField" in levelset.__all__ and "ExtendReport" in levelset.__all__
    assert lsf.ExtendReport._fields == ("rounds", "changed", "frozen_points", "reached", "unreached", "converged")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_extendfield():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bextendField\b", public)
    assert "BIND(C,NAME='lsf_extend_field')" in src
    assert re.search(r"^SUBROUTINE extendField\(q,phi,nx,ny,nz,dx,band\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_extend_field',rc)" in src


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and a[1:] == b[1:]


@pytest.mark.parametrize("shape", [(12, 9, 7), (8, 7, 3)])
def test_the_three_forms_agree_bit_for_bit(shape):
    phi = D.sphere_distance(D.grid_points(shape, 0.1, (-0.5, -0.4, -0.3)), (0.1, 0.05, 0.0), 0.3)
    frozen = E.frozen_set(phi, 0.1, band=1.5)
    q = np.where(frozen, E.quantity(shape, 0.1), 7.0)
    q[tuple(np.argwhere(~frozen)[3])] = np.nan  # ignored
    keep_q, keep_phi = q.copy(), phi.copy()
    for cap in (1, 64):
        a = E.extend_loops(q, phi, 0.1, band=1.5, max_rounds=cap)
        b = E.extend(q, phi, 0.1, band=1.5, max_rounds=cap)
        c = E.extend_tiles(q, phi, 0.1, band=1.5, max_rounds=cap, tile=(4, 2, 2))
        assert _same(a, b) and _same(a, c)
        assert a[2][0] > 0 and a[3] == (int(frozen.sum()), int((~frozen).sum()), 0)
        assert np.array_equal(a[0][frozen], q[frozen])
    assert a[2][-1] == 0 and a[1] == len(a[2])
    assert np.array_equal(q, keep_q, equal_nan=True) and np.array_equal(phi, keep_phi)
    # the mask form of the same frozen set
    m = frozen.astype(np.int32)
    assert _same(E.extend(q, phi, 0.1, mask=m), b)
    assert E.check(q, phi, frozen) == (int(frozen.sum()), 0, 0)


@pytest.mark.parametrize("case,tile", [("tiny", (32, 8, 8)), ("thin", (32, 8, 8)), ("long", (32, 8, 8)), ("tiny", (4, 2, 2))])
def test_tile_plane_schedule_equals_the_raster_order(case, tile):
    """Tiles in hyperplane order, each on a private copy with the halo snapshot of its plane's start: the kernel's schedule.  One
    round pins the order (the fixed point would not); the small tile makes 2 x 4 x 2 tiles with partial ones out of the tiny input."""
    q, phi, dx, band = E.inputs(case)
    a = E.extend_tiles(q, phi, dx, band=band, max_rounds=1, tile=tile)
    assert a[1] == 1 and _same(a, E.want(case, 1))


def test_constant_along_the_normal_exactly():
    """phi = (i - 7.5) dx and frozen values from {0, +-0.5, +-1, +-2, +-4}: every w is a multiple of dx by a small integer, every
    product and quotient is exact, and one axis is used -- so each point holds, with ==, the frozen value of its own (j, k) row on
    its own side."""
    shape, dx = (16, 6, 5), np.float64(0.25)
    phi = np.broadcast_to(((np.arange(16) - 7.5) * dx)[:, None, None], shape).copy()
    frozen = E.frozen_set(phi, dx, band=1.5)
    assert np.array_equal(np.flatnonzero(frozen[:, 0, 0]), [7, 8])
    rng = np.random.default_rng(5)
    vals = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0])
    q = np.full(shape, 7.0)
    q[7:9] = vals[rng.integers(0, len(vals), size=(2,) + shape[1:])]
    out, rounds, trace, info = E.extend(q, phi, dx, band=1.5)
    assert rounds == 2 and trace[-1] == 0 and info[2] == 0 and info[0] + info[1] == phi.size
    assert (out[:8] == q[7]).all() and (out[8:] == q[8]).all()
    assert _same(E.extend_loops(q, phi, dx, band=1.5), (out, rounds, trace, info))


# N -> (max error over phi > 0, trace): the figures of the restatement, which are also those of the prototype the issue quotes
FIGURES = {21: (0.0464, [27053, 0]), 41: (0.0288, [205753, 0])}


@pytest.fixture(scope="module")
def sphere_errors():
    out = {}
    for N in FIGURES:
        q, phi, dx = E.sphere_case(N)
        got, rounds, trace, info = E.extend(q, phi, dx, band=1.5)
        frozen = E.frozen_set(phi, dx, band=1.5)
        err = float(np.abs(got - q)[phi > 0].max())
        print("N", N, "max error", err, "rounds", rounds, "trace", trace, "info", info)
        assert rounds == len(trace) == 2 and info[2] == 0 and not np.isnan(got).any()
        assert np.array_equal(got[frozen], q[frozen])
        assert got.min() >= q[frozen].min() and got.max() <= q[frozen].max()  # a convex combination of frozen values
        out[N] = (err, trace)
    return out


@pytest.mark.parametrize("N", sorted(FIGURES))
def test_scheme_against_the_closed_form(sphere_errors, N):
    err, trace = sphere_errors[N]
    assert trace == FIGURES[N][1] and abs(err - FIGURES[N][0]) < 0.0006  # the recorded figures (rounded)


def test_scheme_converges_under_refinement(sphere_errors):
    ratio = sphere_errors[21][0] / sphere_errors[41][0]
    print("ratio", ratio)
    assert ratio >= 1.3  # no convergence gives <= 1, first order tends to 2; 1.61 observed


def test_a_plateau_is_left_unreached_and_reported():
    q, phi, dx = E.sphere_case(21, clamp_cells=3)
    out, rounds, trace, info = E.extend(q, phi, dx, band=1.5)
    frozen = E.frozen_set(phi, dx, band=1.5)
    nan = np.isnan(out)
    print("rounds", rounds, "trace", trace, "info", info)
    assert info[2] == int(nan.sum()) == 6705 and info[2] > 0 and trace == [4021, 0]
    assert info[0] + info[1] + info[2] == out.size == 9261
    assert np.isfinite(out[~nan]).all() and not nan[frozen].any()
    assert (np.abs(phi[nan]) == 3 * dx).all()  # the plateau, and the ring of it that touches the tube is reached


def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    q = np.ones((6, 6, 6), order="F")
    phi = np.ones((6, 6, 6), order="F")
    mask = np.ones((6, 6, 6), dtype=np.int32, order="F")
    with pytest.raises(ValueError):
        lsf.extendField(q, phi, 5, 5, 5, 0.1)
    with pytest.raises(ValueError):
        lsf.extendField(q, phi, 5, 5, 5, 0.1, band=2.0, mask=mask)
    with pytest.raises(ValueError):
        lsf.extendField(np.ones((6, 6, 5), order="F"), phi, 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(ValueError):
        lsf.extendField(q, np.ones((6, 6, 5), order="F"), 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(ValueError):
        lsf.extendField(np.ones((6, 6, 6), order="C"), phi, 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(ValueError):
        lsf.extendField(q, phi, 5, 5, 5, 0.1, mask=np.ones((6, 5, 6), dtype=np.int32, order="F"))
    with pytest.raises(TypeError):
        lsf.extendField(q.astype(np.float32), phi, 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(TypeError):
        lsf.extendField(q, phi.astype(np.float32), 5, 5, 5, 0.1, band=2.0)
    with pytest.raises(TypeError):
        lsf.extendField(q, phi, 5, 5, 5, 0.1, mask=mask.astype(np.int64))
    with pytest.raises(TypeError):
        lsf.extendField(q, [1.0] * 216, 5, 5, 5, 0.1, band=2.0)
    assert np.all(q == 1.0) and np.all(phi == 1.0)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    q = np.full((6, 6, 6), 3.0, order="F")
    phi = np.ones((6, 6, 6), order="F")
    mask = np.ones((6, 6, 6), dtype=np.int32, order="F")
    for kw in (dict(band=2.0), dict(mask=mask)):
        with pytest.raises(lsf.LsfError) as e:
            lsf.extendField(q, phi, 5, 5, 5, 0.1, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(q == 3.0)
