"""lsf_extend_field_band without a GPU: the interface through every layer, the serial statement of the contract
(tests/extend_band_ref.py: its two forms against each other, the figures of the prototype the contract was written from, equality
with the converged full-grid statement tests/extend_ref.py on tubes that keep clear of the walls), argument validation before the
library, and no CPU fallback."""
import os
import re

import numpy as np
import pytest

import advect_ref as R
import extend_band_ref as X
import extend_ref as E
from advect_band_ref import list_of
from conftest import ROOT


# ---------------------------------------------------------------------------------- the interface
def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsf.h")).read(), flags=re.S)
    for name, nargs in (("lsf_extend_field_band", 14), ("lsf_extend_field_band_device", 15)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+LSF_EXTEND_BAND_INFO_LEN\s+4\b", hdr) and _lib.LSF_EXTEND_BAND_INFO_LEN == 4
    assert callable(lsf.extendFieldBand) and "extendFieldBand" in levelset.__all__ and "ExtendBandReport" in levelset.__all__
    assert lsf.ExtendBandReport._fields == ("passes", "converged", "trace", "cells", "frozen", "reached", "unreached")
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_fortran_shim_exports_extendfieldband():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\bextendFieldBand\b", public)
    assert "BIND(C,NAME='lsf_extend_field_band')" in src
    assert re.search(r"^SUBROUTINE extendFieldBand\(q,phi,mask,nx,ny,nz,dx,band\)", src, flags=re.M)
    assert "CALL lsf_fail('lsf_extend_field_band',rc)" in src
    assert re.search(r"^!\s+extendFieldBand\(q,phi,mask,nx,ny,nz,dx,band\)", src, flags=re.M)  # the header comment's list of procedures


# ---------------------------------------------------------------------------------- the statement
def _same(a, b):
    return np.array_equal(a.field, b.field, equal_nan=True) and tuple(a[1:]) == tuple(b[1:])


def _case_12_9_7():
    phi, dx = R.sphere_distance((12, 9, 7), (0.1, 0.05, 0.0), 0.3)
    mask = np.asfortranarray((np.abs(phi) < 2.6 * dx).astype(np.int32))
    q = X.prefill(phi.shape)
    frozen = X.frozen_of(phi, list_of(mask), dx, 1.2)
    assert frozen.any() and (list_of(mask) & ~frozen).any()
    q[frozen] = E.quantity(phi.shape, dx)[frozen]
    return q, phi, mask, dx, 1.2


@pytest.mark.parametrize("cap", [1, 64])
@pytest.mark.parametrize("case", ["small", "12x9x7"])
def test_the_two_forms_agree_bit_for_bit(case, cap):
    if case == "small":
        q, phi, mask, known, dx, band = X.inputs("small")
    else:
        q, phi, mask, dx, band = _case_12_9_7()
        known = np.asfortranarray(X.frozen_of(phi, list_of(mask), dx, band).astype(np.int32))
    keep = [a.copy() for a in (q, phi, mask, known)]
    a = X.extend_band_loops(q, phi, mask, dx, band=band, max_passes=cap)
    b = X.extend_band(q, phi, mask, dx, band=band, max_passes=cap)
    c = X.extend_band(q, phi, mask, dx, known=known, max_passes=cap)
    assert _same(a, b) and _same(a, c)
    assert a.passes == len(a.trace) <= cap and a.trace[0] > 0 and a.converged == (cap == 64)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(keep, (q, phi, mask, known)))  # the arguments are left alone


# the figures of the numpy prototype the contract was written from; a deviation is a deviation from the contract
TABLE = {
    "small": (246, 104, 4, [108, 96, 38, 0]),
    "general": (6170, 2202, 12, [1218, 2064, 2754, 2580, 2036, 1462, 948, 538, 222, 76, 14, 0]),
    "wide": (13144, 2202, 20, [1218, 2064, 2852]),
    "interior": (12167, 898, 30, [549, 964]),
}


@pytest.mark.parametrize("case", sorted(TABLE))
def test_figures_of_the_prototype(case):
    cells, frozen, passes, trace = TABLE[case]
    r = X.want(case, "band")
    print(case, r.cells, r.frozen, r.passes, r.trace)
    assert (r.cells, r.frozen, r.passes) == (cells, frozen, passes)
    assert r.trace[:len(trace)] == trace and r.trace[-1] == 0 and r.unreached == 0 and r.reached == cells - frozen
    if case == "wide":
        assert r.trace[-3:] == [88, 4, 0]
    if case == "interior":
        assert r.trace[-3:] == [8, 2, 0]
    assert _same(r, X.want(case, "known"))  # the same frozen set handed in as `known`: the band is ignored, and so are the 1s off the list


def test_known_on_one_side_only_leaves_136_cells_unreached():
    r = X.want("onesided", "known")
    q, phi, mask, known, dx, _ = X.inputs("onesided")
    lst = list_of(mask)
    print(r.cells, r.frozen, r.passes, r.unreached)
    assert (r.cells, r.frozen, r.passes, r.unreached) == (6170, 1274, 12, 136) and r.trace[-1] == 0
    nan = lst & np.isnan(r.field)
    assert nan.sum() == 136 and np.all(phi[nan] < 0) and r.reached == 6170 - 1274 - 136  # left NaN and counted, never guessed


SPHERES = {21: (4.1, 2819, 842, 10, [524, 934, 1318, 1332, 1053, 727, 406, 152, 19, 0]), 41: (6.1, 15263, 3307, 18, None),
           65: (8.1, 49882, 8452, 25, None)}


@pytest.mark.parametrize("N", sorted(SPHERES))
def test_tube_clear_of_the_walls_equals_the_converged_full_grid_statement(N):
    width, cells, frozen, passes, trace = SPHERES[N]
    q, phi, dx = E.sphere_case(N)
    mask = (np.abs(phi) < width * dx).astype(np.int32)
    lst = list_of(mask)
    assert lst.sum() == mask.sum()  # no 1 on a wall point ...
    grown = lst.copy()
    for a in range(3):
        grown |= np.roll(lst, 1, a) | np.roll(lst, -1, a)
    assert not grown[0].any() and not grown[-1].any() and not grown[:, 0].any() and not grown[:, -1].any() and not grown[:, :, 0].any() \
        and not grown[:, :, -1].any()  # ... and none next to one: the tube touches no wall point
    r = X.extend_band(q, phi, mask, dx, band=1.5)
    print(N, r.cells, r.frozen, r.passes, r.trace)
    assert (r.cells, r.frozen, r.passes, r.unreached) == (cells, frozen, passes, 0) and r.trace[-1] == 0
    if trace:
        assert r.trace == trace
    fz = X.frozen_of(phi, lst, dx, 1.5)
    full = E.extend(q, phi, dx, mask=fz.astype(np.int32))
    assert full[2][-1] == 0  # converged
    assert np.array_equal(r.field[lst], full[0][lst], equal_nan=True) and not np.isnan(r.field[lst]).any()
    assert np.array_equal(r.field[~lst], q[~lst])  # off the list: the caller's


@pytest.mark.parametrize("case", ["small", "general", "interior", "values", "onesided"])
def test_every_value_lies_between_the_frozen_values(case):
    form = "known" if case == "onesided" else "band"
    r = X.want(case, form)
    q, phi, mask, known, dx, band = X.inputs(case)
    lst = list_of(mask)
    fz = X.frozen_of(phi, lst, dx, band, known if form == "known" else None)
    got = r.field[lst & ~fz]
    got = got[~np.isnan(got)]
    assert got.size == r.reached and q[fz].min() <= got.min() and got.max() <= q[fz].max()  # convex combinations, rounded monotonically
    assert np.array_equal(r.field[fz], q[fz])


@pytest.mark.parametrize("cap", [1, 3, 11])
def test_max_passes_below_the_chain_length(cap):
    full = X.want("general", "band")
    r = X.want("general", "band", cap)
    assert full.passes == 12 and r.passes == cap and not r.converged and r.trace == full.trace[:cap]
    # (the 12th pass only confirms the fixed point: after 11 the field is there, and the call cannot know it)
    assert np.array_equal(r.field, full.field, equal_nan=True) == (cap == 11)
    q, phi, mask, known, dx, band = X.inputs("general")
    if cap == 1:
        assert _same(r, X.extend_band_loops(q, phi, mask, dx, band=band, max_passes=cap))  # the field after that many passes
    assert r.reached + r.unreached == r.cells - r.frozen and (r.unreached > 0 or cap == 11)


@pytest.mark.parametrize("which", [0, 1])
def test_off_list_q_is_untouched_bit_pattern_by_bit_pattern(which):
    q0, phi, mask, known, dx, band = X.inputs("general")
    lst = list_of(mask)
    q = np.where(X.frozen_of(phi, lst, dx, band), q0, X.prefill(q0.shape, which))
    r = X.extend_band(q, phi, mask, dx, band=band)
    assert np.array_equal(r.field[~lst].view(np.uint64), q[~lst].view(np.uint64))
    assert np.isnan(q[~lst]).any() and (q[~lst] == -7.0).any()
    assert np.array_equal(r.field[lst], X.want("general", "band").field[lst])  # ... and was not read: the list cells do not depend on it


def test_negative_zero_on_a_frozen_cell_stays():
    q0, phi, mask, known, dx, band = X.inputs("small")
    fz = X.frozen_of(phi, list_of(mask), dx, band)
    cell = tuple(np.argwhere(fz)[len(np.argwhere(fz)) // 2])
    q = q0.copy(order="F")
    q[cell] = -0.0
    r = X.extend_band(q, phi, mask, dx, band=band)
    assert r.field[cell] == 0.0 and np.signbit(r.field[cell])


def test_check_counts_what_the_library_refuses():
    q0, phi0, mask, known, dx, band = X.inputs("small")
    assert X.check(q0, phi0, mask, dx, band=band) == (246, 104, 0, 0)
    lst = list_of(mask)
    cell = tuple(np.argwhere(lst)[100])
    phi = phi0.copy(order="F")
    phi[cell] = np.inf
    six = sum(int(lst[tuple(np.add(cell, d))]) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
    assert X.check(q0, phi, mask, dx, known=known)[3] == 1 + six
    q = q0.copy(order="F")
    q[tuple(np.argwhere(X.frozen_of(phi0, lst, dx, band))[3])] = np.nan
    assert X.check(q, phi0, mask, dx, band=band)[2] == 1
    with pytest.raises(ValueError):
        X.extend_band(q0, phi0, np.zeros_like(mask), dx, band=band)
    with pytest.raises(ValueError):
        X.extend_band(q0, phi0, mask, dx, band=1e-9)


# ---------------------------------------------------------------------------------- the Python layer
def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    q = np.full((6, 6, 6), -7.0, order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    bad = [
        (ValueError, (q, phi, None, 0.1), dict(band=1.5)),
        (ValueError, (q, phi, m, 0.1), dict()),  # neither known nor band
        (ValueError, (q, phi, m, 0.1), dict(known=m, band=1.5)),
        (ValueError, (q, phi, m, 0.0), dict(band=1.5)),
        (ValueError, (q, phi, m, float("nan")), dict(band=1.5)),
        (ValueError, (q, phi, m, 0.1), dict(band=0.0)),
        (ValueError, (q, phi, m, 0.1), dict(band=float("inf"))),
        (ValueError, (q, phi, m, 0.1), dict(band=1.5, max_passes=0)),
        (ValueError, (q, phi, m, 0.1), dict(band=1.5, trace_cap=-1)),
        (ValueError, (q, q, m, 0.1), dict(band=1.5)),
        (ValueError, (q, np.ones((6, 6, 5), order="F"), m, 0.1), dict(band=1.5)),
        (ValueError, (q, np.ones((6, 6, 6), order="C"), m, 0.1), dict(band=1.5)),
        (ValueError, (q, phi, np.ones((6, 5, 6), np.int32, order="F"), 0.1), dict(band=1.5)),
        (ValueError, (q, phi, m, 0.1), dict(known=np.ones((5, 6, 6), np.int32, order="F"))),
        (ValueError, (q.ravel(order="F"), phi, m, 0.1), dict(band=1.5)),  # the grid size comes from q's shape
        (TypeError, (q.astype(np.float32), phi, m, 0.1), dict(band=1.5)),
        (TypeError, (q, phi.astype(np.float32), m, 0.1), dict(band=1.5)),
        (TypeError, (q, phi, m.astype(np.int64), 0.1), dict(band=1.5)),
        (TypeError, (q, phi, m, 0.1), dict(known=m.astype(bool))),
        (TypeError, ([[1.0]], phi, m, 0.1), dict(band=1.5)),
    ]
    for exc, args, kw in bad:
        with pytest.raises(exc):
            lsf.extendFieldBand(*args, **kw)
    assert np.all(phi == 1.0) and np.all(q == -7.0) and np.all(m == 1)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    m = np.ones((6, 6, 6), np.int32, order="F")
    q = np.full((6, 6, 6), -7.0, order="F")
    for kw in (dict(band=1.5), dict(known=m.copy(order="F"))):
        with pytest.raises(lsf.LsfError) as e:
            lsf.extendFieldBand(q, phi, m, 0.1, **kw)
        assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(q == -7.0) and np.all(phi == 1.0) and np.all(m == 1)
