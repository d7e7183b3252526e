"""lsf_redistance_band without a GPU: the interface (second header, second ctypes table, package, Fortran shim), the wrapper's refusals
before the library loads, LSF_ERR_NO_DEVICE, the argument checks of levelsetfortran_amd/csrc/lsf_host_args_redistance.hpp held against
tests/golden/redistance_args_messages.txt, and the properties of the statement tests/redistance_ref.py that the GPU tests compare the
library with (tests/test_gpu_redistance_band.py).

The accuracy figures of DESIGN.md section 4.27 are printed by test_accuracy_table (pytest -s); no test ranks the call against the
sweeps."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import distance_fill_ref as DF
import redistance_cases as C
import redistance_ref as R
import sample_ref as S
from advect_band_ref import list_of
from conftest import GOLDEN as GOLDEN_DIR, ROOT

HEADER = os.path.join(ROOT, "include", "lsf_redistance.h")
ARGS_HEADER = os.path.join(ROOT, "levelsetfortran_amd", "csrc", "lsf_host_args_redistance.hpp")
GOLDEN = os.path.join(GOLDEN_DIR, "redistance_args_messages.txt")
NAMES = ["lsf_redistance_band", "lsf_redistance_band_device"]


# ---------------------------------------------------------------------------------- the interface
def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lsf_[a-z0-9_]+)\s*\(", txt)))


def test_the_interface_lives_in_the_second_header_and_the_second_table():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    assert _declared(HEADER) == NAMES
    assert '#include "lsf.h"' in open(HEADER).read() and "LSF_REDISTANCE_INFO_LEN 9" in open(HEADER).read()
    assert sorted(_lib.SIGNATURES_REDISTANCE) == NAMES and _lib.LSF_REDISTANCE_INFO_LEN == 9
    host, dev = (_lib.SIGNATURES_REDISTANCE[n] for n in NAMES)
    assert dev[0] is host[0] and dev[1] == host[1] + [_lib.c_void_p] and len(host[1]) == 15
    # include/lsf.h and the first table do not name it: tests/test_abi.py and tests/test_python_seam_cpu.py pin both
    assert not any("redistance" in n for n in _declared(os.path.join(ROOT, "include", "lsf.h")))
    assert "redistance" not in open(os.path.join(ROOT, "include", "lsf.h")).read()
    assert not any("redistance" in n for n in _lib.SIGNATURES) and not any("redistance" in n for n in _lib.DEVICE_TWINS)
    lib = _lib.load()
    for n in NAMES:
        fn = getattr(lib, n)
        assert fn.argtypes == _lib.SIGNATURES_REDISTANCE[n][1]
    assert lib.lsf_version() == 106
    for name in ("redistanceBand", "RedistanceReport"):
        assert name in levelset.__all__ and getattr(lsf, name) is getattr(levelset, name)
    assert lsf.RedistanceReport._fields == ("passes", "converged", "trace", "change", "cells", "frozen", "filled", "unreached", "offband", "outside",
                                           "flat", "not_converged", "far")
    shim = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    assert "PUBLIC :: redistanceBand" in shim and "SUBROUTINE redistanceBand(phi,mask,nx,ny,nz,dx,near)" in shim
    assert "BIND(C,NAME='lsf_redistance_band')" in shim and "redist_iters,redist_tol,redist_passes" in shim


# ---------------------------------------------------------------------------------- the wrapper's refusals
N = (5, 4, 3)
SHAPE = (6, 5, 4)


def _valid():
    x, y, z = np.meshgrid(*[np.arange(s) * 0.25 for s in SHAPE], indexing="ij")
    return dict(phi=np.asfortranarray(x + 0.5 * y - 0.25 * z - 0.7), mask=np.ones(SHAPE, np.int32, order="F"), nx=5, ny=4, nz=3, dx=0.25)


# (what is wrong, the replaced arguments, the exception, its message)
DEFECTS = [
    ("dx 0", dict(dx=0.0), ValueError, "dx must be finite and > 0"),
    ("dx nan", dict(dx=float("nan")), ValueError, "dx must be finite and > 0"),
    ("near 0", dict(near=0.0), ValueError, "near must be finite and > 0"),
    ("near inf", dict(near=float("inf")), ValueError, "near must be finite and > 0"),
    ("iters 0", dict(iters=0), ValueError, "iters must be >= 1"),
    ("tol negative", dict(tol=-1e-9), ValueError, "tol must be finite and >= 0"),
    ("tol nan", dict(tol=float("nan")), ValueError, "tol must be finite and >= 0"),
    ("max_passes 0", dict(max_passes=0), ValueError, "max_passes must be >= 1"),
    ("phi float32", dict(phi=np.zeros(SHAPE, np.float32, order="F")), TypeError, "phi must be a numpy array of float64"),
    ("phi a list", dict(phi=[0.0] * 120), TypeError, "phi must be a numpy array of float64"),
    ("phi C-ordered", dict(phi=np.zeros(SHAPE)), ValueError, "phi must be Fortran-ordered with shape (nx+1, ny+1, nz+1) = (6, 5, 4)"),
    ("phi of another shape", dict(phi=np.zeros((6, 5, 5), order="F")), ValueError, "phi must be Fortran-ordered with shape (nx+1, ny+1, nz+1) = (6, 5, 4)"),
    ("phi read-only", "readonly", ValueError, "phi must be writeable (it is INTENT(INOUT) in the reference)"),
    ("mask float64", dict(mask=np.ones(SHAPE, order="F")), TypeError, "mask must be a numpy array of int32"),
    ("mask of another shape", dict(mask=np.ones((6, 5, 3), np.int32, order="F")), ValueError,
     "mask must be Fortran-ordered with shape (nx+1, ny+1, nz+1) = (6, 5, 4)"),
    ("mask missing", dict(mask=None), TypeError, "mask must be a numpy array of int32"),
]


@pytest.mark.parametrize("what,patch,exc,msg", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_a_single_defect_is_refused_before_the_library_loads(monkeypatch, what, patch, exc, msg):
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    kw = _valid()
    if patch == "readonly":
        kw["phi"].setflags(write=False)
    else:
        kw.update(patch)
    before = kw["phi"].copy() if isinstance(kw["phi"], np.ndarray) else None
    with pytest.raises(exc) as e:
        lsf.redistanceBand(**kw)
    assert str(e.value) == msg
    if before is not None:
        assert np.array_equal(kw["phi"], before)


def test_no_device_is_an_error_and_phi_is_untouched():
    """fails without the feature: there is no redistanceBand"""
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    if lib.lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    kw = _valid()
    before = kw["phi"].copy()
    with pytest.raises(lsf.LsfError) as e:
        lsf.redistanceBand(**kw)
    assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.array_equal(kw["phi"].view(np.uint64), before.view(np.uint64))
    for name in NAMES:  # ... and through the C ABI, the device form too: no output is written
        done, change, info = _lib.c_int(-7), _lib.c_double(-7.0), np.full(9, -7, np.int64)
        args = [kw["phi"].ctypes.data, kw["mask"].ctypes.data, 5, 4, 3, 0.25, 2.5, 8, 1e-9, 64, done, None, 0, change, info.ctypes.data]
        assert getattr(lib, name)(*args, *([None] if name.endswith("_device") else [])) == _lib.LSF_ERR_NO_DEVICE
        assert done.value == -7 and change.value == -7.0 and (info == -7).all()
    assert np.array_equal(kw["phi"].view(np.uint64), before.view(np.uint64))


# ---------------------------------------------------------------------------------- the argument checks
@pytest.fixture(scope="module")
def lines():
    src = os.path.join(ROOT, "tests", "host_args", "redistance_args_main.cpp")
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    assert cxx, "no host C++ compiler (c++, or ROCm's clang++)"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "redistance_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wno-unused-function", "-o", exe, src], check=True)
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_every_case_gives_the_recorded_code_and_message(lines):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for n, (g, w) in enumerate(zip(lines, want), 1):
        assert g == w, f"line {n}"
    assert len(lines) == len(want) >= 35
    for line in lines:
        name, rc, msg = (p.strip() for p in line.split("|"))
        valid = name.startswith("valid")
        assert int(rc) == (0 if valid else 2), name
        assert (msg == "") == valid, name
        # (the dimensions are refused in the shared words of lsf_reinit_band's check, which carry no call name)
        assert valid or msg.startswith("lsf_redistance_band: ") or msg in ("nx, ny, nz must be >= 2", "field too large",
                                                                            "a k-plane of the field exceeds 2 GB"), name


def test_the_table_reaches_every_refusal_of_the_header(lines):
    """every piece of message text in the header -- a string literal of a line with fail( or grid_ok(, or of the line that continues
    one -- is part of some refused case's message; so are the shared refusals of the dimensions and the overlap"""
    with open(ARGS_HEADER) as f:
        text = f.read()
    assert "#include" not in text  # it depends on include/lsf.h, <cmath>, <cstdint>, <string>, fail() and lsf_host_args.hpp alone
    code = [ln for ln in text.splitlines() if "fail(" in ln or "grid_ok(" in ln or ln.lstrip().startswith('"')]
    pieces = [s for ln in code for s in re.findall(r'"([^"]+)"', ln)]
    assert len(pieces) >= 10
    messages = [ln.split(" | ", 2)[2] for ln in lines if " | 2 | " in ln]
    unreached = [s for s in pieces if not any(s in m for m in messages)]
    assert not unreached, unreached
    for needle in ("phi overlaps mask", "nx, ny, nz must be >= 2", "field too large", "a k-plane of the field exceeds 2 GB", "more than 2^31 - 1 points"):
        assert any(needle in m for m in messages), needle


# ---------------------------------------------------------------------------------- the statement
GRIDS = (25, 41)
# the table of the issue prints its three columns to these steps; a figure is compared with a row of the table at that precision
PRINTED = (0.5e-4, 0.5e-4, 0.5e-2)
# the largest value error of the cubic within 1.5 dx of a sphere of 6 cells radius (its 25^3 grid), in dx.  The
# spheres here have 6.4 and 10.7 cells radius -- flatter in cells, so the figure bounds both
CUBIC_VALUE_ERROR = 2.68e-3


def test_the_visit_is_distance_fill_s():
    rng = np.random.default_rng(7)
    v = rng.uniform(0.0, 1.0, (400, 3))
    v[rng.random((400, 3)) < 0.2] = np.inf
    v[:, 0] = np.minimum(v[:, 0], 5.0)  # one finite operand each
    for dx in (0.1, 0.37):
        got = R.visit(v[:, 0], v[:, 1], v[:, 2], np.float64(dx))
        with np.errstate(invalid="ignore"):
            want = np.array([DF._solve_scalar(*row, np.float64(dx)) for row in v])
        assert np.array_equal(got, want)


def test_accuracy_table():
    """the table of DESIGN.md section 4.27 (pytest -s prints it), and what must hold of it: no unreached cell and no NOT_CONVERGED or
    FLAT foot on the four inputs, and the error over |d| < 1.5 dx at 41^3 below half that at 25^3 on both fields"""
    print("\npoints  g       passes  |d| < 1.5 dx  frozen    whole list   info")
    near = {}
    for kind in ("mild", "strong"):
        for n in GRIDS:
            r, e = R.sphere_want(n, kind), R.errors(n, kind)
            print(f"{n}^3    {kind:7s} {r.passes:3d}     {e[0]:.5f}       {e[1]:.5f}   {e[2]:.4f}       {r.info}")
            near[kind, n] = e[0]
            assert r.trace[-1] == 0 and r.passes < R.SETTINGS["max_passes"]
            assert r.info[3] == 0 and r.info[6] == 0 and r.info[7] == 0, r.info
            assert r.info[1] + sum(r.info[4:]) == r.info[0] == sum(r.info[1:4])
        ratio = near[kind, 25] / near[kind, 41]
        print(f"        {kind:7s} ratio of the first column, 25^3 over 41^3: {ratio:.2f} (second order would give {(40 / 24) ** 2:.2f})")
        assert near[kind, 41] < 0.5 * near[kind, 25]


@pytest.mark.parametrize("n", GRIDS)
def test_an_exact_distance_stays_within_the_mild_row(n):
    """the three errors on the exact distance against the mild row of the same grid, at the precision the table prints"""
    exact, mild = R.errors(n, "exact"), R.errors(n, "mild")
    print(n, exact, mild)
    for e, m, step in zip(exact, mild, PRINTED):
        assert e <= m + step


@pytest.mark.parametrize("n", GRIDS)
@pytest.mark.parametrize("kind", ["exact", "mild", "strong"])
def test_signs_and_the_rest_of_the_field(n, kind):
    phi, mask, dx, _ = R.sphere_case(n, kind)
    r = R.sphere_want(n, kind)
    lst = list_of(mask)
    assert np.array_equal(r.field[lst] < 0, phi[lst] < 0)
    assert np.array_equal(r.field[~lst].view(np.uint64), phi[~lst].view(np.uint64))
    assert r.change == np.abs(r.field - phi).max()


@pytest.mark.parametrize("n", GRIDS)
def test_frozen_magnitudes_are_not_below_the_distance(n):
    """dist is the distance to a point of the interpolant's level set, which lies within the cubic's value error of the sphere"""
    phi, mask, dx, d = R.sphere_case(n, "exact")
    r = R.sphere_want(n, "exact")
    slack = (np.abs(r.field[r.frozen]) - np.abs(d[r.frozen])) / dx
    print(n, slack.min(), slack.max())
    assert slack.min() >= -CUBIC_VALUE_ERROR


@pytest.mark.parametrize("n", GRIDS)
def test_the_converged_fill_is_distance_fill_s_on_the_same_frozen_set(n):
    """On a list that holds every point the full-grid call would draw on -- here: the band |d| < 8.1 dx of a sphere, where a cell draws
    on neighbours nearer to the surface only, which are list cells and never wall points (at 25^3 the band reaches the walls) -- the
    converged magnitudes at list cells equal the converged lsf_distance_fill with the frozen cells as its mask."""
    phi, mask, dx, _ = R.sphere_case(n, "exact")
    r = R.sphere_want(n, "exact")
    lst = list_of(mask)
    full, rounds, trace, nfrozen = DF.fill(r.field, dx, mask=r.frozen.astype(np.int32), max_rounds=64)
    assert trace[-1] == 0 and nfrozen == r.info[1]
    assert np.array_equal(np.abs(full[lst]), np.abs(r.field[lst]))


def test_the_pass_cap_is_a_state_not_an_error():
    phi, mask, dx, _ = R.sphere_case(25, "mild")
    whole = R.sphere_want(25, "mild")
    for cap in (1, 3):
        r = R.redistance_band(phi, mask, dx, **dict(R.SETTINGS, max_passes=cap))
        assert r.passes == cap and r.trace == whole.trace[:cap] and r.info[3] > 0
        assert r.info[:2] == whole.info[:2] and r.info[2] + r.info[3] == whole.info[2]


def test_the_statement_refuses_what_the_library_refuses():
    phi, mask, dx, kw = C.inputs("baseline")
    bad = phi.copy()
    bad[tuple(np.argwhere(list_of(mask))[5])] = np.nan
    with pytest.raises(R.Invalid, match="1 list cell"):
        R.redistance_band(bad, mask, dx, **kw)
    with pytest.raises(R.Invalid, match="empty"):
        R.redistance_band(phi, np.zeros_like(mask), dx, **kw)
    with pytest.raises(R.Invalid, match="no frozen cell"):
        R.redistance_band(phi, mask, dx, **dict(kw, near=1e-9))
    off = np.where(list_of(mask), phi, np.nan)  # phi off the list is never read
    assert np.array_equal(R.redistance_band(off, mask, dx, **kw).field[list_of(mask)], C.want("baseline").field[list_of(mask)])


def test_every_gpu_case_reaches_the_path_it_is_named_after():
    info = {c: C.want(c).info for c in C.CASES}
    for c in C.CASES:
        phi, mask, dx, kw = C.inputs(c)
        r = C.want(c)
        assert r.info[1] + sum(r.info[4:]) == r.info[0] == sum(r.info[1:4]) and r.info[1] > 0, c
        lst = list_of(mask)
        assert np.array_equal(r.field[lst] < 0, phi[lst] < 0), c
    assert info["baseline"][0] > 4 * 256 and info["baseline"][0] % 256 != 0  # several chunks with a ragged last one
    assert C.inputs("asymmetric")[0].shape == (70, 21, 45)
    assert info["cut"][3] > 0 and info["cut"][4] > 0  # a piece without a frozen cell, kept bit for bit; feet off the band
    phi, mask, dx, kw = C.inputs("cut")
    r = C.want("cut")
    assert np.array_equal(r.field[18:22, 2:6, 13:17].view(np.uint64), phi[18:22, 2:6, 13:17].view(np.uint64))
    # list cells in the layers next to two walls, crossed by the surface.  Their cubic stencil holds wall points, and so do the eight
    # corners the joint rule falls back to beside a wall: the band rule refuses both, the cells are OFFBAND and are filled from
    # further inside with their wall neighbours counting as +inf
    phi, mask, dx, kw = C.inputs("walls")
    r = C.want("walls")
    lst = list_of(mask)
    at = np.argwhere(lst)
    for layer in ((at[:, 0] == 1), (at[:, 2] == phi.shape[2] - 2)):
        assert layer.sum() > 20 and (r.status[layer] == S.OFFBAND).all()
    for near_wall in ((at[:, 0] <= 2), (at[:, 2] >= phi.shape[2] - 3)):  # the surface within two cells of the wall: both signs there
        assert len({bool(v) for v in phi[tuple(at[near_wall].T)] < 0}) == 2
    assert (mask[0] == 1).any() and (mask[:, :, -1] == 1).any() and not r.frozen[1].any() and r.info[3] == 0
    phi, mask, dx, kw = C.inputs("zeros")
    zero = (phi == 0) & list_of(mask)
    r = C.want("zeros")
    assert zero.sum() == 12 and np.signbit(phi[zero]).sum() == 6
    kept = zero & r.frozen  # dist == 0.0: the value on entry, the sign bit of -0.0 included
    assert kept.sum() == 10 and np.array_equal(r.field[kept].view(np.uint64), phi[kept].view(np.uint64))
    filled = zero & ~r.frozen  # two of them sit two cells from the upper z wall: OFFBAND, filled, and +u for -0.0 too ((-0.0 < 0) is false)
    assert filled.sum() == 2 and (r.field[filled] > 0).all() and np.signbit(phi[filled]).any()
    assert C.want("cap1").passes == 1 and C.want("cap3").passes == 3 and info["cap3"][3] > 0
    assert C.want("cap3").trace == C.want("baseline").trace[:3]
    assert C.want("baseline").passes == 12 > 9  # the caps at the edge of a batch of 8 cut a run that would go on
    for cap in (8, 9):
        assert C.want(f"cap{cap}").passes == cap and C.want(f"cap{cap}").trace == C.want("baseline").trace[:cap]
        assert not np.array_equal(C.want(f"cap{cap}").field, C.want("baseline").field)  # (every cell is reached by then: values still fall)
    assert info["one_iteration"][7] > 0 and info["flat"][6] > 0
    assert set(np.unique(C.inputs("values")[1])) == {-1, 0, 1, 7} and info["values"] == info["baseline"]
    assert np.array_equal(C.want("values").field, C.want("baseline").field)
