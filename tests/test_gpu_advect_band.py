"""lsf_advect_field_band on the GPU against tests/advect_band_ref.py, the serial statement of the contract in include/lsf.h.  With the
STRICT arithmetic the field, the change trace, the CFL number, info and margin are compared with `==`; FAST within the project's
1e-12 RMS of STRICT over the list cells (the bound of tests/test_gpu_advect_field.py: same operator, same arithmetic).

Grids and masks, the smallest on which each piece can go wrong (a chunk is 256 list entries, MB_CH in csrc/lsf_minmax_band.hpp):
  small     (10,10,10), |phi| < 2.1 dx: 246 cells -- one ragged chunk -- among them the grid's one WENO cell (4,4,4)
  firstord  (9,12,10): no WENO cell
  general   (40,33,27), |phi| < 4.1 dx: about 6 000 cells, 25 chunks, the last ragged; x not a multiple of anything
  interior  (25,25,25), every interior point: the edge cells are the wall-adjacent ones
  onecell   a list of one cell (the WENO cell of (10,10,10))
  values    (12,11,10): a mask carrying 0, 7, -1 and 1s on wall points
  big       (73,73,73), every interior point, steps = 0: 357 911 cells, more than one entry per thread of the scan and the closing pass"""
import ctypes
import functools
import math

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R

pytestmark = pytest.mark.gpu

FAST_RMS_TOL = 1.0e-12  # tests/test_gpu_advect_field.py
CHUNK = 256  # MB_CH
CASES = ["small", "firstord", "general", "interior", "onecell", "values"]
TERMS = ["velocity", "speed", "both"]
SCHEMES = [("rk3", 3), ("euler", 3)]  # Euler with an odd count: the result is scattered out of the second buffer
SEAMS = ["host", "device"]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _geometry(case):
    """(phi0, mask, npts, dx) of a case; shared and read-only"""
    if case in ("small", "onecell"):
        npts = (10, 10, 10)
        phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
        if case == "small":
            mask = (np.abs(phi0) < 2.1 * dx).astype(np.int32)
        else:
            mask = np.zeros(npts, np.int32)
            mask[4, 4, 4] = 1
    elif case == "firstord":
        npts = (9, 12, 10)
        phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
        mask = (np.abs(phi0) < 2.1 * dx).astype(np.int32)
    elif case == "general":
        npts = (40, 33, 27)
        phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
        mask = (np.abs(phi0) < 4.1 * dx).astype(np.int32)
    elif case == "interior":
        npts = (25, 25, 25)
        phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
        mask = np.ones(npts, np.int32)
    else:
        npts = (12, 11, 10)
        phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
        band = np.abs(phi0) < 1.3 * dx
        mask = np.where(band, 1, 0).astype(np.int32)
        mask[~band & (phi0 > 3.5 * dx)] = 7  # not 1: not in the list
        mask[~band & (phi0 < 0)] = -1
        for a in range(3):  # 1s on all six walls: ignored
            sl = [slice(None)] * 3
            for side in (0, -1):
                sl[a] = side
                mask[tuple(sl)] = 1
        inner = mask[1:-1, 1:-1, 1:-1]
        assert (inner == 0).any() and (inner == 7).any() and (inner == -1).any()
    mask = np.asfortranarray(mask)
    phi0.setflags(write=False), mask.setflags(write=False)
    return phi0, mask, npts, dx


def test_the_cases_are_what_the_docstring_says():
    phi0, mask, npts, dx = _geometry("small")
    lst = B.list_of(mask)
    assert lst.sum() == 246 < CHUNK and lst[4, 4, 4]  # the one cell with 4 <= i, j, k <= n - 5 = 4
    assert B.list_of(_geometry("onecell")[1]).sum() == 1
    n = int(B.list_of(_geometry("general")[1]).sum())
    assert (n + CHUNK - 1) // CHUNK == 25 and n % CHUNK != 0, n
    assert _geometry("firstord")[2][0] - 1 - 5 < 4  # nx = 8: no i with 4 <= i <= nx - 5
    lst = B.list_of(_geometry("interior")[1])
    assert lst.sum() == 23 ** 3 and B.edge_of(lst).sum() == 23 ** 3 - 21 ** 3
    phi0, mask, npts, dx = _geometry("values")
    assert B.list_of(mask).sum() == np.count_nonzero(np.abs(phi0[1:-1, 1:-1, 1:-1]) < 1.3 * dx) < mask[mask == 1].size


@functools.lru_cache(maxsize=None)
def _inputs(case, terms):
    """(phi0, mask, vel or None, F or None, (nx, ny, nz), dx, dt): dt puts the CFL number over the whole grid at 0.5"""
    phi0, mask, npts, dx = _geometry(case)
    u, v, w, f, _ = R.wavy_inputs(npts)
    vel = (u, v, w) if terms in ("velocity", "both") else None
    F = f if terms in ("speed", "both") else None
    dt = 0.5 * dx / R.max_speed(vel, F)
    for a in (u, v, w, f):
        a.setflags(write=False)
    return phi0, mask, vel, F, tuple(n - 1 for n in npts), dx, dt


@functools.lru_cache(maxsize=None)
def _want(case, terms, scheme, steps):
    phi0, mask, vel, F, _, dx, dt = _inputs(case, terms)
    r = B.advect_band(phi0, mask, vel, F, dx, dt, steps, scheme)
    assert r.steps == steps and 0 < r.cfl <= 0.5 and not r.nan
    r.field.setflags(write=False)
    return r


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, steps, **kw):
    """advectFieldBand on fresh copies through one seam; returns (field, report); asserts that mask and inputs are unchanged"""
    nx, ny, nz = n
    ins = ([] if vel is None else list(vel)) + ([] if F is None else [F])
    if seam == "host":
        got, m = phi0.copy(order="F"), mask.copy(order="F")
        args = [a.copy(order="F") for a in ins]
    else:
        got, m = _dev(phi0), _dev(mask)
        args = [_dev(a) for a in ins]
    velocity = tuple(args[:3]) if vel is not None else None
    speed = args[-1] if F is not None else None
    try:
        rep = lsf.advectFieldBand(got, m, nx, ny, nz, dx, dt, steps, velocity=velocity, speed=speed, **kw)
    finally:
        for a, b in zip(args + [m], ins + [mask]):
            assert _same(a if seam == "host" else _host(a, b.shape), b)  # read, never written
    return (got if seam == "host" else _host(got, phi0.shape)), rep


def _assert_report(rep, want):
    assert rep.steps == want.steps and rep.cfl == want.cfl and rep.change == want.change
    assert (rep.cells, rep.edge_cells, rep.edge_flips) == (want.cells, want.edge_cells, want.edge_flips)
    assert rep.margin == want.margin


# ---------------------------------------------------------------------------------- 1: STRICT == the statement
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("scheme,steps", SCHEMES)
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("case", CASES)
def test_strict_is_bit_identical_to_the_statement(lsf, case, terms, scheme, steps, seam):
    phi0, mask, vel, F, n, dx, dt = _inputs(case, terms)
    want = _want(case, terms, scheme, steps)
    got, rep = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, steps, scheme=scheme, arith="strict")
    diff = np.abs(got - want.field)
    print(f"{case} {terms} {scheme} {seam}: max |got - want| = {diff.max():.3e} at {np.unravel_index(diff.argmax(), diff.shape)}, cfl {rep.cfl!r}, "
          f"change {rep.change}, cells {rep.cells}, edge {rep.edge_cells}, flips {rep.edge_flips}, margin {rep.margin!r} (want {want.margin!r})")
    assert np.array_equal(got, want.field)  # the whole field: nothing outside the list is written
    _assert_report(rep, want)
    lst = B.list_of(mask)
    assert np.array_equal(got[~lst], phi0[~lst]) and not np.array_equal(got[lst], phi0[lst])


# ---------------------------------------------------------------------------------- 2: the inputs are read at list cells only
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("scheme,steps", SCHEMES)
def test_nan_in_the_inputs_outside_the_list_changes_nothing(lsf, scheme, steps, seam):
    phi0, mask, vel, F, n, dx, dt = _inputs("general", "both")
    want = _want("general", "both", scheme, steps)
    vel_nan, F_nan = B.masked_inputs(B.list_of(mask), vel, F)
    assert np.isnan(F_nan).sum() > F_nan.size // 2
    got, rep = _run(lsf, seam, phi0, mask, vel_nan, F_nan, n, dx, dt, steps, scheme=scheme)
    assert np.array_equal(got, want.field)
    _assert_report(rep, want)


# ---------------------------------------------------------------------------------- 3: streams, no state between calls, run to run
@pytest.mark.parametrize("scheme", ["rk3", "euler"])
def test_side_stream_split_calls_and_run_to_run(lsf, scheme):
    import torch

    phi0, mask, vel, F, n, dx, dt = _inputs("general", "both")
    want = _want("general", "both", scheme, 4)
    nx, ny, nz = n
    for _ in range(2):  # the second run of a call equals the first
        t, m, ins = _dev(phi0), _dev(mask), [_dev(a) for a in (*vel, F)]
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            rep = lsf.advectFieldBand(t, m, nx, ny, nz, dx, dt, 4, velocity=tuple(ins[:3]), speed=ins[3], scheme=scheme)
        torch.cuda.synchronize()
        _assert_report(rep, want)
        assert np.array_equal(_host(t, phi0.shape), want.field)
    # one call of 4 steps equals two calls of 2 (each seam): field, trace and cfl; the flips are relative to each call's own entry
    half_want = _want("general", "both", scheme, 2)
    for seam in SEAMS:
        half, rep1 = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, 2, scheme=scheme)
        full, rep2 = _run(lsf, seam, half, mask, vel, F, n, dx, dt, 2, scheme=scheme)
        _assert_report(rep1, half_want)
        assert np.array_equal(full, want.field) and rep1.change + rep2.change == want.change and rep1.cfl == rep2.cfl == want.cfl
        assert rep2.margin == want.margin and (rep2.cells, rep2.edge_cells) == (want.cells, want.edge_cells)


# ---------------------------------------------------------------------------------- 4: deep cells are lsf_advect_field's
def test_deep_cells_equal_the_full_grid_call_on_the_device(lsf):
    """(33,31,29), RK3, one step: the list cells farther than 9 (city-block) from every non-list point hold what lsf_advect_field
    itself computes, for the all-interior mask (1287 cells) and for a tube."""
    npts = (33, 31, 29)
    n = tuple(v - 1 for v in npts)
    phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
    u, v, w, f, smax = R.wavy_inputs(npts)
    dt = 0.5 * dx / smax
    full = _dev(phi0)
    lsf.advectField(full, *n, dx, dt, 1, velocity=tuple(_dev(a) for a in (u, v, w)), speed=_dev(f))
    full = _host(full, npts)
    for mask, count in ((np.ones(npts, np.int32, order="F"), 1287), (np.asfortranarray((np.abs(phi0) < 11.5 * dx).astype(np.int32)), None)):
        deep = B.depth_of(B.list_of(mask), 9) > 9
        assert deep.sum() > 0 and (count is None or deep.sum() == count)
        got, rep = _run(lsf, "device", phi0, mask, (u, v, w), f, n, dx, dt, 1)
        assert rep.steps == 1 and np.array_equal(got[deep], full[deep]) and not np.array_equal(got[deep], phi0[deep])


# ---------------------------------------------------------------------------------- 5: FAST within 1e-12 RMS of STRICT
@pytest.mark.parametrize("scheme,steps", SCHEMES)
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("case", ["small", "firstord", "general", "interior"])
def test_fast_arithmetic_within_tolerance_of_strict(lsf, case, terms, scheme, steps):
    phi0, mask, vel, F, n, dx, dt = _inputs(case, terms)
    want = _want(case, terms, scheme, steps)
    got, rep = _run(lsf, "device", phi0, mask, vel, F, n, dx, dt, steps, scheme=scheme, arith="fast")
    lst = B.list_of(mask)
    rms = float(np.sqrt(np.mean((got[lst] - want.field[lst]) ** 2)))
    print(f"{case} {terms} {scheme}: FAST against STRICT over the list cells: rms {rms:.3e}, max {np.abs(got - want.field).max():.3e}")
    assert rep.steps == steps and rep.cfl == want.cfl  # the CFL number has one arithmetic
    assert (rep.cells, rep.edge_cells) == (want.cells, want.edge_cells)
    assert np.array_equal(got[~lst], phi0[~lst])
    assert rms <= FAST_RMS_TOL


# ---------------------------------------------------------------------------------- 6: errors and edges
def _raw(lib, seam, phi, mask, u, v, w, f, n, dx, dt, steps, scheme, mode):
    done, cfl, margin = ctypes.c_int(-7), ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    trace = np.full(8, -7.0)
    info = np.full(3, -7, np.int64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), ptr(u), ptr(v), ptr(w), ptr(f), n[0], n[1], n[2], dx, dt, steps, scheme, mode, ctypes.byref(done), ctypes.byref(cfl),
            trace.ctypes.data, 8, info.ctypes.data, ctypes.byref(margin))
    rc = lib.lsf_advect_field_band_device(*args, None) if seam == "device" else lib.lsf_advect_field_band(*args)
    return rc, done.value, cfl.value, trace, list(info), margin.value, (lib.lsf_last_error() or b"").decode()


@pytest.mark.parametrize("seam", SEAMS)
def test_invalid_arguments_leave_phi_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask0, (u0, v0, w0), f0, n, dx, dt = _inputs("values", "both")
    lst = B.list_of(mask0)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    phi, mask, u, v, w, f = (mk(a) for a in (phi0, mask0, u0, v0, w0, f0))
    cells = np.argwhere(lst)
    bad = f0.copy(order="F")
    bad[~lst] = np.nan  # legal
    bad[tuple(cells[0])], bad[tuple(cells[7])], bad[tuple(cells[-1])] = np.nan, np.inf, -np.inf
    badf = mk(bad)
    ok = dict(phi=phi, mask=mask, u=u, v=v, w=w, f=f, n=n, dx=dx, dt=dt, steps=2, scheme=_lib.LSF_ADVECT_RK3,
              mode=_lib.LSF_ORDER_JACOBI | _lib.LSF_ARITH_STRICT)
    cases = {
        "NULL phi": dict(phi=None),
        "NULL mask": dict(mask=None),
        "partial velocity": dict(w=None),
        "one component": dict(u=None, v=None),
        "neither": dict(u=None, v=None, w=None, f=None),
        "nx < 2": dict(n=(1, n[1], n[2])),
        "nz < 2": dict(n=(n[0], n[1], 0)),
        "dx = 0": dict(dx=0.0),
        "dx NaN": dict(dx=float("nan")),
        "dt < 0": dict(dt=-dt),
        "dt inf": dict(dt=float("inf")),
        "steps < 0": dict(steps=-1),
        "scheme": dict(scheme=2),
        "GS order": dict(mode=_lib.LSF_ORDER_GS | _lib.LSF_ARITH_STRICT),
        "unknown order": dict(mode=7),
        "non-finite speed": dict(f=badf),
        "non-finite velocity": dict(v=badf, f=None),
    }
    for name, change in cases.items():
        rc, done, cfl, trace, info, margin, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and done == -7 and cfl == -7.0 and np.all(trace == -7.0) and info == [-7, -7, -7] and margin == -7.0, name  # nothing reported
        if name.startswith("non-finite"):
            assert "3 non-finite" in msg, msg
        back = _host(phi, phi0.shape) if seam == "device" else phi
        assert np.array_equal(back, phi0), name
    # a valid call follows: the library is in working order, and the Python layer raises the same error
    rc, done, cfl, trace, info, margin, _ = _raw(lib, seam, **ok)
    want = B.advect_band(phi0, mask0, (u0, v0, w0), f0, dx, dt, 2)
    assert rc == 0 and done == 2 and cfl == want.cfl and list(trace[:2]) == want.change and np.all(trace[2:] == -7.0)
    assert info == [want.cells, want.edge_cells, want.edge_flips] and margin == want.margin
    assert np.array_equal(_host(phi, phi0.shape) if seam == "device" else phi, want.field)
    with pytest.raises(lsf.LsfError) as e:
        lsf.advectFieldBand(mk(phi0), mk(mask0), *n, dx, dt, 2, speed=badf)
    assert e.value.code == _lib.LSF_ERR_INVALID and "3 non-finite" in str(e.value)


@pytest.mark.parametrize("seam", SEAMS)
def test_zero_steps_empty_list_and_a_nan(lsf, seam):
    phi0, mask, vel, F, n, dx, dt = _inputs("general", "both")
    want0 = _want("general", "both", "rk3", 0)
    got, rep = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, 0)
    assert rep.steps == 0 and rep.change == [] and rep.edge_flips == 0 and np.array_equal(got, phi0)
    _assert_report(rep, want0)
    # an empty list: 1s on wall points only
    walls = np.zeros(phi0.shape, np.int32, order="F")
    walls[0, :, :], walls[:, -1, :] = 1, 1
    got, rep = _run(lsf, seam, phi0, walls, vel, F, n, dx, dt, 3)
    assert np.array_equal(got, phi0)
    assert (rep.steps, rep.cfl, rep.change, rep.cells, rep.edge_cells, rep.edge_flips, rep.margin) == (0, 0.0, [], 0, 0, 0, math.inf)
    # a NaN planted in phi at one list cell
    bad = phi0.copy(order="F")
    bad[tuple(np.argwhere(B.list_of(mask))[1000])] = np.nan
    want = B.advect_band(bad, mask, vel, F, dx, dt, 3)
    assert want.nan and want.steps == 1 and math.isnan(want.change[0])
    with pytest.raises(lsf.LsfNaNError) as e:
        _run(lsf, seam, bad, mask, vel, F, n, dx, dt, 3)
    rep = e.value.report
    assert rep.steps == 1 and len(rep.change) == 1 and math.isnan(rep.change[0]) and rep.cfl == want.cfl
    assert (rep.cells, rep.edge_cells, rep.edge_flips, rep.margin) == (None, None, None, None)  # reported on LSF_OK only


# ---------------------------------------------------------------------------------- 7: a list longer than one entry per thread
# The scan and the closing pass run at most 1024 blocks of 256 threads (ADV_SCAN_BLOCKS in csrc/lsf_advect_field.hpp): beyond
# 262 144 list cells a thread takes a second entry.  72^3 cells, every interior point in the list: 71^3 = 357 911 entries.
# steps = 0 still runs the scan, the edge pass and the closing pass; what they report is computed here directly.
BIG = (73, 73, 73)
BIG_SPOTS = {"first": ((1, 1, 1), (1, 1, 1)), "middle": ((36, 36, 36), (1, 36, 36)), "last": ((71, 71, 71), (71, 71, 71))}


@functools.lru_cache(maxsize=None)
def _big():
    """(phi, u, v, w, f, interior, edge): |phi| in [1, 2), the inputs in [-1, 1); edge = the wall-adjacent interior points, the only
    list cells with a neighbour outside the list when every interior point is in it"""
    rng = np.random.default_rng(72)
    phi = np.asfortranarray((1.0 + rng.random(BIG)) * np.where(rng.random(BIG) < 0.5, -1.0, 1.0))
    u, v, w, f = (np.asfortranarray(rng.uniform(-1.0, 1.0, BIG)) for _ in range(4))
    interior = np.zeros(BIG, bool)
    interior[1:-1, 1:-1, 1:-1] = True
    edge = interior.copy()
    edge[2:-2, 2:-2, 2:-2] = False
    for a in (phi, u, v, w, f, interior, edge):
        a.setflags(write=False)
    return phi, u, v, w, f, interior, edge


@pytest.mark.parametrize("spot", list(BIG_SPOTS))
def test_a_list_longer_than_one_entry_per_thread(lsf, spot):
    phi0, u0, v0, w0, f0, interior, edge = _big()
    assert interior.sum() == 357911 > 1024 * 256 and edge.sum() == 71 ** 3 - 69 ** 3
    at_max, at_min = BIG_SPOTS[spot]
    assert interior[at_max] and edge[at_min]
    phi, u, v, w, f = (a.copy(order="F") for a in (phi0, u0, v0, w0, f0))
    u[at_max], v[at_max], w[at_max], f[at_max] = 2.0, -3.0, 1.5, -2.5  # |u| + |v| + |w| + |speed| = 9 there, below 4 elsewhere
    phi[at_min] = -0.125  # the smallest |phi| of an edge cell
    phi[36, 35, 36] = 0.0625  # a smaller one at a cell that is no edge cell
    dx, dt = 1.0 / 72, 0.25 / 72
    s = (np.abs(u) + np.abs(v)) + np.abs(w)
    s = s + np.abs(f)
    want_cfl = (dt * s[interior].max()) / dx
    assert s[interior].max() == 9.0 == s[at_max] and np.abs(phi[edge]).min() == 0.125
    mask = np.ones(BIG, np.int32, order="F")
    got, rep = _run(lsf, "device", phi, mask, (u, v, w), f, (72, 72, 72), dx, dt, 0)
    print(f"{spot}: cfl {rep.cfl!r} (want {want_cfl!r}), cells {rep.cells}, edge {rep.edge_cells}, flips {rep.edge_flips}, margin {rep.margin!r}")
    assert np.array_equal(got, phi)
    assert rep.steps == 0 and rep.change == [] and rep.cfl == want_cfl
    assert (rep.cells, rep.edge_cells, rep.edge_flips) == (357911, int(edge.sum()), 0)
    assert rep.margin == 0.125


def test_a_long_list_counts_its_non_finite_inputs(lsf):
    from levelsetfortran_amd import _lib

    phi0, u0, v0, w0, f0, interior, _ = _big()
    u = u0.copy(order="F")
    for at, _ in BIG_SPOTS.values():
        u[at] = np.nan
    u[0, 5, 5] = np.nan  # a wall point: not a list cell, legal
    mask = np.ones(BIG, np.int32, order="F")
    with pytest.raises(lsf.LsfError) as e:
        _run(lsf, "device", phi0, mask, (u, v0, w0), f0, (72, 72, 72), 1.0 / 72, 0.25 / 72, 0)
    assert e.value.code == _lib.LSF_ERR_INVALID and "3 non-finite" in str(e.value), str(e.value)
