"""lsf_evolve_band on the GPU against tests/evolve_band_ref.py, the serial statement of the contract in include/lsf.h.  With the
STRICT arithmetic phi, mask, trace, cfl, info and margin are compared with `==` on both seams; FAST takes the same schedule and stays
within the project's 1e-12 RMS of STRICT over the final list (the bound of tests/test_gpu_advect_field.py).

Every case starts from the distance to a sphere clamped to +-far, far = (core + ring) dx, with the mask |distance| < far, and moves
it at the given CFL number (a chunk is 256 list entries, MB_CH in csrc/lsf_minmax_band.hpp):
  small     (14,13,12), u = (1,0,0), core 1.5, ring 2, 1 sweep, 6 steps: 668 cells, one rebuild after the fourth step, 248 cells
            enter; wall-adjacent list cells are present, so the open-edge rule matters
  general   (40,33,27), u = (1,.5,-.25), core 3, ring 3, 2 sweeps, 16 steps: 5 893 cells (24 chunks, ragged) grow past 32 chunks;
            a rebuild after the seventh step and at least one more
  both      general with the speed 0.5 beside the velocity
  grow      (24,22,20), speed 1, core 2, ring 3, 2 sweeps, 8 steps: the list goes 1 626 -> 5 616, every workspace slot grows mid-call
  euler     (24,22,20), u = (1,.3,0), Euler, CFL 0.3, core 2, ring 3, 2 sweeps, 9 steps: no rebuild, an odd step count
  thinflip  20^3, u = (1,0,0), the mask |phi| < 0.6 dx, core .25, ring 1, no sweeps: ends after the first step with 44 flips
  big       (section 7, its own fields) 73^3 points, every interior point, steps = 0: more than one entry per thread of scan and check
The properties are asserted on the statement first (test_the_cases_show_their_properties): a case that stops exercising its path
fails loudly."""
import ctypes
import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R
import evolve_band_ref as V

pytestmark = pytest.mark.gpu

FAST_RMS_TOL = 1.0e-12  # tests/test_gpu_advect_field.py
CHUNK = 256  # MB_CH
SEAMS = ["host", "device"]


class Case(NamedTuple):
    npts: Tuple[int, int, int]
    centre: Tuple[float, float, float]
    radius: float
    u: Optional[Tuple[float, float, float]]
    speed: Optional[float]
    core: float
    ring: int
    sweeps: int
    steps: int
    cfl: float
    scheme: str = "rk3"
    thin: Optional[float] = None  # the mask is |phi| < thin dx instead of |phi| < far


CASES = {
    "small": Case((14, 13, 12), (-0.1, -0.2, -0.3), 0.45, (1, 0, 0), None, 1.5, 2, 1, 6, 0.5),
    "general": Case((40, 33, 27), (-0.25, -0.3, -0.5), 0.4, (1, .5, -.25), None, 3, 3, 2, 16, 0.5),
    "both": Case((40, 33, 27), (-0.25, -0.3, -0.5), 0.4, (1, .5, -.25), 0.5, 3, 3, 2, 16, 0.5),
    "grow": Case((24, 22, 20), (0, -0.1, -0.25), 0.3, None, 1.0, 2, 3, 2, 8, 0.5),
    "euler": Case((24, 22, 20), (-0.1, -0.1, -0.25), 0.4, (1, .3, 0), None, 2, 3, 2, 9, 0.3, "euler"),
    "rk3twin": Case((24, 22, 20), (-0.1, -0.1, -0.25), 0.4, (1, .3, 0), None, 2, 3, 2, 9, 0.3, "rk3"),
    "thinflip": Case((20, 20, 20), (-0.1, 0, 0), 0.5, (1, 0, 0), None, .25, 1, 0, 4, 0.5, "rk3", 0.6),
}
STRICT_CASES = ["small", "general", "both", "grow", "euler", "thinflip"]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(phi0, mask, vel or None, F or None, (nx, ny, nz), dx, dt, keywords of the call); shared and read-only"""
    c = CASES[case]
    dist, dx = R.sphere_distance(c.npts, c.centre, c.radius)
    far = (c.core + float(c.ring)) * dx
    phi0 = np.asfortranarray(np.clip(dist, -far, far))
    mask = np.asfortranarray((np.abs(dist) < (far if c.thin is None else c.thin * dx)).astype(np.int32))
    vel = None if c.u is None else tuple(np.asfortranarray(np.full(c.npts, float(x))) for x in c.u)
    F = None if c.speed is None else np.asfortranarray(np.full(c.npts, float(c.speed)))
    dt = c.cfl * dx / R.max_speed(vel, F)
    for a in (phi0, mask) + (vel or ()) + ((F,) if F is not None else ()):
        a.setflags(write=False)
    kw = dict(scheme=c.scheme, core=float(c.core), ring=c.ring, reinit_sweeps=c.sweeps, h=0.5 * dx)
    return phi0, mask, vel, F, tuple(n - 1 for n in c.npts), dx, dt, kw


@functools.lru_cache(maxsize=None)
def _want(case, steps=None, check_every=1):
    phi0, mask, vel, F, _, dx, dt, kw = _inputs(case)
    r = V.evolve_band(phi0, mask, vel, F, dx, dt, CASES[case].steps if steps is None else steps, check_every=check_every, **kw)
    assert not r.nan
    r.field.setflags(write=False), r.mask.setflags(write=False)
    # FAST must take the same schedule: no margin of a check within 1e-6 dx of the threshold (the statement's stay 0.01 dx away)
    core_dx = CASES[case].core * dx
    assert all(abs(m - core_dx) >= 1e-6 * dx for m in r.margins), (case, [m / dx for m in r.margins])
    return r


def test_the_cases_show_their_properties():
    cells0 = lambda case: int(B.list_of(_inputs(case)[1]).sum())
    r = _want("small")
    assert cells0("small") == 668 and (r.steps, r.rebuilt_after, r.entered, r.flips) == (6, [4], 248, 0)
    lst = r.mask == 1
    assert V.near_wall_of(lst).sum() > 0 and B.edge_of(lst).sum() > V.open_edge_of(lst).sum()  # the open-edge rule matters
    for case in ("general", "both"):
        r = _want(case)
        n0 = cells0(case)
        assert n0 == 5893 and (n0 + CHUNK - 1) // CHUNK == 24 and n0 % CHUNK != 0
        assert r.steps == 16 and r.rebuilds >= 2 and r.flips == 0 and (r.cells + CHUNK - 1) // CHUNK >= 32 and r.cells % CHUNK != 0
    assert _want("general").rebuilt_after[0] == 7 and _want("general", 8).cells == 8068
    assert (-(-8068 // CHUNK)) == 32
    r = _want("grow")
    assert cells0("grow") == 1626 and (r.cells, r.rebuilds, r.steps, r.flips) == (5616, 1, 8, 0)
    for case in ("euler", "rk3twin"):
        r = _want(case)
        assert (r.steps, r.rebuilds, r.flips) == (9, 0, 0) and r.cfl == pytest.approx(0.3)
    r = _want("thinflip")
    assert (r.steps, r.flips, r.rebuilds) == (1, 44, 0)
    assert all(abs(_want(c).cfl - CASES[c].cfl) < 1e-12 for c in CASES)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, steps, **kw):
    """evolveBand on fresh copies through one seam; returns (field, mask, report); asserts that the inputs are unchanged.  With
    `raises` the exception is returned in place of the report."""
    nx, ny, nz = n
    raises = kw.pop("raises", None)
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
        if raises is None:
            rep = lsf.evolveBand(got, m, nx, ny, nz, dx, dt, steps, velocity=velocity, speed=speed, **kw)
        else:
            with pytest.raises(raises) as e:
                lsf.evolveBand(got, m, nx, ny, nz, dx, dt, steps, velocity=velocity, speed=speed, **kw)
            rep = e.value
    finally:
        for a, b in zip(args, ins):
            assert np.array_equal(a if seam == "host" else _host(a, b.shape), b)  # read, never written
    if seam == "device":
        got, m = _host(got, phi0.shape), _host(m, mask.shape)
    return got, m, rep


def _assert_report(rep, want):
    assert rep.steps == want.steps and rep.cfl == want.cfl and rep.change == want.change
    assert (rep.cells, rep.open_cells, rep.flips, rep.rebuilds, rep.entered, rep.near_wall) == \
        (want.cells, want.open_cells, want.flips, want.rebuilds, want.entered, want.near_wall)
    assert rep.margin == want.margin


def _assert_equal(case, got, m, rep, want, label=""):
    diff = np.abs(got - want.field)
    print(f"{case} {label}: max |got - want| = {np.nanmax(diff):.3e} at {np.unravel_index(np.nanargmax(diff), diff.shape)}, mask differs at "
          f"{int((m != want.mask).sum())}, report {rep}, want rebuilds after {want.rebuilt_after}, margin {want.margin!r}")
    assert np.array_equal(m, want.mask)
    assert np.array_equal(got, want.field)  # the whole field: nothing outside the lists is written
    _assert_report(rep, want)


# ---------------------------------------------------------------------------------- 1: STRICT == the statement
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("case", STRICT_CASES)
def test_strict_is_bit_identical_to_the_statement(lsf, case, seam):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs(case)
    want = _want(case)
    got, m, rep = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, CASES[case].steps, **kw)
    _assert_equal(case, got, m, rep, want, seam)


@pytest.mark.parametrize("check_every", [1, 3])
def test_check_every(lsf, check_every):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs("general")
    want = _want("general", None, check_every)
    assert want.rebuilds >= 1 and all(s % check_every == 0 or s == 16 for s in want.rebuilt_after)
    got, m, rep = _run(lsf, "device", phi0, mask, vel, F, n, dx, dt, 16, check_every=check_every, **kw)
    _assert_equal("general", got, m, rep, want, f"check_every {check_every}")


# ---------------------------------------------------------------------------------- 2: no rebuild = the public calls
@pytest.mark.parametrize("case", ["euler", "rk3twin"])
def test_without_a_rebuild_the_loop_is_the_public_calls(lsf, case):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs(case)
    assert _want(case).rebuilds == 0
    c = CASES[case]
    loop, m, ins = _dev(phi0), _dev(mask), tuple(_dev(a) for a in vel)
    for _ in range(c.steps):
        lsf.advectFieldBand(loop, m, *n, dx, dt, 1, velocity=ins, scheme=c.scheme, arith="strict")
        lsf.reinitBand(loop, m, *n, c.sweeps - 1, dx, 0.5 * dx, tol=0.0, arith="strict")
    one, m1 = _dev(phi0), _dev(mask)
    rep = lsf.evolveBand(one, m1, *n, dx, dt, c.steps, velocity=ins, arith="strict", **kw)
    assert rep.steps == c.steps and rep.rebuilds == 0
    import torch

    assert torch.equal(one, loop) and torch.equal(m1, m)


# ---------------------------------------------------------------------------------- 3: calls compose, streams, run to run
@pytest.mark.parametrize("seam", SEAMS)
def test_eight_steps_are_four_and_four(lsf, seam):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs("grow")
    want = _want("grow")
    assert want.rebuilt_after == [5]  # in the second half
    half, mh, rep1 = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, 4, **kw)
    _assert_equal("grow", half, mh, rep1, _want("grow", 4), f"{seam}, first half")
    full, mf, rep2 = _run(lsf, seam, half, mh, vel, F, n, dx, dt, 4, **kw)
    assert np.array_equal(full, want.field) and np.array_equal(mf, want.mask) and rep1.change + rep2.change == want.change
    assert rep1.cfl == rep2.cfl == want.cfl and rep2.margin == want.margin and rep1.rebuilds + rep2.rebuilds == want.rebuilds
    assert (rep2.cells, rep2.open_cells, rep2.entered) == (want.cells, want.open_cells, want.entered)


def test_side_stream_twice(lsf):
    import torch

    phi0, mask, vel, F, n, dx, dt, kw = _inputs("general")
    want = _want("general")
    for _ in range(2):  # the second run of a call equals the first
        t, m, ins = _dev(phi0), _dev(mask), tuple(_dev(a) for a in vel)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            rep = lsf.evolveBand(t, m, *n, dx, dt, 16, velocity=ins, **kw)
        torch.cuda.synchronize()
        _assert_equal("general", _host(t, phi0.shape), _host(m, mask.shape), rep, want, "side stream")


# ---------------------------------------------------------------------------------- 4: the mask
@pytest.mark.parametrize("seam", SEAMS)
def test_a_mask_of_many_values_comes_back_zero_one(lsf, seam):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs("small")
    want = _want("small")
    lst = B.list_of(mask)
    ijk = np.add.outer(np.add.outer(np.arange(phi0.shape[0]), np.arange(phi0.shape[1])), np.arange(phi0.shape[2])) % 3
    wild = np.where(lst, 1, np.choose(ijk, [7, -1, 0])).astype(np.int32)  # off the list: 7, -1 and 0 in turn
    for a in range(3):  # 1s on all six walls: ignored
        sl = [slice(None)] * 3
        for side in (0, -1):
            sl[a] = side
            wild[tuple(sl)] = 1
    wild = np.asfortranarray(wild)
    inner = wild[1:-1, 1:-1, 1:-1]
    assert (inner == 7).any() and (inner == -1).any() and (inner == 0).any() and np.array_equal(B.list_of(wild), lst) and wild.sum() != mask.sum()
    for steps in (6, 0):
        got, m, rep = _run(lsf, seam, phi0, wild, vel, F, n, dx, dt, steps, **kw)
        _assert_equal("small", got, m, rep, _want("small", steps), f"{seam}, wild mask, {steps} steps")
        assert set(np.unique(m)) == {0, 1}
    # an empty list: 1s on wall points only
    walls = np.asfortranarray(np.where(lst, 0, wild).astype(np.int32))
    walls[1:-1, 1:-1, 1:-1][walls[1:-1, 1:-1, 1:-1] == 1] = 0
    assert (walls == 1).any() and not B.list_of(walls).any()
    got, m, rep = _run(lsf, seam, phi0, walls, vel, F, n, dx, dt, 3, **kw)
    assert np.array_equal(got, phi0) and not m.any()
    assert tuple(rep) == (0, 0.0, [], 0, 0, 0, 0, 0, 0, math.inf)


# ---------------------------------------------------------------------------------- 5: errors and edges
def _raw(lib, seam, phi, mask, u, v, w, f, n, dx, dt, steps, scheme, mode, core, ring, sweeps, h, check_every):
    done, cfl, margin = ctypes.c_int(-7), ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    trace = np.full(8, -7.0)
    info = np.full(6, -7, np.int64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), ptr(u), ptr(v), ptr(w), ptr(f), n[0], n[1], n[2], dx, dt, steps, scheme, mode, core, ring, sweeps, h, check_every,
            ctypes.byref(done), ctypes.byref(cfl), trace.ctypes.data, 8, info.ctypes.data, ctypes.byref(margin))
    rc = lib.lsf_evolve_band_device(*args, None) if seam == "device" else lib.lsf_evolve_band(*args)
    return rc, done.value, cfl.value, trace, list(info), margin.value, (lib.lsf_last_error() or b"").decode()


@pytest.mark.parametrize("seam", SEAMS)
def test_invalid_arguments_leave_phi_and_mask_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask0, (u0, v0, w0), _, n, dx, dt, kw = _inputs("small")
    f0 = np.asfortranarray(np.full(phi0.shape, 0.25))
    mask0 = mask0.copy(order="F")
    mask0[0], mask0[2, 2, 2] = 1, 7  # not normalised: an invalid call must leave it so
    lst = B.list_of(mask0)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    phi, mask, u, v, w, f = (mk(a) for a in (phi0, mask0, u0, v0, w0, f0))
    bad = f0.copy(order="F")
    bad[tuple(np.argwhere(lst)[0])], bad[0, 0, 0], bad[tuple(np.argwhere(~lst)[-1])] = np.nan, np.inf, -np.inf  # on the list, a wall, off it
    badf = mk(bad)
    nan, inf = float("nan"), float("inf")
    ok = dict(phi=phi, mask=mask, u=u, v=v, w=w, f=f, n=n, dx=dx, dt=dt, steps=2, scheme=_lib.LSF_ADVECT_RK3,
              mode=_lib.LSF_ORDER_JACOBI | _lib.LSF_ARITH_STRICT, core=1.5, ring=2, sweeps=1, h=0.5 * dx, check_every=1)
    cases = {
        "NULL phi": dict(phi=None), "NULL mask": dict(mask=None), "partial velocity": dict(w=None), "one component": dict(u=None, v=None),
        "neither": dict(u=None, v=None, w=None, f=None), "nx < 2": dict(n=(1, n[1], n[2])), "nz < 2": dict(n=(n[0], n[1], 0)),
        "dx = 0": dict(dx=0.0), "dx NaN": dict(dx=nan), "dt < 0": dict(dt=-dt), "dt inf": dict(dt=inf), "steps < 0": dict(steps=-1),
        "scheme": dict(scheme=2), "GS order": dict(mode=_lib.LSF_ORDER_GS | _lib.LSF_ARITH_STRICT), "unknown order": dict(mode=7),
        "core = 0": dict(core=0.0), "core < 0": dict(core=-1.0), "core NaN": dict(core=nan), "core inf": dict(core=inf),
        "ring = 0": dict(ring=0), "ring = 9": dict(ring=9), "sweeps < 0": dict(sweeps=-1), "h = 0": dict(h=0.0), "h NaN": dict(h=nan),
        "h inf": dict(h=inf), "check_every = 0": dict(check_every=0),
        "non-finite speed": dict(f=badf), "non-finite velocity": dict(v=badf, f=None),
    }
    for name, change in cases.items():
        rc, done, cfl, trace, info, margin, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and done == -7 and cfl == -7.0 and np.all(trace == -7.0) and info == [-7] * 6 and margin == -7.0, name  # nothing reported
        if name.startswith("non-finite"):
            assert "3 non-finite" in msg, msg
        back, mback = (_host(phi, phi0.shape), _host(mask, mask0.shape)) if seam == "device" else (phi, mask)
        assert np.array_equal(back, phi0) and np.array_equal(mback, mask0), name
    # h is not looked at without sweeps
    rc = _raw(lib, seam, **dict(ok, sweeps=0, h=nan, steps=0))[0]
    assert rc == 0
    phi, mask = mk(phi0), mk(mask0)
    # a valid call follows: the library is in working order, and the Python layer raises the same error
    rc, done, cfl, trace, info, margin, _ = _raw(lib, seam, **dict(ok, phi=phi, mask=mask))
    want = V.evolve_band(phi0, mask0, (u0, v0, w0), f0, dx, dt, 2, "rk3", 1.5, 2, 1, 0.5 * dx, 1)
    assert rc == 0 and done == 2 and cfl == want.cfl and list(trace[:2]) == want.change and np.all(trace[2:] == -7.0)
    assert info == [want.cells, want.open_cells, want.flips, want.rebuilds, want.entered, want.near_wall] and margin == want.margin
    back, mback = (_host(phi, phi0.shape), _host(mask, mask0.shape)) if seam == "device" else (phi, mask)
    assert np.array_equal(back, want.field) and np.array_equal(mback, want.mask)
    with pytest.raises(lsf.LsfError) as e:
        lsf.evolveBand(mk(phi0), mk(mask0), *n, dx, dt, 2, speed=badf)
    assert e.value.code == _lib.LSF_ERR_INVALID and "3 non-finite" in str(e.value)


@pytest.mark.parametrize("scheme", ["rk3", "euler"])
@pytest.mark.parametrize("seam", SEAMS)
def test_a_nan_at_a_list_cell(lsf, seam, scheme):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs("general")
    kw = dict(kw, scheme=scheme)
    bad = phi0.copy(order="F")
    bad[tuple(np.argwhere(B.list_of(mask))[1000])] = np.nan
    want = V.evolve_band(bad, mask, vel, F, dx, dt, 3, scheme, 3.0, 3, 2, 0.5 * dx, 1)
    assert want.nan and want.steps == 1 and math.isnan(want.change[0])
    got, m, err = _run(lsf, seam, bad, mask, vel, F, n, dx, dt, 3, raises=lsf.LsfNaNError, **kw)
    rep = err.report
    assert rep.steps == 1 and len(rep.change) == 1 and math.isnan(rep.change[0]) and rep.cfl == want.cfl
    assert tuple(rep)[3:] == (None,) * 7  # info and margin are reported on LSF_OK only
    assert np.array_equal(m, want.mask)  # ... the mask is written
    assert np.array_equal(got, want.field, equal_nan=True)  # the state after the transport of the NaN step: its sweeps are not run


# ---------------------------------------------------------------------------------- 6: FAST against STRICT
def test_fast_takes_the_same_schedule_within_tolerance_of_strict(lsf):
    phi0, mask, vel, F, n, dx, dt, kw = _inputs("general")
    want = _want("general")
    got, m, rep = _run(lsf, "device", phi0, mask, vel, F, n, dx, dt, 16, arith="fast", **kw)
    lst = want.mask == 1
    rms = float(np.sqrt(np.mean((got[lst] - want.field[lst]) ** 2)))
    print(f"general: FAST against STRICT over the final list: rms {rms:.3e}, max {np.abs(got - want.field).max():.3e}, rebuilds {rep.rebuilds}")
    assert np.array_equal(m, want.mask) and rep.rebuilds == want.rebuilds and rep.steps == 16 and rep.cfl == want.cfl
    assert (rep.cells, rep.open_cells, rep.entered, rep.flips) == (want.cells, want.open_cells, want.entered, want.flips)
    assert rms <= FAST_RMS_TOL


# ---------------------------------------------------------------------------------- 7: a list longer than one entry per thread
# The scan of the inputs and the check run at most 1024 blocks of 256 threads (ADV_SCAN_BLOCKS, EVB_CHECK_BLOCKS): beyond 262 144
# entries a thread takes a second one.  72^3 cells, every interior point in the list: 71^3 = 357 911 list cells, 73^3 scanned
# points.  steps = 0 still runs the scan, the first list, the edge pass and the check; what they report is computed here directly:
# the CFL number over ALL points, no open-edge cell (every interior neighbour of a list cell is in the list, so the margin is +inf)
# and the wall-adjacent cells with |phi| < core dx.
BIG = (73, 73, 73)
BIG_SPOTS = {"first": (1, 1, 1), "middle": (36, 36, 36), "last": (71, 71, 71)}
BIG_KW = dict(core=3.0, ring=3, reinit_sweeps=2)


@functools.lru_cache(maxsize=None)
def _big():
    """(phi, u, v, w, f, interior, near): |phi| in [0, 0.1) -- core dx = 3 / 72 lies inside --, the inputs in [-1, 1); near = the
    wall-adjacent interior points"""
    rng = np.random.default_rng(73)
    phi = np.asfortranarray(0.1 * rng.random(BIG) * np.where(rng.random(BIG) < 0.5, -1.0, 1.0))
    u, v, w, f = (np.asfortranarray(rng.uniform(-1.0, 1.0, BIG)) for _ in range(4))
    interior = np.zeros(BIG, bool)
    interior[1:-1, 1:-1, 1:-1] = True
    near = interior.copy()
    near[2:-2, 2:-2, 2:-2] = False
    for a in (phi, u, v, w, f, interior, near):
        a.setflags(write=False)
    return phi, u, v, w, f, interior, near


@pytest.mark.parametrize("spot", list(BIG_SPOTS))
def test_a_list_longer_than_one_entry_per_thread(lsf, spot):
    phi0, u0, v0, w0, f0, interior, near = _big()
    assert interior.sum() == 357911 > 1024 * 256
    at = BIG_SPOTS[spot]
    u, v, w, f = (a.copy(order="F") for a in (u0, v0, w0, f0))
    u[at], v[at], w[at], f[at] = 2.0, -3.0, 1.5, -2.5  # |u| + |v| + |w| + |speed| = 9 there, below 4 elsewhere
    dx, dt = 1.0 / 72, 0.25 / 72
    s = (np.abs(u) + np.abs(v)) + np.abs(w)
    s = s + np.abs(f)
    assert s.max() == 9.0 == s[at]
    want_cfl = (dt * s.max()) / dx
    want_near = int((near & (np.abs(phi0) < 3.0 * dx)).sum())
    assert 0 < want_near < near.sum()
    mask = np.ones(BIG, np.int32, order="F")
    got, m, rep = _run(lsf, "device", phi0, mask, (u, v, w), f, (72, 72, 72), dx, dt, 0, **BIG_KW)
    print(f"{spot}: {rep}, want cfl {want_cfl!r}, near_wall {want_near}")
    assert np.array_equal(got, phi0) and np.array_equal(m, interior.astype(np.int32))
    assert rep.steps == 0 and rep.change == [] and rep.cfl == want_cfl
    assert (rep.cells, rep.open_cells, rep.flips, rep.rebuilds, rep.entered, rep.near_wall) == (357911, 0, 0, 0, 0, want_near)
    assert rep.margin == math.inf


def test_a_long_list_with_open_edge_cells_behind_the_first_entry_per_thread(lsf):
    """The mask of all ones has no open-edge cell.  One interior cell left out, (68,68,68), opens its six neighbours: the list is
    sorted by bricks of 8 x 8 x 4 points, layer k >> 2 first, and all six have k >= 67, behind the 63 * 71 * 71 = 317 583 cells with
    k <= 63 -- second entries of their threads -- so the minimum and the open and flip counts of the check come from there."""
    phi0, u0, v0, w0, f0, interior, near = _big()
    hole = (68, 68, 68)
    opened = [(67, 68, 68), (69, 68, 68), (68, 67, 68), (68, 69, 68), (68, 68, 67), (68, 68, 69)]
    assert 63 * 71 * 71 > 1024 * 256 and min(c[2] for c in opened) >> 2 >= 16
    phi = phi0.copy(order="F")
    for q, c in enumerate(opened):
        phi[c] = (-1.0) ** q * (0.01 + 0.001 * q)  # the smallest |phi| of an open-edge cell is 0.01; both signs: no flip at steps = 0
    phi[hole] = 0.0009765625  # smaller, but not a list cell
    mask = np.ones(BIG, np.int32, order="F")
    mask[hole] = 0
    dx, dt = 1.0 / 72, 0.25 / 72
    s = (np.abs(u0) + np.abs(v0)) + np.abs(w0)
    s = s + np.abs(f0)
    want_near = int((near & (np.abs(phi) < 3.0 * dx)).sum())
    got, m, rep = _run(lsf, "device", phi, mask, (u0, v0, w0), f0, (72, 72, 72), dx, dt, 0, **BIG_KW)
    print(f"hole: {rep}, want near_wall {want_near}")
    want_mask = interior.astype(np.int32)
    want_mask[hole] = 0
    assert np.array_equal(got, phi) and np.array_equal(m, want_mask)
    assert rep.steps == 0 and rep.cfl == (dt * s.max()) / dx
    assert (rep.cells, rep.open_cells, rep.flips, rep.rebuilds, rep.entered, rep.near_wall) == (357910, 6, 0, 0, 0, want_near)
    assert rep.margin == 0.01


def test_a_long_list_counts_its_non_finite_inputs(lsf):
    from levelsetfortran_amd import _lib

    phi0, u0, v0, w0, f0, _, _ = _big()
    u = u0.copy(order="F")
    for at in BIG_SPOTS.values():
        u[at] = np.nan
    phi, mask = _dev(phi0), _dev(np.ones(BIG, np.int32, order="F"))
    with pytest.raises(lsf.LsfError) as e:
        lsf.evolveBand(phi, mask, 72, 72, 72, 1.0 / 72, 0.25 / 72, 0, velocity=tuple(_dev(a) for a in (u, v0, w0)), speed=_dev(f0), **BIG_KW)
    assert e.value.code == _lib.LSF_ERR_INVALID and "3 non-finite" in str(e.value), str(e.value)
    assert np.array_equal(_host(phi, BIG), phi0) and np.all(_host(mask, BIG) == 1)  # refused before anything is written
