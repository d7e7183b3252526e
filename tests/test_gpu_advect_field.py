"""lsf_advect_field on the GPU against tests/advect_ref.py, the numpy restatement of the contract in include/lsf.h.  With the STRICT
arithmetic the field (walls included), the change trace and the CFL number are compared with `==`; FAST within the project's 1e-12
RMS of STRICT.

Grids (points per axis), the smallest on which each piece of the kernel can go wrong: (40,33,27) the general case; (10,10,10)
exactly one WENO cell; (9,12,10) none, all first order; (5,5,5); (70,21,45) more than the 64 lanes of a block in x with a ragged
last block; (13,11,75) longer in z than the 32 planes one block marches (ADV_KC in csrc/lsf_advect_field.hpp): three chunks, the
last one partial."""
import ctypes
import functools

import numpy as np
import pytest

import advect_ref as R

pytestmark = pytest.mark.gpu

FAST_RMS_TOL = 1.0e-12  # tests/test_gpu_parity.py
MARCH_CHUNK = 32  # ADV_KC
assert 75 - 2 > 2 * MARCH_CHUNK  # the interior planes of (13,11,75): two full chunks and a partial one

GRIDS = [(40, 33, 27), (10, 10, 10), (9, 12, 10), (5, 5, 5), (70, 21, 45), (13, 11, 75)]
RAGGED = [(70, 21, 45), (13, 11, 75)]  # the two spheres lie outside these: one off-centre sphere, as tests/test_gpu_reinit_band.py
TERMS = ["velocity", "speed", "both"]
SCHEMES = [("rk3", 3), ("euler", 4)]
# ... and, on the smallest grid with a WENO cell, runs that reach the host's look at the stop flag (every 8 steps): Euler with an odd count
# ends in the second buffer after a look at step 8; RK3 with 8 steps ends on the step whose look is left out because it is the last
STRICT_CASES = [(g, t, sc, st) for g in GRIDS for t in TERMS for sc, st in SCHEMES] + [((10, 10, 10), "both", "euler", 9), ((10, 10, 10), "both", "rk3", 8)]
SEAMS = ["host", "device"]


def _gid(g):
    return "x".join(map(str, g))


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _inputs(npts, terms):
    """(phi0, vel or None, F or None, (nx, ny, nz), dx, dt): dt puts the CFL number of the terms present at 0.5"""
    from levelsetfortran_amd import fields

    if npts in RAGGED:
        phi0, dx = fields.sphere_phi0(npts, radius=0.7, centers=((0.1, -0.2, 0.05),))
    else:
        phi0, dx = fields.two_sphere_phi0(npts)
    u, v, w, f, _ = R.wavy_inputs(npts)
    vel = (u, v, w) if terms in ("velocity", "both") else None
    F = f if terms in ("speed", "both") else None
    dt = 0.5 * dx / R.max_speed(vel, F)
    for a in (phi0, u, v, w, f):
        a.setflags(write=False)  # shared between the tests: nobody changes them
    return phi0, vel, F, tuple(n - 1 for n in npts), dx, dt


@functools.lru_cache(maxsize=None)
def _want(npts, terms, scheme, steps):
    phi0, vel, F, _, dx, dt = _inputs(npts, terms)
    field, change, cfl = R.advect(phi0, vel, F, dx, dt, steps, scheme)
    assert len(change) == steps and abs(cfl - 0.5) < 1e-9
    field.setflags(write=False)
    return field, change, cfl


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _run(lsf, seam, phi0, vel, F, n, dx, dt, steps, **kw):
    """advectField on fresh copies through one seam; returns (field, report); asserts that the inputs are unchanged"""
    nx, ny, nz = n
    ins = ([] if vel is None else list(vel)) + ([] if F is None else [F])
    if seam == "host":
        got = phi0.copy(order="F")
        cp = [a.copy(order="F") for a in ins]
        args = cp
    else:
        got = _dev(phi0)
        args = [_dev(a) for a in ins]
    velocity = tuple(args[:3]) if vel is not None else None
    speed = args[-1] if F is not None else None
    rep = lsf.advectField(got, nx, ny, nz, dx, dt, steps, velocity=velocity, speed=speed, **kw)
    for a, b in zip(args, ins):
        back = a if seam == "host" else _host(a, b.shape)
        assert np.array_equal(back, b) and np.array_equal(np.signbit(back), np.signbit(b))  # read, never written
    return (got if seam == "host" else _host(got, phi0.shape)), rep


# ---------------------------------------------------------------------------------- 1: STRICT == the statement
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("npts,terms,scheme,steps", STRICT_CASES, ids=lambda v: _gid(v) if isinstance(v, tuple) else None)
def test_strict_is_bit_identical_to_the_statement(lsf, oracle, npts, terms, scheme, steps, seam):
    phi0, vel, F, n, dx, dt = _inputs(npts, terms)
    want, change, cfl = _want(npts, terms, scheme, steps)
    got, rep = _run(lsf, seam, phi0, vel, F, n, dx, dt, steps, scheme=scheme, arith="strict")
    diff = np.abs(got - want)
    print(f"{_gid(npts)} {terms} {scheme} {seam}: max |got - want| = {diff.max():.3e} at {np.unravel_index(diff.argmax(), diff.shape)}, "
          f"cfl {rep.cfl!r}, change {rep.change}")
    assert rep.steps == steps and rep.cfl == cfl
    assert np.array_equal(got, want)  # the whole field, walls included
    assert rep.change == change
    assert not np.array_equal(got, phi0)


# ---------------------------------------------------------------------------------- 2: streams, no state between calls, run to run
@pytest.mark.parametrize("scheme", ["rk3", "euler"])
def test_side_stream_split_calls_and_run_to_run(lsf, oracle, scheme):
    import torch

    npts, terms = (40, 33, 27), "both"
    phi0, vel, F, n, dx, dt = _inputs(npts, terms)
    want, change, cfl = _want(npts, terms, scheme, 4)
    nx, ny, nz = n
    outs = []
    for _ in range(2):  # the second run of a call equals the first
        t, ins = _dev(phi0), [_dev(a) for a in (*vel, F)]
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            rep = lsf.advectField(t, nx, ny, nz, dx, dt, 4, velocity=tuple(ins[:3]), speed=ins[3], scheme=scheme)
        torch.cuda.synchronize()
        assert rep.steps == 4 and rep.change == change and rep.cfl == cfl
        outs.append(_host(t, phi0.shape))
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    # one call of 4 steps equals two calls of 2 (each seam)
    for seam in SEAMS:
        half, rep1 = _run(lsf, seam, phi0, vel, F, n, dx, dt, 2, scheme=scheme)
        full, rep2 = _run(lsf, seam, half, vel, F, n, dx, dt, 2, scheme=scheme)
        assert np.array_equal(full, want) and rep1.change + rep2.change == change


# ---------------------------------------------------------------------------------- 3: FAST within 1e-12 RMS of STRICT
@pytest.mark.parametrize("scheme,steps", SCHEMES)
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("npts", GRIDS, ids=_gid)
def test_fast_arithmetic_within_tolerance_of_strict(lsf, oracle, npts, terms, scheme, steps):
    phi0, vel, F, n, dx, dt = _inputs(npts, terms)
    want, change, cfl = _want(npts, terms, scheme, steps)
    got, rep = _run(lsf, "device", phi0, vel, F, n, dx, dt, steps, scheme=scheme, arith="fast")
    rms = float(np.sqrt(np.mean((got - want) ** 2)))
    print(f"{_gid(npts)} {terms} {scheme}: FAST against STRICT rms {rms:.3e}, max {np.abs(got - want).max():.3e}, "
          f"change rel {max(abs(a / b - 1) for a, b in zip(rep.change, change)):.3e}")
    assert rep.steps == steps and rep.cfl == cfl  # the CFL number has one arithmetic
    assert rms <= FAST_RMS_TOL


# ---------------------------------------------------------------------------------- 4: the closed form on the GPU
def test_translated_sphere_is_the_statements_field(lsf, oracle):
    """The translate case of tests/test_advect_field_cpu.py at 49 points, RK3: by bit-identity its error IS the CPU test's."""
    phi0, vel, F, dx, dt, steps, exact = R.closed_form_case(49, "translate")
    want, change, cfl, err, _ = R.closed_form_run(49, "translate", "rk3")
    got, rep = _run(lsf, "device", phi0, vel, F, (48, 48, 48), dx, dt, steps)
    print(f"translate, 49 points, {steps} steps: max error near the surface {R.band_error(got, exact, dx) / dx:.3e} dx (statement {err / dx:.3e} dx)")
    assert steps == 17 and rep.steps == 17
    assert np.array_equal(got, want) and rep.change == change and rep.cfl == cfl
    assert R.band_error(got, exact, dx) == err


def test_host_inputs_are_read_from_the_host_not_from_an_earlier_twin(lsf, oracle):
    """Without lsf_mirror the host copy of an input is the truth: the array that was phi in one host-seam call (and so has a device
    twin holding that call's result) is overwritten on the host and handed in as the speed of the next call."""
    npts = (12, 11, 10)
    n = tuple(v - 1 for v in npts)
    phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
    u, v, w, f, smax = R.wavy_inputs(npts)
    dt = 0.5 * dx / smax
    a = phi0.copy(order="F")
    lsf.advectField(a, *n, dx, dt, 1, velocity=(u, v, w), speed=f)
    a[...] = f  # same address, same size, new content
    b = phi0.copy(order="F")
    rep = lsf.advectField(b, *n, dx, dt, 2, speed=a, scheme="euler")
    want, change, cfl = R.advect(phi0, None, f, dx, dt, 2, "euler")
    assert rep.cfl == cfl and rep.change == change and np.array_equal(b, want) and np.array_equal(a, f)


# ---------------------------------------------------------------------------------- 5: errors and edges
def _raw(lib, seam, phi, u, v, w, f, n, dx, dt, steps, scheme, mode):
    done, cfl = ctypes.c_int(-7), ctypes.c_double(-7.0)
    trace = np.full(8, -7.0)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(u), ptr(v), ptr(w), ptr(f), n[0], n[1], n[2], dx, dt, steps, scheme, mode, ctypes.byref(done), ctypes.byref(cfl),
            trace.ctypes.data, 8)
    rc = lib.lsf_advect_field_device(*args, None) if seam == "device" else lib.lsf_advect_field(*args)
    return rc, done.value, cfl.value, trace, (lib.lsf_last_error() or b"").decode()


@pytest.mark.parametrize("seam", SEAMS)
def test_invalid_arguments_leave_phi_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    npts = (12, 11, 10)
    n = tuple(v - 1 for v in npts)
    phi0, dx = R.sphere_distance(npts, (0.1, 0.0, -0.1), 0.6)
    u0, v0, w0, f0, smax = R.wavy_inputs(npts)
    dt = 0.5 * dx / smax
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    phi, u, v, w, f = (mk(a) for a in (phi0, u0, v0, w0, f0))
    bad = f0.copy(order="F")
    bad[3, 4, 5], bad[0, 0, 0], bad[11, 10, 9] = np.nan, np.inf, -np.inf  # an interior point, two wall corners
    badf = mk(bad)
    ok = dict(phi=phi, u=u, v=v, w=w, f=f, n=n, dx=dx, dt=dt, steps=2, scheme=_lib.LSF_ADVECT_RK3, mode=_lib.LSF_ORDER_JACOBI | _lib.LSF_ARITH_STRICT)
    cases = {
        "NULL phi": dict(phi=None),
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
        rc, done, cfl, trace, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and done == -7 and cfl == -7.0 and np.all(trace == -7.0), name  # nothing reported either
        if name.startswith("non-finite"):
            assert "3 non-finite" in msg, msg
        back = _host(phi, phi0.shape) if seam == "device" else phi
        assert np.array_equal(back, phi0), name
    # a valid call follows: the library is in working order, and the Python layer raises the same error
    rc, done, cfl, trace, _ = _raw(lib, seam, **ok)
    want, change, cfl_want = R.advect(phi0, (u0, v0, w0), f0, dx, dt, 2)
    assert rc == 0 and done == 2 and cfl == cfl_want and list(trace[:2]) == change and np.all(trace[2:] == -7.0)
    assert np.array_equal(_host(phi, phi0.shape) if seam == "device" else phi, want)
    with pytest.raises(lsf.LsfError) as e:
        lsf.advectField(mk(phi0), *n, dx, dt, 2, speed=badf)
    assert e.value.code == _lib.LSF_ERR_INVALID and "3 non-finite" in str(e.value)


@pytest.mark.parametrize("seam", SEAMS)
def test_zero_steps_and_a_nan(lsf, oracle, seam):
    npts, terms = (40, 33, 27), "both"
    phi0, vel, F, n, dx, dt = _inputs(npts, terms)
    got, rep = _run(lsf, seam, phi0, vel, F, n, dx, dt, 0)
    assert rep.steps == 0 and rep.change == [] and rep.cfl == R.cfl_number(vel, F, dx, dt) and np.array_equal(got, phi0)
    bad = phi0.copy(order="F")
    bad[20, 16, 13] = np.nan
    want, change, cfl = R.advect(bad, vel, F, dx, dt, 3)
    assert len(change) == 1 and np.isnan(change[0])
    with pytest.raises(lsf.LsfNaNError) as e:
        _run(lsf, seam, bad, vel, F, n, dx, dt, 3)
    rep = e.value.report
    assert rep.steps == 1 and len(rep.change) == 1 and np.isnan(rep.change[0]) and rep.cfl == cfl
