"""lsf_evolve_band_curv on the GPU against tests/evolve_band_curv_ref.py, the serial statement of the contract in include/lsf.h.
With the STRICT arithmetic phi, mask, trace, cfl, diffusion, info and margin are compared with `==` on both seams; FAST takes the same
schedule and stays within the project's 1e-12 RMS of STRICT over the final list (the bound of tests/test_gpu_advect_field.py).

The cases -- curvsmall, curvonly, dumbbell, euler -- and what each is for are in tests/evolve_band_curv_cases.py; their properties are
asserted on the statement in tests/test_evolve_band_curv_cpu.py, so a case that stops exercising its path fails loudly."""
import ctypes
import math

import numpy as np
import pytest

import advect_band_ref as B
import evolve_band_curv_cases as K
import evolve_band_curv_ref as VC

pytestmark = pytest.mark.gpu

FAST_RMS_TOL = 1.0e-12  # tests/test_gpu_advect_field.py
SEAMS = ["host", "device"]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, steps, bcurv, **kw):
    """evolveBandCurv (`plain`: evolveBand) on fresh copies through one seam; returns (field, mask, report); asserts that every input
    array is unchanged.  With `raises` the exception is returned in place of the report."""
    nx, ny, nz = n
    raises = kw.pop("raises", None)
    plain = kw.pop("plain", False)
    ins = ([] if vel is None else list(vel)) + ([] if F is None else [F])
    if seam == "host":
        got, m = phi0.copy(order="F"), mask.copy(order="F")
        args = [a.copy(order="F") for a in ins]
    else:
        got, m = _dev(phi0), _dev(mask)
        args = [_dev(a) for a in ins]
    velocity = tuple(args[:3]) if vel is not None else None
    speed = args[-1] if F is not None else None
    if plain:
        kw.pop("clamp", None)
        call = lambda: lsf.evolveBand(got, m, nx, ny, nz, dx, dt, steps, velocity=velocity, speed=speed, **kw)
    else:
        call = lambda: lsf.evolveBandCurv(got, m, nx, ny, nz, dx, dt, steps, curvature=bcurv, velocity=velocity, speed=speed, **kw)
    try:
        if raises is None:
            rep = call()
        else:
            with pytest.raises(raises) as e:
                call()
            rep = e.value
    finally:
        for a, b in zip(args, ins):
            assert np.array_equal(a if seam == "host" else _host(a, b.shape), b)  # read, never written
    if seam == "device":
        got, m = _host(got, phi0.shape), _host(m, mask.shape)
    return got, m, rep


def _assert_report(rep, want):
    assert rep.steps == want.steps and rep.cfl == want.cfl and rep.diffusion == want.diffusion and rep.change == want.change
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
@pytest.mark.parametrize("case", list(K.CASES))
def test_strict_is_bit_identical_to_the_statement(lsf, case, seam):
    phi0, mask, vel, F, n, dx, dt, bcurv, kw = K.inputs(case)
    want, _ = K.want(case)
    got, m, rep = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, K.CASES[case].steps, bcurv, **kw)
    _assert_equal(case, got, m, rep, want, seam)
    never = ~B.list_of(mask) & ~(want.mask == 1)  # points in neither the first nor the last list keep their bits
    assert never.any() and np.array_equal(got[never].view(np.uint64), phi0[never].view(np.uint64))


# ---------------------------------------------------------------------------------- 2: bcurv = 0 is lsf_evolve_band
@pytest.mark.parametrize("seam", SEAMS)
def test_without_the_term_the_call_is_evolve_band(lsf, seam):
    phi0, mask, vel, F, n, dx, dt, _, kw = K.inputs("curvsmall")
    a, ma, ra = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, 6, 0.0, **dict(kw, clamp=0.37))  # the clamp is ignored
    b, mb, rb = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, 6, None, plain=True, **kw)
    assert rb.rebuilds == 1 and ra.diffusion == 0.0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(ma, mb)
    assert tuple(x for f, x in zip(ra._fields, ra) if f != "diffusion") == tuple(rb)


# ---------------------------------------------------------------------------------- 3: calls compose
@pytest.mark.parametrize("seam", SEAMS)
def test_six_steps_are_three_and_three(lsf, seam):
    phi0, mask, vel, F, n, dx, dt, bcurv, kw = K.inputs("curvsmall")
    want, _ = K.want("curvsmall")
    half, mh, rep1 = _run(lsf, seam, phi0, mask, vel, F, n, dx, dt, 3, bcurv, **kw)
    _assert_equal("curvsmall", half, mh, rep1, K.want("curvsmall", 3)[0], f"{seam}, first half")
    full, mf, rep2 = _run(lsf, seam, half, mh, vel, F, n, dx, dt, 3, bcurv, **kw)
    assert np.array_equal(full, want.field) and np.array_equal(mf, want.mask) and rep1.change + rep2.change == want.change


# ---------------------------------------------------------------------------------- 4: FAST against STRICT
@pytest.mark.parametrize("case", ["dumbbell", "curvonly"])
def test_fast_takes_the_same_schedule_within_tolerance_of_strict(lsf, case):
    phi0, mask, vel, F, n, dx, dt, bcurv, kw = K.inputs(case)
    want, _ = K.want(case)  # (asserts that no margin of the statement lies within 1e-6 dx of core dx)
    got, m, rep = _run(lsf, "device", phi0, mask, vel, F, n, dx, dt, K.CASES[case].steps, bcurv, arith="fast", **kw)
    lst = want.mask == 1
    rms = float(np.sqrt(np.mean((got[lst] - want.field[lst]) ** 2)))
    print(f"{case}: FAST against STRICT over the final list: rms {rms:.3e}, max {np.abs(got - want.field).max():.3e}, rebuilds {rep.rebuilds}")
    assert np.array_equal(m, want.mask) and rep.rebuilds == want.rebuilds and rep.steps == want.steps
    assert rep.cfl == want.cfl and rep.diffusion == want.diffusion
    assert (rep.cells, rep.open_cells, rep.entered, rep.flips) == (want.cells, want.open_cells, want.entered, want.flips)
    assert rms <= FAST_RMS_TOL


# ---------------------------------------------------------------------------------- 5: a NaN
@pytest.mark.parametrize("seam", SEAMS)
def test_a_nan_at_a_list_cell(lsf, seam):
    phi0, mask, vel, F, n, dx, dt, bcurv, kw = K.inputs("curvsmall")
    bad = phi0.copy(order="F")
    bad[tuple(np.argwhere(B.list_of(mask))[300])] = np.nan
    want = VC.evolve_band_curv(bad, mask, vel, F, dx, dt, 3, bcurv, **kw)
    assert want.nan and want.steps == 1 and math.isnan(want.change[0])
    got, m, err = _run(lsf, seam, bad, mask, vel, F, n, dx, dt, 3, bcurv, raises=lsf.LsfNaNError, **kw)
    rep = err.report
    assert rep.steps == 1 and len(rep.change) == 1 and math.isnan(rep.change[0]) and rep.cfl == want.cfl and rep.diffusion == want.diffusion
    assert tuple(rep)[4:] == (None,) * 7  # info and margin are reported on LSF_OK only
    assert np.array_equal(m, want.mask) and set(np.unique(m)) == {0, 1}  # the mask is written, normalised
    assert np.array_equal(got, want.field, equal_nan=True)  # the state after the transport of the NaN step: its sweeps are not run


# ---------------------------------------------------------------------------------- 6: errors
def _raw(lib, seam, phi, mask, u, v, w, f, n, dx, dt, steps, bcurv, clamp):
    from levelsetfortran_amd import _lib

    done, cfl, diff, margin = ctypes.c_int(-7), ctypes.c_double(-7.0), ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    trace = np.full(8, -7.0)
    info = np.full(6, -7, np.int64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), ptr(u), ptr(v), ptr(w), ptr(f), n[0], n[1], n[2], dx, dt, steps, _lib.LSF_ADVECT_RK3,
            _lib.LSF_ORDER_JACOBI | _lib.LSF_ARITH_STRICT, 1.5, 2, 1, 0.5 * dx, 1, bcurv, clamp, ctypes.byref(done), ctypes.byref(cfl),
            ctypes.byref(diff), trace.ctypes.data, 8, info.ctypes.data, ctypes.byref(margin))
    rc = lib.lsf_evolve_band_curv_device(*args, None) if seam == "device" else lib.lsf_evolve_band_curv(*args)
    return rc, done.value, cfl.value, diff.value, trace, list(info), margin.value, (lib.lsf_last_error() or b"").decode()


@pytest.mark.parametrize("seam", SEAMS)
def test_the_new_invalid_arguments_leave_phi_and_mask_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask0, (u0, v0, w0), _, n, dx, dt, bcurv, kw = K.inputs("curvsmall")
    mask0 = mask0.copy(order="F")
    mask0[0], mask0[2, 2, 2] = 1, 7  # not normalised: an invalid call must leave it so
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    phi, mask, u, v, w = (mk(a) for a in (phi0, mask0, u0, v0, w0))
    nan, inf = float("nan"), float("inf")
    ok = dict(phi=phi, mask=mask, u=u, v=v, w=w, f=None, n=n, dx=dx, dt=dt, steps=2, bcurv=bcurv, clamp=1.0)
    cases = {
        "bcurv < 0": dict(bcurv=-bcurv), "bcurv NaN": dict(bcurv=nan), "bcurv inf": dict(bcurv=inf), "bcurv -inf": dict(bcurv=-inf),
        "bcurv = 0 with neither": dict(bcurv=0.0, u=None, v=None, w=None), "clamp < 0": dict(clamp=-1.0), "clamp NaN": dict(clamp=nan),
        "clamp inf": dict(clamp=inf), "bad clamp without the term": dict(bcurv=0.0, clamp=nan),
        "partial velocity": dict(w=None), "NULL mask": dict(mask=None),  # lsf_evolve_band's own, through the new entry
    }
    for name, change in cases.items():
        rc, done, cfl, diff, trace, info, margin, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and done == -7 and cfl == -7.0 and diff == -7.0 and np.all(trace == -7.0) and info == [-7] * 6 and margin == -7.0, name
        back, mback = (_host(phi, phi0.shape), _host(mask, mask0.shape)) if seam == "device" else (phi, mask)
        assert np.array_equal(back, phi0) and np.array_equal(mback, mask0), name
    # a valid call follows: the library is in working order; both input groups absent is legal with bcurv > 0
    rc, done, cfl, diff, trace, info, margin, _ = _raw(lib, seam, **dict(ok, u=None, v=None, w=None))
    want = VC.evolve_band_curv(phi0, mask0, None, None, dx, dt, 2, bcurv, 1.0, "rk3", 1.5, 2, 1, 0.5 * dx, 1)
    assert rc == 0 and done == 2 and cfl == 0.0 and diff == want.diffusion and list(trace[:2]) == want.change and np.all(trace[2:] == -7.0)
    assert info == [want.cells, want.open_cells, want.flips, want.rebuilds, want.entered, want.near_wall] and margin == want.margin
    back, mback = (_host(phi, phi0.shape), _host(mask, mask0.shape)) if seam == "device" else (phi, mask)
    assert np.array_equal(back, want.field) and np.array_equal(mback, want.mask)


# ---------------------------------------------------------------------------------- 7: the host seam under lsf_mirror
def test_the_host_seam_under_trust_and_lazy_equals_the_device_seam(lsf):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask, vel, F, n, dx, dt, bcurv, kw = K.inputs("curvsmall")
    dev, md, rd = _run(lsf, "device", phi0, mask, vel, F, n, dx, dt, 6, bcurv, **kw)
    got, m = phi0.copy(order="F"), mask.copy(order="F")
    ins = tuple(a.copy(order="F") for a in vel)
    try:
        # fresh arrays may sit at the address of an array an earlier host-seam call left a twin for: TRUST would take that twin for theirs
        for a in (got, m, *ins):
            _lib.check(lib.lsf_mirror_forget(a.ctypes.data))
        _lib.check(lib.lsf_mirror(_lib.LSF_MIRROR_TRUST | _lib.LSF_MIRROR_LAZY))
        rep = lsf.evolveBandCurv(got, m, *n, dx, dt, 6, curvature=bcurv, velocity=ins, **kw)
        for a in (got, m):
            _lib.check(lib.lsf_mirror_sync(a.ctypes.data))
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())
    assert all(np.array_equal(a, b) for a, b in zip(ins, vel))
    print(f"host seam, trust | lazy: phi differs at {int((got != dev).sum())}, mask at {int((m != md).sum())}; report {rep}; device seam {rd}")
    assert np.array_equal(got.view(np.uint64), dev.view(np.uint64)) and np.array_equal(m, md) and tuple(rep) == tuple(rd)
