"""lsf_extend_field on the GPU against its serial restatement (tests/extend_ref.py).  Every comparison is np.array_equal (NaN-aware)
on field, rounds, trace and info: the tile-plane order reproduces the raster order, so there is no tolerance anywhere.  The runs
capped at 1 and 2 rounds pin the ordering itself; a fixed point alone would hide a race or a wrong visiting order."""
import ctypes
import os

import numpy as np
import pytest

import distance_fill_ref as D
import extend_ref as E
import stl_io
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


def _n(a):
    return tuple(s - 1 for s in a.shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(rep, got, want):
    field, rounds, trace, info = want
    print("rounds", rep.rounds, "trace", rep.changed, "info", rep[2:5], "| reference", rounds, trace, info)
    assert rep.rounds == rounds and rep.changed == trace and tuple(rep[2:5]) == info
    assert rep.converged == (trace[-1] == 0)
    assert np.array_equal(got, field, equal_nan=True)


def _dev(a, dt=np.float64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt).ravel(order="F"))).to("cuda")


def _home(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


@pytest.mark.parametrize("cap", [1, 2, 64])
@pytest.mark.parametrize("case", E.CASES)
def test_field_rounds_trace_and_info_equal_the_serial_sweeps(lsf, case, cap):
    q0, phi0, dx, band = E.inputs(case)
    nx, ny, nz = _n(phi0)
    frozen = E.frozen_set(phi0, dx, band=band)
    want = E.want(case, cap)
    # the band form
    q, phi = np.array(q0, order="F"), np.array(phi0, order="F")
    rep = lsf.extendField(q, phi, nx, ny, nz, dx, band=band, max_rounds=cap)
    _same(rep, q, want)
    assert np.array_equal(phi, phi0)
    assert np.array_equal(_bits(q[frozen]), _bits(q0[frozen]))  # the caller's bits: a -0.0 stays a -0.0
    assert rep.frozen_points + rep.reached + rep.unreached == q.size
    if cap == 64:
        assert rep.converged and rep.unreached == 0 and np.isfinite(q).all()
    # the mask form of the same frozen set: band is ignored
    q2 = np.array(q0, order="F")
    mask = np.array(frozen, dtype=np.int32, order="F")
    keep = mask.copy(order="F")
    rep2 = lsf.extendField(q2, phi, nx, ny, nz, dx, mask=mask, max_rounds=cap)
    assert rep2 == rep and np.array_equal(q2, q, equal_nan=True)
    assert np.array_equal(mask, keep) and np.array_equal(phi, phi0)


def test_a_plateau_is_left_unreached_and_reported(lsf):
    q0, phi0, dx = E.sphere_case(21, clamp_cells=3)
    want = E.extend(q0, phi0, dx, band=1.5)
    q, phi = np.array(q0, order="F"), np.array(phi0, order="F")
    rep = lsf.extendField(q, phi, 20, 20, 20, dx, band=1.5)
    _same(rep, q, want)
    assert rep.unreached == int(np.isnan(q).sum()) == 6705 and rep.changed == [4021, 0] and rep.converged
    assert np.isfinite(q[~np.isnan(q)]).all()


def test_device_seam_on_a_side_stream_and_run_to_run(lsf):
    import torch

    q0, phi0, dx, band = E.inputs("twospheres")
    nx, ny, nz = _n(phi0)
    frozen = E.frozen_set(phi0, dx, band=band)
    host = np.array(q0, order="F")
    rep_h = lsf.extendField(host, np.array(phi0, order="F"), nx, ny, nz, dx, band=band, max_rounds=2)
    _same(rep_h, host, E.want("twospheres", 2))
    assert not rep_h.converged  # this input needs 4 rounds
    outs = []
    for _ in range(2):
        t, f, m = _dev(q0), _dev(phi0), _dev(frozen, np.int32)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            rep_d = lsf.extendField(t, f, nx, ny, nz, dx, band=band, max_rounds=2)
            t2 = _dev(q0)
            rep_m = lsf.extendField(t2, f, nx, ny, nz, dx, mask=m, max_rounds=2)
            rep_full = lsf.extendField(t2, f, nx, ny, nz, dx, mask=m)
        assert rep_d == rep_h == rep_m and not rep_d.converged
        assert rep_full.converged and rep_full.rounds == 4
        outs.append(_home(t, phi0.shape))
        assert np.array_equal(_home(t2, phi0.shape), E.want("twospheres", 64)[0])
        assert np.array_equal(_home(f, phi0.shape), phi0) and np.array_equal(_home(m, phi0.shape), frozen)
    assert np.array_equal(outs[0], host, equal_nan=True) and np.array_equal(outs[1], host, equal_nan=True)


def test_errors_leave_q_alone_and_a_valid_call_follows(lsf):
    import torch

    from levelsetfortran_amd import _lib

    lib = _lib.load()
    q0, phi0, dx, band = E.inputs("sphere15")
    nx, ny, nz = _n(phi0)
    frozen = E.frozen_set(phi0, dx, band=band)

    def call(t, f, m=None, n=(nx, ny, nz), dx_=dx, band_=band, rounds=64):
        done = ctypes.c_int(-1)
        tr = np.full(64, -1, dtype=np.int64)
        info = np.full(3, -1, dtype=np.int64)
        rc = lib.lsf_extend_field_device(t.data_ptr() if t is not None else None, f.data_ptr() if f is not None else None,
                                         m.data_ptr() if m is not None else None, n[0], n[1], n[2], dx_, band_, rounds, ctypes.byref(done),
                                         tr.ctypes.data, 64, info.ctypes.data, None)
        assert (info == -1).all()  # info is written on LSF_OK only
        return rc, (lib.lsf_last_error() or b"").decode()

    mask = _dev(frozen, np.int32)
    at_fz, at_far = np.argwhere(frozen), np.argwhere(~frozen)
    cases = []
    for bad in (np.nan, np.inf):  # a non-finite q on frozen points; one on a non-frozen point is legal and not counted
        g = np.array(q0)
        g[tuple(at_fz[5])] = bad
        g[tuple(at_fz[len(at_fz) // 2])] = -bad
        g[tuple(at_far[9])] = bad
        cases.append((g, phi0, dict(), "2 frozen point(s) hold a non-finite q"))
        cases.append((g, phi0, dict(m=mask), "2 frozen point(s) hold a non-finite q"))
    p = np.array(phi0)
    p[tuple(at_far[11])] = np.nan
    p[tuple(at_far[40])] = -np.inf
    p[tuple(at_fz[7])] = np.inf
    cases.append((q0, p, dict(), "3 point(s) hold a non-finite phi"))
    cases.append((q0, p, dict(m=mask), "3 point(s) hold a non-finite phi"))
    cases.append((q0, phi0, dict(m=_dev(np.zeros(phi0.shape), np.int32)), "no frozen point"))
    cases.append((q0, np.full(phi0.shape, 7.0), dict(), "no frozen point"))
    cases += [(q0, phi0, dict(band_=0.0), "band"), (q0, phi0, dict(band_=float("nan")), "band"), (q0, phi0, dict(band_=float("inf")), "band"),
              (q0, phi0, dict(dx_=0.0), "dx"), (q0, phi0, dict(dx_=-0.1), "dx"), (q0, phi0, dict(dx_=float("inf")), "dx"),
              (q0, phi0, dict(dx_=float("nan")), "dx"), (q0, phi0, dict(rounds=0), "max_rounds"), (q0, phi0, dict(n=(nx, 0, nz)), "nx, ny, nz"),
              (q0, phi0, dict(n=(2047, 2047, 511)), "2^31 - 1 points")]
    for g, p, kw, text in cases:
        t, f = _dev(g), _dev(p)
        before, before_f = t.clone(), f.clone()
        rc, msg = call(t, f, **kw)
        assert rc == _lib.LSF_ERR_INVALID and text in msg and "lsf_extend_field" in msg, (kw, text, rc, msg)
        assert torch.equal(t.view(torch.int64), before.view(torch.int64)), (kw, text)
        assert torch.equal(f.view(torch.int64), before_f.view(torch.int64)), (kw, text)
    t, f = _dev(q0), _dev(phi0)
    for a, b, text in ((None, f, "q is NULL"), (t, None, "phi is NULL")):
        rc, msg = call(a, b)
        assert rc == _lib.LSF_ERR_INVALID and text in msg
    assert torch.equal(t.view(torch.int64), _dev(q0).view(torch.int64))
    # the host seam refuses the same way and copies nothing back
    g = np.array(q0, order="F")
    g[tuple(at_fz[5])] = np.nan
    keep = g.copy(order="F")
    with pytest.raises(lsf.LsfError) as e:
        lsf.extendField(g, np.array(phi0, order="F"), nx, ny, nz, dx, band=band)
    assert e.value.code == _lib.LSF_ERR_INVALID and "1 frozen point(s) hold a non-finite q" in str(e.value)
    assert np.array_equal(_bits(g), _bits(keep))
    # ... and after all of those a valid call succeeds, with a mask that does not separate the signs (one side of the band only)
    rep = lsf.extendField(t, f, nx, ny, nz, dx, band=band)
    _same(rep, _home(t, phi0.shape), E.want("sphere15", 64))
    one_side = frozen & (phi0 > 0)
    t = _dev(q0)
    rep = lsf.extendField(t, f, nx, ny, nz, dx, mask=_dev(one_side, np.int32))
    _same(rep, _home(t, phi0.shape), E.extend(q0, phi0, dx, mask=one_side.astype(np.int32)))


@pytest.fixture(scope="module")
def cube40_surface():
    s = np.load(os.path.join(GOLDEN, "surfaces.npz"))
    return s["cube40_surfX"].astype(np.float64), s["cube40_surfElem"]


def test_chain_mesh_distance_fill_extend_advect(lsf, oracle, cube40_surface, cube40):
    """A speed known on the tube of the mesh distance only, extended, then used: meshDistance -> distanceFill -> extendField ->
    advectField(speed=...), 2 RK3 steps in STRICT arithmetic, against advect_ref fed with extend_ref's field."""
    import advect_ref as A

    X, S = cube40_surface
    n, xLo, _, _ = stl_io.grid_from_surface(X)
    dx = float(cube40["dx"])
    shape = tuple(v + 1 for v in n)
    assert shape == (62, 62, 62) and dx == 0.05
    phi = np.full(shape, 7.0, order="F")
    lsf.meshDistance(phi, n[0], n[1], n[2], dx, xLo, X, S, width=3.5)
    tube = np.abs(phi) < 3.5 * dx
    assert lsf.distanceFill(phi, n[0], n[1], n[2], dx, band=3.5).converged
    filled = phi.copy(order="F")
    speed0 = np.array(np.where(tube, 0.6 * E.quantity(shape, dx) - 1.0, np.nan), order="F")  # changes sign on the tube
    speed = speed0.copy(order="F")
    mask = np.array(tube, dtype=np.int32, order="F")  # "known on the tube": the filled field need not keep |phi| >= 3.5 dx outside it
    rep = lsf.extendField(speed, phi, n[0], n[1], n[2], dx, mask=mask)
    want = E.extend(speed0, filled, dx, mask=mask)
    _same(rep, speed, want)
    assert rep.frozen_points == 66282 == int(tube.sum()) and rep.converged and rep.unreached == 0
    assert np.array_equal(phi, filled) and (speed[tube] < 0).any() and (speed[tube] > 0).any()
    dt = 0.5 * dx / float(np.abs(want[0]).max())
    arep = lsf.advectField(phi, n[0], n[1], n[2], dx, dt, 2, speed=speed, arith="strict")
    moved, change, cfl = A.advect(filled, None, want[0], dx, dt, 2, "rk3")
    assert arep.steps == 2 and arep.change == change and arep.cfl == cfl
    assert np.array_equal(phi, moved)


def test_host_seam_under_lazy_mirror_takes_phi_from_its_twin_and_brings_q_home(lsf):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    inp, width = D.CASES["sphere15"]
    ref, dx = D.exact(inp)
    clamped = D.clamp(ref, dx, width)
    nx, ny, nz = _n(ref)
    tube = np.abs(clamped) < width * dx
    q0 = np.where(tube, E.quantity(ref.shape, dx), 7.0)
    filled = D.fill(clamped, dx, band=width)[0]
    mask = np.array(tube, dtype=np.int32, order="F")
    want = E.extend(q0, filled, dx, mask=mask)
    assert want[3][2] == 0 and E.extend(q0, clamped, dx, mask=mask)[3][2] > 0  # the host copy of phi would leave a plateau
    try:
        _lib.check(lib.lsf_mirror(_lib.LSF_MIRROR_TRUST | _lib.LSF_MIRROR_LAZY))
        phi = np.array(clamped, order="F")
        q = np.array(q0, order="F")
        assert lsf.distanceFill(phi, nx, ny, nz, dx, band=width).converged
        assert np.array_equal(phi, clamped)  # the filled field is on the device only
        rep = lsf.extendField(q, phi, nx, ny, nz, dx, mask=mask)
        _same(rep, q, want)  # phi came from its current twin; q is home although the mirror is lazy
        assert np.array_equal(phi, clamped)
        _lib.check(lib.lsf_mirror_sync(phi.ctypes.data))
        assert np.array_equal(phi, filled)
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())
