"""lsf_distance_fill on the GPU against its serial restatement (tests/distance_fill_ref.py).  Every comparison is np.array_equal on
field, rounds and trace: the tile-plane order reproduces the raster order, so there is no tolerance anywhere.  The runs capped at 1
and 2 rounds pin the ordering itself; a fixed point alone would hide a race or a wrong visiting order."""
import functools
import os

import numpy as np
import pytest

import distance_fill_ref as R
import stl_io
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _input(case):
    inp, width = R.CASES[case]
    ref, dx = R.exact(inp)
    f = R.clamp(ref, dx, width)
    f.setflags(write=False)
    return f, dx, width


@functools.lru_cache(maxsize=None)
def _want(case, cap):
    f, dx, width = _input(case)
    return R.fill(f, dx, band=width, max_rounds=cap)


def _n(a):
    return tuple(s - 1 for s in a.shape)


def _same(rep, got, want):
    field, rounds, trace, nfz = want
    print("rounds", rep.rounds, "trace", rep.changed, "frozen", rep.frozen_points, "| reference", rounds, trace, nfz)
    assert rep.rounds == rounds and rep.changed == trace and rep.frozen_points == nfz
    assert rep.converged == (trace[-1] == 0)
    assert np.array_equal(got, field)


@pytest.mark.parametrize("cap", [1, 2, 64])
@pytest.mark.parametrize("case", list(R.CASES))
def test_field_rounds_and_trace_equal_the_serial_sweeps(lsf, case, cap):
    f, dx, width = _input(case)
    nx, ny, nz = _n(f)
    phi = np.array(f, order="F")
    rep = lsf.distanceFill(phi, nx, ny, nz, dx, band=width, max_rounds=cap)
    _same(rep, phi, _want(case, cap))
    assert np.isfinite(phi).all()
    if cap == 64:
        assert rep.converged and rep.rounds == {"box35": 3, "box15": 3, "sphere35": 2, "sphere15": 2, "twospheres": 4}.get(case, rep.rounds)


@pytest.fixture(scope="module")
def cube40_surface():
    s = np.load(os.path.join(GOLDEN, "surfaces.npz"))
    return s["cube40_surfX"].astype(np.float64), s["cube40_surfElem"]


def test_chain_from_the_mesh_distance(lsf, cube40_surface, cube40):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    X, E = cube40_surface
    n, xLo, _, _ = stl_io.grid_from_surface(X)
    dx, h = float(cube40["dx"]), float(cube40["h"])
    shape = tuple(v + 1 for v in n)
    assert shape == (62, 62, 62) and dx == 0.05

    def chain():
        phi = np.full(shape, 7.0, order="F")
        nb = np.zeros(shape, dtype=np.int32, order="F")
        sb = np.zeros(shape, dtype=np.int32, order="F")
        lsf.meshDistance(phi, n[0], n[1], n[2], dx, xLo, X, E, width=3.5)
        rep = lsf.distanceFill(phi, n[0], n[1], n[2], dx, band=3.5)
        lsf.narrowBand(n[0], n[1], n[2], dx, phi, nb, sb)
        return phi, nb, sb, rep

    clamped = np.full(shape, 7.0, order="F")
    lsf.meshDistance(clamped, n[0], n[1], n[2], dx, xLo, X, E, width=3.5)
    tube = np.abs(clamped) < 3.5 * dx
    filled, nb0, sb0, rep = chain()
    _same(rep, filled, R.fill(clamped, dx, band=3.5))
    assert rep.frozen_points == 66282 == int(tube.sum()) and rep.converged
    assert np.array_equal(filled[tube], clamped[tube])  # the tube's bits
    assert nb0.sum() > 0 and sb0.sum() > nb0.sum()
    try:
        _lib.check(lib.lsf_mirror(_lib.LSF_MIRROR_TRUST | _lib.LSF_MIRROR_LAZY))
        phi, nb, sb, rep2 = chain()
        assert not nb.any() and not sb.any() and np.all(phi == 7.0)  # the results are on the device only
        for a in (phi, nb, sb):
            _lib.check(lib.lsf_mirror_sync(a.ctypes.data))
        assert rep2 == rep and np.array_equal(phi, filled) and np.array_equal(nb, nb0) and np.array_equal(sb, sb0)
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())
    # reinit afterwards is optional and shorter (CPU oracle: 367 sweeps from the filled field, 565 from the clamped one)
    a, b = np.array(filled, order="F"), np.array(clamped, order="F")
    rep_f = lsf.reinit(a, None, None, n[0], n[1], n[2], 10000, dx, h, order="gs", arith="strict")
    rep_c = lsf.reinit(b, None, None, n[0], n[1], n[2], 10000, dx, h, order="gs", arith="strict")
    print("reinit sweeps from the filled field:", rep_f.count, "from the clamped field:", rep_c.count)
    assert rep_f.converged and rep_c.converged and rep_f.count <= rep_c.count


def test_mask_form_equals_the_band_form(lsf):
    f, dx, width = _input("twospheres")
    nx, ny, nz = _n(f)
    mask = np.array(np.abs(f) < width * dx, dtype=np.int32, order="F")
    keep = mask.copy(order="F")
    phi = np.array(np.where(mask == 1, f, np.where(f < 0, -7.0, 7.0)), order="F")
    rep = lsf.distanceFill(phi, nx, ny, nz, dx, mask=mask)
    _same(rep, phi, _want("twospheres", 64))
    assert np.array_equal(mask, keep)


def test_device_seam_on_a_side_stream_and_run_to_run(lsf):
    import torch

    f, dx, width = _input("long")
    nx, ny, nz = _n(f)
    host = np.array(f, order="F")
    rep_h = lsf.distanceFill(host, nx, ny, nz, dx, band=width)
    _same(rep_h, host, _want("long", 64))
    outs = []
    for _ in range(2):
        t = torch.from_numpy(np.ascontiguousarray(f.ravel(order="F"))).to("cuda")
        m = torch.from_numpy(np.ascontiguousarray((np.abs(f) < width * dx).astype(np.int32).ravel(order="F"))).to("cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            rep_d = lsf.distanceFill(t, nx, ny, nz, dx, band=width, max_rounds=2)
            rep_m = lsf.distanceFill(t.clone(), nx, ny, nz, dx, mask=m, max_rounds=2)
        assert rep_d == rep_h == rep_m
        outs.append(t.cpu().numpy().reshape(f.shape, order="F"))
        assert bool((m.cpu().numpy().reshape(f.shape, order="F") == (np.abs(f) < width * dx)).all())
    assert np.array_equal(outs[0], host) and np.array_equal(outs[1], host)


def test_errors_leave_the_field_alone_and_a_valid_call_follows(lsf):
    import ctypes

    import torch

    from levelsetfortran_amd import _lib

    lib = _lib.load()
    f, dx, width = _input("sphere15")
    nx, ny, nz = _n(f)
    frozen = np.abs(f) < width * dx
    far = np.where(f < 0, -7.0, 7.0)

    def dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt).ravel(order="F"))).to("cuda")

    def call(t, m=None, n=(nx, ny, nz), dx_=dx, band=width, rounds=64):
        done, nfz = ctypes.c_int(-1), ctypes.c_int64(-1)
        tr = np.full(64, -1, dtype=np.int64)
        rc = lib.lsf_distance_fill_device(t.data_ptr(), m.data_ptr() if m is not None else None, n[0], n[1], n[2], dx_, band, rounds,
                                          ctypes.byref(done), tr.ctypes.data, 64, ctypes.byref(nfz), None)
        return rc, (lib.lsf_last_error() or b"").decode()

    mask = dev(frozen, np.int32)
    i_fz = tuple(np.argwhere(frozen)[len(np.argwhere(frozen)) // 2])
    i_far = tuple(np.argwhere(~frozen & (f > 0))[7])
    cases = []
    for bad in (np.nan, np.inf):  # a non-finite value on a frozen point (the mask says so; |phi| < far never would)
        g = np.where(frozen, f, far)
        g[i_fz] = bad
        cases.append((g, dict(m=mask), "1 frozen point(s) hold a non-finite"))
    cases.append((f, dict(m=dev(np.zeros(f.shape), np.int32)), "no frozen point"))
    cases.append((np.full(f.shape, 7.0), dict(), "no frozen point"))
    g = np.array(f)
    g[i_far] = -g[i_far]  # a sign jump between non-frozen neighbours
    jumps = R.check(g, R.frozen_set(g, dx, band=width))[2]
    assert jumps >= 3
    cases.append((g, dict(), "%d pair(s) of axis neighbours" % jumps))
    cases += [(f, dict(band=0.0), "band"), (f, dict(band=float("nan")), "band"), (f, dict(dx_=0.0), "dx"), (f, dict(dx_=-0.1), "dx"),
              (f, dict(dx_=float("inf")), "dx"), (f, dict(rounds=0), "max_rounds"), (f, dict(n=(nx, 0, nz)), "nx, ny, nz")]
    for g, kw, text in cases:
        t = dev(g, np.float64)
        before = t.clone()
        rc, msg = call(t, **kw)
        assert rc == _lib.LSF_ERR_INVALID and text in msg, (kw, text, rc, msg)
        assert torch.equal(t.view(torch.int64), before.view(torch.int64)), (kw, text)
    done = ctypes.c_int(0)
    assert lib.lsf_distance_fill_device(None, None, nx, ny, nz, dx, width, 64, ctypes.byref(done), None, 0, None, None) == _lib.LSF_ERR_INVALID
    # ... and after all of those a valid call succeeds
    t = dev(f, np.float64)
    rep = lsf.distanceFill(t, nx, ny, nz, dx, band=width)
    _same(rep, t.cpu().numpy().reshape(f.shape, order="F"), _want("sphere15", 64))
