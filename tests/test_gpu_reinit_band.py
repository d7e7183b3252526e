"""lsf_reinit_band on the GPU against the CPU emulator (tests/band_emulator.py: one full-interior Jacobi sweep of the oracle, kept
at the list cells).  STRICT arithmetic, the untouched points and the stop sweep are compared with `==`; the RMS trace within
1e-11 relative (a parallel against a sequential sum); FAST within the project's 1e-12 RMS of STRICT."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, F

pytestmark = pytest.mark.gpu

FAST_RMS_TOL = 1.0e-12  # tests/test_gpu_parity.py
TRACE_RTOL = 1.0e-11

# two_sphere_phi0 on the first four grids ((9,12,10) and (5,5,5) have no WENO cell).  The two ragged grids carry the off-centre
# sphere that tests/test_gpu_parity.py runs on them (..._ragged_sizes): the two spheres lie outside a (70,21,45) grid, whose
# stencil band would then be empty.
SYNTH = [(40, 33, 27), (24, 24, 24), (9, 12, 10), (5, 5, 5), (21, 27, 13), (70, 21, 45)]
RAGGED = [(21, 27, 13), (70, 21, 45)]
CASES = [("cube40", "SBfinal"), ("cube40", "NBfinal")] + [(npts, m) for npts in SYNTH for m in ("stencil", "bernoulli", "ones")]
SEAMS = ["host", "device"]


def _case_id(c):
    return f"{c[0] if isinstance(c[0], str) else 'x'.join(map(str, c[0]))}-{c[1]}"


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(phi0, mask int32, (nx, ny, nz), dx, h, sweeps)"""
    from levelsetfortran_amd import fields

    src, kind = case
    if src == "cube40":
        g = np.load(os.path.join(GOLDEN, "cube40_62.npz"), allow_pickle=False)
        n = (int(g["nx"]), int(g["ny"]), int(g["nz"]))
        return F(g["phi_minmax"]), np.asfortranarray(g[kind].astype(np.int32)), n, float(g["dx"]), float(g["h"]), 40
    if src in RAGGED:
        phi0, dx = fields.sphere_phi0(src, radius=0.7, centers=((0.1, -0.2, 0.05),))
    else:
        phi0, dx = fields.two_sphere_phi0(src)
    n = tuple(v - 1 for v in src)
    if kind == "stencil":
        mask = (np.abs(phi0) < 8.1 * dx).astype(np.int32)
    elif kind == "bernoulli":
        mask = (np.random.default_rng(20240 + sum(src)).random(phi0.shape) < 0.3).astype(np.int32)
    else:
        mask = np.ones(phi0.shape, dtype=np.int32)  # walls included: they are ignored
    return phi0, np.asfortranarray(mask), n, dx, fields.reinit_step(dx), 20


@functools.lru_cache(maxsize=None)
def _emulated(case, tol=0.0):
    import band_emulator as be

    phi0, mask, (nx, ny, nz), dx, h, sweeps = _inputs(case)
    field, n, trace, nan = be.reinit_band(phi0, mask, nx, ny, nz, sweeps - 1, dx, h, tol=tol)
    assert not nan
    return field, n, trace


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a.ravel(order="F"))).cuda()


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _run(lsf, seam, phi0, mask, n, iters, dx, h, **kw):
    """reinitBand on a fresh copy through one seam; returns (field, report)."""
    nx, ny, nz = n
    if seam == "host":
        got = phi0.copy(order="F")
        rep = lsf.reinitBand(got, mask.copy(order="F"), nx, ny, nz, iters, dx, h, **kw)
        return got, rep
    t, m = _dev(phi0), _dev(mask)
    if kw.get("phiS") is not None:
        kw = dict(kw, phiS=_dev(kw["phiS"]))
    rep = lsf.reinitBand(t, m, nx, ny, nz, iters, dx, h, **kw)
    assert np.array_equal(_host(m, mask.shape), mask)  # the mask is an input
    return _host(t, phi0.shape), rep


# ---------------------------------------------------------------------------------- 1, 2: STRICT == emulator; untouched points
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_strict_is_bit_identical_to_the_emulator(lsf, oracle, case, seam):
    import band_emulator as be

    phi0, mask, n, dx, h, sweeps = _inputs(case)
    want, n_want, tr_want = _emulated(case)
    got, rep = _run(lsf, seam, phi0, mask, n, sweeps - 1, dx, h, tol=0.0, arith="strict")
    M = be.list_mask(mask, *n)
    if case == ("cube40", "SBfinal"):
        assert int(M.sum()) == 161222 and M.size == 238328
    print(f"{_case_id(case)} {seam}: list {int(M.sum())} of {M.size}, max |got - want| = {np.abs(got - want).max():.3e}, "
          f"trace rel {np.max(np.abs(np.array(rep.rms) / np.array(tr_want) - 1)) if rep.count == n_want else float('nan'):.3e}")
    assert rep.count == n_want == sweeps and not rep.converged
    assert np.array_equal(got, want)
    assert np.array_equal(got[~M], phi0[~M])  # never written, walls included
    assert np.allclose(rep.rms, tr_want, rtol=TRACE_RTOL, atol=0)
    if case == ((24, 24, 24), "stencil"):
        # 8 sweeps: the last one is where the host would look at the stop flag (every 8 sweeps) and does not; 9: one past that look
        for iters in (7, 8):
            want, n_want, tr_want, _ = be.reinit_band(phi0, mask, *n, iters, dx, h, tol=0.0)
            got, rep = _run(lsf, seam, phi0, mask, n, iters, dx, h, tol=0.0, arith="strict")
            assert rep.count == n_want == iters + 1 and not rep.converged
            assert np.array_equal(got, want)
            assert np.allclose(rep.rms, tr_want, rtol=TRACE_RTOL, atol=0)


@pytest.mark.parametrize("seam", SEAMS)
def test_points_outside_the_list_are_untouched_and_only_one_is_in(lsf, oracle, seam):
    """mask values 0, 2 and -1 are all 'out'; a 1 on a wall point is ignored"""
    import band_emulator as be

    phi0, _, n, dx, h, _ = _inputs(((40, 33, 27), "stencil"))
    rng = np.random.default_rng(7)
    mask = np.asfortranarray(rng.choice(np.array([0, 1, 2, -1], dtype=np.int32), size=phi0.shape))
    mask[0, :, :] = 1
    mask[:, -1, :] = 1
    M = be.list_mask(mask, *n)
    want, n_want, _, _ = be.reinit_band(phi0, mask, *n, 5, dx, h, tol=0.0)
    for arith in ("strict", "fast"):
        got, rep = _run(lsf, seam, phi0, mask, n, 5, dx, h, tol=0.0, arith=arith)
        assert rep.count == n_want == 6
        assert np.array_equal(got[~M], phi0[~M])
        assert not np.array_equal(got[M], phi0[M])
        if arith == "strict":
            assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------- 3: stop verdict
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_stop_verdict(lsf, oracle, case, seam):
    """tol = geometric mean of the emulator's RMS values s and s + 1: the call stops at the same sweep as the emulator, after s + 2
    sweeps.  The host looks at the stop flag every 8 sweeps: s = 5, 6, 7 stop one sweep before a look, on it and one past it; s = 10
    past the first look, not on one."""
    phi0, mask, n, dx, h, sweeps = _inputs(case)
    _, _, tr = _emulated(case)
    for s in (5, 6, 7, 10):
        lo, hi = sorted((tr[s], tr[s + 1]))
        assert (hi - lo) / hi >= 7.6e-4  # far above the summation allowance
        tol = float(np.sqrt(lo * hi))
        want, n_want, tr_want = _emulated(case, tol)
        assert n_want < sweeps and tr_want[-1] < tol
        got, rep = _run(lsf, seam, phi0, mask, n, sweeps - 1, dx, h, tol=tol, arith="strict")
        print(f"{_case_id(case)} {seam}: stop after {rep.count} sweeps (emulator {n_want}), tol {tol:.6e}")
        # (the RMS falls from s to s + 1 everywhere but on (70,21,45)-stencil at s = 10, where it rises and entry s is the one below tol)
        falling = tr[s + 1] < tr[s]
        assert falling or s == 10
        assert rep.count == n_want == (s + 2 if falling else s + 1) and rep.converged
        assert np.array_equal(got, want)
        assert np.allclose(rep.rms, tr_want, rtol=TRACE_RTOL, atol=0)


# ---------------------------------------------------------------------------------- 4: continuation
@pytest.mark.parametrize("case", [("cube40", "SBfinal"), ((40, 33, 27), "stencil"), ((9, 12, 10), "bernoulli")], ids=_case_id)
def test_continuation_with_the_original_sign_field(lsf, case):
    phi0, mask, (nx, ny, nz), dx, h, _ = _inputs(case)
    whole, m = _dev(phi0), _dev(mask)
    r = lsf.reinitBand(whole, m, nx, ny, nz, 19, dx, h, tol=0.0, arith="strict")
    parts, orig = _dev(phi0), _dev(phi0)
    r1 = lsf.reinitBand(parts, m, nx, ny, nz, 9, dx, h, tol=0.0, arith="strict")
    r2 = lsf.reinitBand(parts, m, nx, ny, nz, 9, dx, h, tol=0.0, arith="strict", phiS=orig)
    assert (r.count, r1.count, r2.count) == (20, 10, 10)
    assert bool((parts == whole).all())
    assert r1.rms + r2.rms == r.rms  # the same sums in the same order
    assert np.array_equal(_host(orig, phi0.shape), phi0)


# ---------------------------------------------------------------------------------- 5: FAST
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fast_within_tolerance_of_strict(lsf, oracle, case, seam):
    import band_emulator as be

    phi0, mask, n, dx, h, _ = _inputs(case)
    M = be.list_mask(mask, *n)
    strict, rs = _run(lsf, seam, phi0, mask, n, 15, dx, h, tol=0.0, arith="strict")
    fast, rf = _run(lsf, seam, phi0, mask, n, 15, dx, h, tol=0.0, arith="fast")
    rms = float(np.sqrt(np.mean((fast[M] - strict[M]) ** 2)))
    print(f"{_case_id(case)} {seam}: FAST against STRICT over the list after 16 sweeps: rms {rms:.3e}, max {np.abs(fast - strict).max():.3e}")
    assert rs.count == rf.count == 16
    assert rms < FAST_RMS_TOL
    assert np.array_equal(np.signbit(fast), np.signbit(strict))
    assert np.array_equal(fast[~M], phi0[~M])


# ---------------------------------------------------------------------------------- 6: errors
def test_gs_ordering_is_invalid(lsf):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask, (nx, ny, nz), dx, h, _ = _inputs(((24, 24, 24), "stencil"))
    done = ctypes.c_int(-1)
    for arith in (_lib.LSF_ARITH_FAST, _lib.LSF_ARITH_STRICT):
        got = phi0.copy(order="F")
        rc = lib.lsf_reinit_band(got.ctypes.data, mask.ctypes.data, nx, ny, nz, 3, dx, h, 0.0, _lib.LSF_ORDER_GS | arith,
                                 ctypes.byref(done), None, 0)
        assert rc == _lib.LSF_ERR_INVALID and b"raster" in lib.lsf_last_error()
        assert np.array_equal(got, phi0)
        t, m = _dev(phi0), _dev(mask)
        rc = lib.lsf_reinit_band_device(t.data_ptr(), None, m.data_ptr(), nx, ny, nz, 3, dx, h, 0.0, _lib.LSF_ORDER_GS | arith,
                                        ctypes.byref(done), None, 0, None)
        assert rc == _lib.LSF_ERR_INVALID
        assert np.array_equal(_host(t, phi0.shape), phi0)
    # the other invalid arguments
    got = phi0.copy(order="F")
    jac = _lib.LSF_ORDER_JACOBI
    assert lib.lsf_reinit_band(got.ctypes.data, None, nx, ny, nz, 3, dx, h, 0.0, jac, None, None, 0) == _lib.LSF_ERR_INVALID
    assert lib.lsf_reinit_band(got.ctypes.data, mask.ctypes.data, nx, ny, nz, -1, dx, h, 0.0, jac, None, None, 0) == _lib.LSF_ERR_INVALID
    assert lib.lsf_reinit_band(got.ctypes.data, mask.ctypes.data, 1, ny, nz, 3, dx, h, 0.0, jac, None, None, 0) == _lib.LSF_ERR_INVALID
    # more than 2^31 - 1 points: refused before anything is touched (the pointers are never followed)
    assert lib.lsf_reinit_band_device(t.data_ptr(), None, m.data_ptr(), 1300, 1300, 1300, 3, dx, h, 0.0, jac, None, None, 0,
                                      None) == _lib.LSF_ERR_INVALID
    assert b"2^31" in lib.lsf_last_error()
    assert np.array_equal(got, phi0)


@pytest.mark.parametrize("seam", SEAMS)
def test_nan_in_one_list_cell_stops_after_the_first_sweep(lsf, seam):
    phi0, mask, n, dx, h, _ = _inputs(((24, 24, 24), "stencil"))
    bad = phi0.copy(order="F")
    assert mask[12, 12, 12] == 1
    bad[12, 12, 12] = np.nan
    with pytest.raises(lsf.LsfNaNError):
        _run(lsf, seam, bad, mask, n, 9, dx, h, tol=0.0, arith="strict")
    # the report of the failing call: one sweep, a NaN residual, the field after that sweep
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    got = bad.copy(order="F")
    done, tr = ctypes.c_int(-1), np.zeros(10)
    rc = lib.lsf_reinit_band(got.ctypes.data, mask.ctypes.data, *n, 9, dx, h, 0.0, _lib.LSF_ORDER_JACOBI | _lib.LSF_ARITH_STRICT,
                             ctypes.byref(done), tr.ctypes.data, 10)
    assert rc == _lib.LSF_ERR_NAN and done.value == 1 and np.isnan(tr[0])
    import band_emulator as be

    want, n_want, _, nan = be.reinit_band(bad, mask, *n, 9, dx, h, tol=0.0)
    assert nan and n_want == 1
    M = be.list_mask(mask, *n)
    assert np.isnan(got[12, 12, 12]) and np.array_equal(got[~M], bad[~M])
    far = np.ones(bad.shape, dtype=bool)
    far[9:16, 9:16, 9:16] = False  # cells whose stencil cannot reach the NaN
    assert np.array_equal(got[far], want[far])


@pytest.mark.parametrize("seam", SEAMS)
def test_empty_list(lsf, seam):
    phi0, _, n, dx, h, _ = _inputs(((24, 24, 24), "stencil"))
    mask = np.zeros(phi0.shape, dtype=np.int32, order="F")
    mask[0, :, :] = 1  # wall points only
    mask[3, 3, 3] = 2
    got, rep = _run(lsf, seam, phi0, mask, n, 9, dx, h, tol=0.0)
    assert rep.count == 0 and rep.rms == [] and not rep.converged
    assert np.array_equal(got, phi0)


# ---------------------------------------------------------------------------------- 7: mirror
def test_host_seam_with_device_twins(lsf):
    """narrowBand -> reinitBand with phiSB as the mask -> lsf_mirror_sync under TRUST | LAZY equals the plain path"""
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, _, (nx, ny, nz), dx, h, _ = _inputs(("cube40", "SBfinal"))

    def chain(which):
        phi = phi0.copy(order="F")
        nb = np.zeros(phi.shape, dtype=np.int32, order="F")
        sb = np.zeros(phi.shape, dtype=np.int32, order="F")
        lsf.narrowBand(nx, ny, nz, dx, phi, nb, sb)
        rep = lsf.reinitBand(phi, sb if which == "sb" else nb, nx, ny, nz, 11, dx, h, tol=0.0, arith="strict")
        return phi, nb, sb, rep

    for which in ("sb", "nb"):
        plain, nb0, sb0, rep0 = chain(which)
        assert rep0.count == 12 and not np.array_equal(plain, phi0)
        try:
            _lib.check(lib.lsf_mirror(_lib.LSF_MIRROR_TRUST | _lib.LSF_MIRROR_LAZY))
            phi, nb, sb, rep = chain(which)
            assert np.array_equal(phi, phi0) and not nb.any() and not sb.any()  # the results are on the device only
            for a in (phi, nb, sb):
                _lib.check(lib.lsf_mirror_sync(a.ctypes.data))
            assert rep.count == rep0.count and rep.rms == rep0.rms
            assert np.array_equal(phi, plain) and np.array_equal(nb, nb0) and np.array_equal(sb, sb0)
        finally:
            _lib.check(lib.lsf_mirror(0))
            _lib.check(lib.lsf_release_workspace())


# ---------------------------------------------------------------------------------- 8: bench size
@pytest.mark.parametrize("field", ["smeared_sign", "distance"])
def test_bench_size_against_the_full_grid_sweep(lsf, field):
    """512^3, phiSB of narrowBand as the mask, 8 sweeps: the product's own full-grid Jacobi sweep (lsf_jacobi_sweep_box, pinned to the
    oracle by tests/test_gpu_parity.py) followed by a masked select, sweep by sweep.  smeared_sign: fields.two_sphere_phi0_device as
    it is (phi = d / sqrt(d^2 + dx^2): |phi| < 8.1 dx is a fraction of a cell wide, a list of some ten thousand cells); distance: the
    signed distance d recovered from it, whose stencil band is 8 cells wide on either side of the surface (about 2 % of the grid)."""
    import torch

    from levelsetfortran_amd import distributed as D
    from levelsetfortran_amd import fields

    N = 512
    nx = ny = nz = N - 1
    dev = torch.device("cuda", 0)
    phi0, dx = fields.two_sphere_phi0_device((N, N, N), dev)
    h = fields.reinit_step(dx)
    if field == "distance":
        phi0 = dx * phi0 / torch.sqrt(1.0 - phi0 * phi0)
        assert bool(torch.isfinite(phi0).all())
    nb = torch.zeros(phi0.numel(), dtype=torch.int32, device=dev)
    sb = torch.zeros(phi0.numel(), dtype=torch.int32, device=dev)
    lsf.narrowBand(nx, ny, nz, dx, phi0, nb, sb)
    del nb
    inner = torch.zeros((N, N, N), dtype=torch.bool, device=dev)
    inner[1:nz, 1:ny, 1:nx] = True
    M = (sb == 1) & inner.reshape(-1)
    del inner
    nL = int(M.sum())
    print(f"512^3 {field}: list {nL} cells = {100.0 * nL / M.numel():.2f} % of the grid")
    assert 0 < nL < 0.10 * M.numel()  # the case the feature exists for
    b = D.make_block(0, (1, 1, 1), (nx, ny, nz))
    cells = [tuple(c) for c in D.interior_cells_local(b)]
    results = {}
    for arith in ("strict", "fast"):
        be = D.HipBackend(dev, arith=arith)
        cur, swept, sumsq = phi0.clone(), phi0.clone(), be.zeros(1)
        want_rms = []
        for _ in range(8):
            be.sweep(cur, swept, phi0, b, cells, dx, h, sumsq, be.compute)
            new = torch.where(M, swept, cur)
            want_rms.append(float(torch.sqrt(((new - cur)[M] ** 2).sum() / nL)))
            cur = new
        del swept, new
        got = phi0.clone()
        rep = lsf.reinitBand(got, sb, nx, ny, nz, 7, dx, h, tol=0.0, arith=arith)
        assert rep.count == 8
        same = bool((got == cur).all())
        rms = float(torch.sqrt((((got - cur)[M]) ** 2).mean()))
        print(f"512^3 {field} {arith}: bit-identical to the full-grid sweep + select: {same}; rms over the list {rms:.3e}")
        assert bool((got[~M] == phi0[~M]).all())
        assert np.allclose(rep.rms, want_rms, rtol=TRACE_RTOL, atol=0)
        if arith == "strict":
            assert same
        else:
            assert rms < FAST_RMS_TOL
            assert bool((torch.signbit(got) == torch.signbit(cur)).all())
        results[arith] = got
        del got, cur
    lsf._lib.check(lsf._lib.load().lsf_release_workspace())
