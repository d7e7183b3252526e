"""lsf_reseed_points / lsf_reseed_get on the GPU against tests/reseed_ref.py, the numpy statement of the contract in include/lsf.h, on
both seams: pts_out, rad_out, src, status, nout and info are compared with `==` on the bit patterns.

Grid, field, mask and old markers: tests/reseed_inputs.py (20 x 18 x 16 cells, dx = 0.125; a sphere of radius 0.55 off the middle; the
mask |phi| < 4.1 dx with holes 0, 7 and -1; old markers seeded by the statement's rule from the sphere shifted by 0.8 dx, with rad 0, NaN
and +-inf, the special points of tests/sample_ref.py, a FAR marker and an over-full cell planted among them).  The conditions on the
inputs are asserted on the statement first."""
import ctypes

import numpy as np
import pytest

import reseed_inputs as I
import reseed_ref as R

pytestmark = pytest.mark.gpu

N = tuple(s - 1 for s in I.SHAPE)
SENT = -7
SEED = 5


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


def _lib():
    from levelsetfortran_amd import _lib

    return _lib.load()


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _bits(a, b):
    """bit for bit where neither is NaN, NaN exactly where the other is"""
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    if a.shape != b.shape:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def _raw(seam, phi, mask, pts, rad, npts, status, order=R.CUBIC, seed=SEED, want_nout=True, want_info=True, stream=None, n=N, dx=I.DX, lo=I.LO,
         **kw):
    """the C call; the arrays are numpy (host seam), torch (device seam) or None: (rc, nout, info, message)"""
    lib = _lib()
    k = dict(I.MAIN, **kw)
    inf = np.full(R.INFO_LEN, SENT, np.int64)
    nout = ctypes.c_int(SENT)
    lo = None if lo is None else np.array(lo, dtype=np.float64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), n[0], n[1], n[2], dx, None if lo is None else lo.ctypes.data, ptr(pts), ptr(rad), npts, k["per_cell"], k["rmin"],
            k["rmax"], k["band"], order, k["iters"], k["tol"], ctypes.c_uint64(seed), ptr(status), ctypes.byref(nout) if want_nout else None,
            inf.ctypes.data if want_info else None)
    rc = lib.lsf_reseed_points_device(*args, stream) if seam == "device" else lib.lsf_reseed_points(*args)
    return rc, nout.value, [int(v) for v in inf], (lib.lsf_last_error() or b"").decode()


def _get(seam, nout, with_src=True, stream=None):
    """(rc, pts (nout, 3) F, rad, src or None)"""
    import torch

    lib = _lib()
    if seam == "device":
        x = torch.full((3 * nout + 1,), float(SENT), dtype=torch.float64, device="cuda")  # (one entry beyond: it must stay)
        r = torch.full((nout + 1,), float(SENT), dtype=torch.float64, device="cuda")
        s = torch.full((nout + 1,), SENT, dtype=torch.int32, device="cuda") if with_src else None
        rc = lib.lsf_reseed_get_device(x.data_ptr(), r.data_ptr(), None if s is None else s.data_ptr(), stream)
        x, r, s = x.cpu().numpy(), r.cpu().numpy(), None if s is None else s.cpu().numpy()
    else:
        x, r = np.full(3 * nout + 1, float(SENT)), np.full(nout + 1, float(SENT))
        s = np.full(nout + 1, SENT, np.int32) if with_src else None
        rc = lib.lsf_reseed_get(x.ctypes.data, r.ctypes.data, None if s is None else s.ctypes.data)
    if rc == 0:
        assert x[-1] == SENT and r[-1] == SENT and (s is None or s[-1] == SENT)  # nothing beyond nout is written
    return rc, x[:-1].reshape((nout, 3), order="F"), r[:-1], None if s is None else s[:-1]


def _run(seam, order, masked, npts, kind="sphere", with_status=True, want_info=True, with_src=True, stream=None, perm=None, **kw):
    """one call and its get through one seam on fresh copies: (pts, rad, src, status, nout, info); asserts LSF_OK and that the inputs
    are unchanged"""
    import torch
    from levelsetfortran_amd import _lib as L

    phi, mask = I.fields(kind)
    pts, rad = I.markers(npts)
    if perm is not None:
        pts, rad = np.asfortranarray(pts[perm]), rad[perm]
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    p, m = mk(phi), mk(mask) if masked else None
    x, r = (mk(pts), mk(rad)) if npts else (None, None)
    status = mk(np.full(npts, SENT, np.int32)) if with_status and npts else None
    if seam == "device":
        L.check(L.load().lsf_set_device(0))
        torch.cuda.synchronize()
    cs = None if stream is None else stream.cuda_stream
    rc, nout, info, msg = _raw(seam, p, m, x, r, npts, status, order=order, want_info=want_info, stream=cs, **kw)
    assert rc == 0, msg
    rc, po, ro, so = _get(seam, nout, with_src, cs)
    assert rc == 0
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert _bits(back(p), phi.ravel(order="F")) and (m is None or np.array_equal(back(m), mask.ravel(order="F")))  # inputs only
    if npts:
        assert _bits(back(x), pts.ravel(order="F")) and _bits(back(r), rad)
    return po, ro, so, None if status is None else back(status), nout, info


def _assert_equal(got, want, what):
    po, ro, so, status, nout, info = got
    print(f"{what}: nout {nout} want {len(want.rad)}, info {info} want {want.info}")
    assert nout == len(want.rad) == want.info[0] + want.info[8], what
    if info[0] != SENT:
        assert info == want.info, what
    assert _bits(po, want.pts) and np.array_equal(np.signbit(po), np.signbit(want.pts)), what
    assert _bits(ro, want.rad), what
    if so is not None:
        assert np.array_equal(so, want.src), what
    if status is not None:
        assert np.array_equal(status, want.status), what


def test_the_inputs_are_what_the_docstring_says():
    phi, mask = I.fields()
    pts, rad = I.old_markers()
    assert len(rad) >= max(I.NPTS) and sorted(set(mask.ravel())) == [-1, 0, 1, 7]
    for order in (R.LINEAR, R.CUBIC):
        for masked in (False, True):
            for npts in I.NPTS:
                w = I.want(order, masked, npts)
                assert w.info[8] >= 0.85 * w.info[7] > 0, (order, masked, npts, w.info)  # at least 85 % of the candidates are accepted
                assert sum(w.info[:6]) == npts and w.info[8] + w.info[9] + w.info[10] == w.info[7]
                if npts >= 63:  # (a single marker is kept or not: no share between 5 % and 50 % exists)
                    assert 0.05 * npts <= npts - w.info[0] <= 0.5 * npts, (order, masked, npts, w.info)
                    assert w.info[4] >= 3 and w.info[5] >= 1 and w.info[11] == 1 and w.info[12] > I.MAIN["per_cell"]
            w = I.want(order, masked, max(I.NPTS))
            assert w.info[1] >= 18 and (w.info[2] > 0) == masked  # the special points; markers off the band under the mask only
            assert I.want(order, masked, max(I.NPTS), kind="nan").info[3] > 0  # NONFINITE
            assert I.want(order, masked, 0, iters=1).info[9] > 0.3 * w.info[7]  # many NOT_CONVERGED
            assert I.want(order, masked, 0, kind="flat").info[9] > I.want(order, masked, 0).info[9]  # FLAT
        w = I.want(order, True, max(I.NPTS), band=3.0)
        assert w.info[9] > (0.3 if order == R.CUBIC else 0.02) * w.info[7], w.info  # OFFBAND at the first sample and on the way


# ---------------------------------------------------------------------------------- 1: order x mask x seam x npts
@pytest.mark.parametrize("seam", ["host", "device"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("order", [R.LINEAR, R.CUBIC], ids=["linear", "cubic"])
def test_every_output_equals_the_statement(lsf, order, masked, seam):
    import torch

    for npts in I.NPTS:
        _assert_equal(_run(seam, order, masked, npts), I.want(order, masked, npts), f"{seam} npts {npts}")
    if seam == "device":
        _assert_equal(_run(seam, order, masked, max(I.NPTS), stream=torch.cuda.Stream()), I.want(order, masked, max(I.NPTS)), "side stream")


# ---------------------------------------------------------------------------------- 2: stress
@pytest.mark.parametrize("order", [R.LINEAR, R.CUBIC], ids=["linear", "cubic"])
def test_band_3_under_the_mask(lsf, order):
    _assert_equal(_run("device", order, True, max(I.NPTS), band=3.0), I.want(order, True, max(I.NPTS), band=3.0), "band 3")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("order", [R.LINEAR, R.CUBIC], ids=["linear", "cubic"])
def test_one_iteration_nan_zero_and_flat_fields(lsf, order, masked):
    _assert_equal(_run("device", order, masked, 0, iters=1), I.want(order, masked, 0, iters=1), "iters 1")
    _assert_equal(_run("device", order, masked, max(I.NPTS), kind="nan"), I.want(order, masked, max(I.NPTS), kind="nan"), "NaN and -0.0")
    _assert_equal(_run("host", order, masked, 0, kind="flat"), I.want(order, masked, 0, kind="flat"), "flat patch")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_reversed_markers_give_the_same_new_markers(lsf, masked):
    npts = max(I.NPTS)
    a = _run("device", R.CUBIC, masked, npts)
    b = _run("device", R.CUBIC, masked, npts, perm=np.arange(npts)[::-1])
    nk = a[5][0]
    assert a[4] == b[4] and a[5] == b[5] and nk > 0 and a[4] > nk
    assert _bits(a[0][nk:], b[0][nk:]) and _bits(a[1][nk:], b[1][nk:])  # the new ones bit for bit
    assert _bits(a[0][:nk][::-1], b[0][:nk]) and _bits(a[1][:nk][::-1], b[1][:nk]) and np.array_equal(npts + 1 - a[2][:nk][::-1], b[2][:nk])
    assert np.array_equal(a[3][::-1], b[3])
    _assert_equal(a, I.want(R.CUBIC, masked, npts), "forward")


@pytest.mark.parametrize("seam", ["host", "device"])
def test_optional_outputs_may_be_null(lsf, seam):
    want = I.want(R.CUBIC, True, 65)
    _assert_equal(_run(seam, R.CUBIC, True, 65, with_status=False), want, "no status")
    _assert_equal(_run(seam, R.CUBIC, True, 65, want_info=False), want, "no info")
    _assert_equal(_run(seam, R.CUBIC, True, 65, with_src=False), want, "no src")


# ---------------------------------------------------------------------------------- 3: the keep rules and the refusals
@pytest.mark.parametrize("seam", ["host", "device"])
def test_keep_rules(lsf, seam):
    lib = _lib()
    assert lib.lsf_release_workspace() == 0
    assert _get(seam, 4)[0] != 0  # a get without a call
    phi, mask = I.fields()
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    p = mk(phi)
    rc, nout, info, msg = _raw(seam, p, None, None, None, 0, None)
    assert rc == 0 and nout > 0, msg
    assert _get(seam, nout)[0] == 0
    assert _get(seam, nout)[0] != 0  # a get twice
    rc, nout, _, _ = _raw(seam, p, None, None, None, 0, None)
    assert rc == 0
    rc, n2, inf, _ = _raw(seam, p, None, None, None, 0, None, per_cell=0)  # a failing call drops the kept result
    assert rc != 0 and n2 == SENT and inf == [SENT] * R.INFO_LEN
    assert _get(seam, nout)[0] != 0
    rc, nout, _, _ = _raw(seam, p, None, None, None, 0, None)
    assert rc == 0 and lib.lsf_release_workspace() == 0  # lsf_release_workspace drops it
    assert _get(seam, nout)[0] != 0
    # a second call releases the un-fetched result of the first and its own result is the one fetched
    rc, n1, _, _ = _raw(seam, p, None, None, None, 0, None, seed=1)
    rc2, n2, _, _ = _raw(seam, p, None, None, None, 0, None, seed=SEED)
    assert rc == 0 and rc2 == 0
    rc, po, ro, so = _get(seam, n2)
    w = I.want(R.CUBIC, False, 0)
    assert rc == 0 and _bits(po, w.pts) and _bits(ro, w.rad) and np.array_equal(so, w.src)


@pytest.mark.parametrize("seam", ["host", "device"])
def test_every_refusal_leaves_the_sentinels(lsf, seam):
    phi, mask = I.fields()
    pts, rad = I.markers(65)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    p, m, x, r = mk(phi), mk(mask), mk(pts), mk(rad)
    status = mk(np.full(65, SENT, np.int32))
    nan, inf = float("nan"), float("inf")
    bad = [dict(phi=None), dict(lo=None), dict(want_nout=False), dict(npts=-1), dict(pts=None), dict(rad=None), dict(n=(0, N[1], N[2])),
           dict(n=(2047, 2047, 2047)), dict(dx=0.0), dict(dx=nan), dict(lo=(0.0, inf, 0.0)), dict(per_cell=0), dict(per_cell=4097), dict(rmin=nan),
           dict(rmax=inf), dict(band=nan), dict(rmin=0.0), dict(rmin=0.6), dict(band=0.1), dict(order=2), dict(iters=0), dict(iters=65),
           dict(tol=-1.0), dict(tol=nan), dict(status="phi"), dict(status="pts"), dict(status="rad"), dict(status="mask")]
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    for b in bad:
        a = dict(phi=p, mask=m, pts=x, rad=r, npts=65, status=status)
        kw = {}
        for k, v in b.items():
            if k == "status":
                a["status"] = {"phi": p, "pts": x, "rad": r, "mask": m}[v]
            elif k in a:
                a[k] = v
            else:
                kw[k] = v
        rc, nout, info, msg = _raw(seam, a["phi"], a["mask"], a["pts"], a["rad"], a["npts"], a["status"], **kw)
        assert rc == 2 and msg, (b, rc, msg)  # LSF_ERR_INVALID
        assert nout == SENT and info == [SENT] * R.INFO_LEN, b
        assert np.all(back(status) == SENT), b
        assert _get(seam, 1)[0] != 0, b  # nothing was kept
    assert _bits(back(p), phi.ravel(order="F")) and _bits(back(x), pts.ravel(order="F")) and _bits(back(r), rad)


# ---------------------------------------------------------------------------------- 4: the public Python call
@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "torch"])
def test_reseed_particles_python(lsf, dev):
    import torch

    phi, mask = I.fields()
    pts, rad = I.markers(2037)
    want = I.want(R.CUBIC, True, 2037)
    if dev:
        f = lambda a: torch.from_numpy(np.array(a.ravel(order="F"))).cuda()
        rep = lsf.reseedParticles(f(phi), *N, I.DX, I.LO, torch.from_numpy(np.ascontiguousarray(pts.T)).cuda().t(), torch.from_numpy(rad).cuda(),
                                  mask=f(mask), order="cubic", seed=SEED, **I.MAIN)
        assert rep.pts.is_cuda and rep.pts.t().is_contiguous()
        got = (rep.pts.cpu().numpy(), rep.rad.cpu().numpy(), rep.src.cpu().numpy(), rep.status.cpu().numpy())
    else:
        rep = lsf.reseedParticles(np.array(phi, order="F"), *N, I.DX, I.LO, pts, rad, mask=np.array(mask, order="F"), order="cubic", seed=SEED, **I.MAIN)
        assert rep.pts.flags.f_contiguous
        got = (rep.pts, rep.rad, rep.src, rep.status)
    _assert_equal(got + (len(got[1]), list(rep.info)), want, "python")
    # from scratch, and the result feeds the next reseed
    rep0 = lsf.reseedParticles(f(phi) if dev else np.array(phi, order="F"), *N, I.DX, I.LO, order="linear", seed=SEED, **I.MAIN)
    w0 = I.want(R.LINEAR, False, 0)
    assert list(rep0.info) == w0.info and _bits(rep0.pts.cpu().numpy() if dev else rep0.pts, w0.pts)
    rep1 = lsf.reseedParticles(f(phi) if dev else np.array(phi, order="F"), *N, I.DX, I.LO, rep0.pts, rep0.rad, order="linear", seed=SEED + 1, **I.MAIN)
    w1 = R.reseed_points(phi, I.DX, I.LO, w0.pts, w0.rad, order=R.LINEAR, seed=SEED + 1, **I.MAIN)
    assert list(rep1.info) == w1.info and _bits(rep1.pts.cpu().numpy() if dev else rep1.pts, w1.pts)
    assert _bits(rep1.rad.cpu().numpy() if dev else rep1.rad, w1.rad)
