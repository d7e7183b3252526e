"""lsf_cast_rays on the GPU against tests/cast_ref.py, the numpy statement of the contract in include/lsf.h, on both seams: thit, hit,
grad, qval, status and info are compared with `==` on the bit patterns, NaNs by position.

The grid (12 x 9 x 7 cells), the fields and the ray sets are those of tests/cast_cases.py; that they hold what they claim -- at least
half the rays of every set of 256 or more HIT, every other status in the largest set -- is asserted on the statement alone in
tests/test_cast_rays_cpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cast_cases as K
import cast_ref as C
from conftest import ROOT

pytestmark = pytest.mark.gpu

N, SHAPE, DX, LO, PAR = K.N, K.SHAPE, K.DX, K.LO, K.PAR
SENT = -7.0
OUTS = ("thit", "hit", "grad", "qval", "status")
PAR_ORDER = ("iso", "tmin", "tmax", "safety", "smin", "smax", "skip", "refine", "max_steps")


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


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


def _raw(lib, seam, phi, mask, q, n, dx, lo, org, dir, nrays, order, par, outs, info="given", stream=None):
    """the C call; phi, mask, q, org, dir and outs[name] are numpy arrays (host seam), torch tensors (device seam) or None:
    (rc, info, message)"""
    inf = np.full(9, -7, np.int64)
    lo = None if lo is None else np.array(lo, dtype=np.float64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), ptr(q), n[0], n[1], n[2], dx, None if lo is None else lo.ctypes.data, ptr(org), ptr(dir), nrays, order,
            *(par[k] for k in PAR_ORDER), *(ptr(outs.get(k)) for k in OUTS), inf.ctypes.data if info == "given" else None)
    rc = lib.lsf_cast_rays_device(*args, stream) if seam == "device" else lib.lsf_cast_rays(*args)
    return rc, [int(v) for v in inf], (lib.lsf_last_error() or b"").decode()


def _fresh_outs(seam, nrays, names=OUTS, pad=0):
    mk = {"thit": (nrays, np.float64), "hit": (3 * nrays, np.float64), "grad": (3 * nrays, np.float64), "qval": (nrays, np.float64),
          "status": (nrays, np.int32)}
    outs = {k: np.full(mk[k][0] + pad, SENT, mk[k][1]) for k in names}
    return {k: _dev(v) for k, v in outs.items()} if seam == "device" else outs


def _home(seam, outs, nrays):
    h = {k: (v.cpu().numpy() if seam == "device" else v) for k, v in outs.items()}
    return {k: (v.reshape((nrays, 3), order="F") if k in ("hit", "grad") else v) for k, v in h.items()}


def _run(seam, order, hasmask, hasq, nrays, names=None, stream=None):
    """one call through one seam on fresh copies: (outs at home, info); asserts LSF_OK and that the inputs are unchanged"""
    import torch
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi, mask, q = K.fields()
    org, dir_ = K.rays(nrays)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    p, m, qq, o, d = mk(phi), mk(mask) if hasmask else None, mk(q) if hasq else None, mk(org), mk(dir_)
    if names is None:
        names = [k for k in OUTS if k != "qval" or hasq]
    outs = _fresh_outs(seam, nrays, names)
    if seam == "device":
        _lib.check(lib.lsf_set_device(0))
        torch.cuda.synchronize()
    st = None if stream is None else stream.cuda_stream
    rc, info, msg = _raw(lib, seam, p, m, qq, N, DX, LO, o, d, nrays, order, PAR, outs, stream=st)
    assert rc == 0, msg
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert _bits(back(p), phi.ravel(order="F")) and _bits(back(o), org.ravel(order="F")) and _bits(back(d), dir_.ravel(order="F"))
    assert m is None or np.array_equal(back(m), mask.ravel(order="F"))
    assert qq is None or _bits(back(qq), q.ravel(order="F"))
    return _home(seam, outs, nrays), info


def _assert_equal(got, info, want, what):
    for k in got:
        w = getattr(want, k)
        assert w is not None, (what, k)
        bad = 0 if _bits(got[k], w) else int(np.count_nonzero(~((got[k] == w) | (np.isnan(got[k].astype(np.float64)) & np.isnan(w.astype(np.float64))))))
        print(f"{what} {k}: differs at {bad} entries")
        assert _bits(got[k], w), (what, k)
    print(f"{what} info {info}, want {want.info}")
    assert info == want.info, what


# ---------------------------------------------------------------------------------- 1: every instance, every size, both seams
@pytest.mark.parametrize("hasq", [False, True])
@pytest.mark.parametrize("hasmask", [False, True])
@pytest.mark.parametrize("order", [C.LINEAR, C.CUBIC], ids=["linear", "cubic"])
def test_every_output_equals_the_statement(lsf, order, hasmask, hasq):
    import torch

    for nrays in K.NRAYS:
        want = K.want(order, hasmask, hasq, nrays)
        dev, dinfo = _run("device", order, hasmask, hasq, nrays)
        assert sorted(dev) == sorted(k for k in OUTS if k != "qval" or hasq)
        _assert_equal(dev, dinfo, want, f"nrays={nrays} device")
        host, hinfo = _run("host", order, hasmask, hasq, nrays)
        _assert_equal(host, hinfo, want, f"nrays={nrays} host")
    again, ainfo = _run("device", order, hasmask, hasq, K.NRAYS[-1], stream=torch.cuda.Stream())  # a second run, on a side stream
    _assert_equal(again, ainfo, K.want(order, hasmask, hasq, K.NRAYS[-1]), "side stream")


# ---------------------------------------------------------------------------------- 2: optional outputs NULL, one at a time
@pytest.mark.parametrize("seam", ["host", "device"])
def test_optional_outputs_may_be_null_one_at_a_time(lsf, seam):
    from levelsetfortran_amd import _lib

    inst = (C.CUBIC, True, True)
    want = K.want(*inst, 256)
    for drop in ("hit", "grad", "qval", "status"):
        names = [k for k in OUTS if k != drop]
        got, info = _run(seam, *inst, 256, names=names)
        assert sorted(got) == sorted(names)
        _assert_equal(got, info, want, f"without {drop}")
    lib = _lib.load()
    phi, mask, q = K.fields()
    org, dir_ = K.rays(256)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    outs = _fresh_outs(seam, 256)
    rc, info, msg = _raw(lib, seam, mk(phi), mk(mask), mk(q), N, DX, LO, mk(org), mk(dir_), 256, C.CUBIC, PAR, outs, info=None)
    assert rc == 0 and info == [-7] * 9, msg
    _assert_equal(_home(seam, outs, 256), want.info, want, "without info")
    # thit alone; q without qval is legal
    got, info = _run(seam, C.LINEAR, False, True, 65, names=["thit"])
    _assert_equal(got, info, K.want(C.LINEAR, False, True, 65), "thit alone")


# ---------------------------------------------------------------------------------- 3: the named rays of the CPU test
@pytest.mark.parametrize("seam", ["host", "device"])
def test_named_status_rays_and_band_cases(lsf, seam):
    import test_cast_rays_cpu as T
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))

    def both(f, dx, o, d, order, par, mask=None, what=""):
        o, d = np.asfortranarray(o, dtype=np.float64), np.asfortranarray(d, dtype=np.float64)
        want = C.cast_rays(f, dx, T.LO, o, d, order=order, mask=mask, **par)
        n = tuple(v - 1 for v in f.shape)
        outs = _fresh_outs(seam, len(o), [k for k in OUTS if k != "qval"])
        rc, info, msg = _raw(lib, seam, mk(f), None if mask is None else mk(mask), None, n, dx, T.LO, mk(o), mk(d), len(o), order,
                             dict(dict(iso=0.0, tmin=0.0, tmax=1e30), **par), outs)
        assert rc == 0, msg
        _assert_equal(_home(seam, outs, len(o)), info, want, what)
        return want

    f, dx = T._sphere(17)
    cases = T._status_rays()
    o = np.array([c[0] for c in cases.values()])
    d = np.array([c[1] for c in cases.values()])
    for order in (C.LINEAR, C.CUBIC):
        w = both(f, dx, o, d, order, dict(T.PAR, tmax=10.0), what=f"status rays, order {order}")
        assert list(w.status) == [c[2] for c in cases.values()]
        w = both(f, dx, o[:1], d[:1], order, dict(T.PAR, max_steps=3), what="max_steps too small")
        assert w.status[0] == C.STEPS
        bad = f.copy(order="F")
        bad[2, 8, 8] = np.nan
        w = both(bad, dx, [[-1.0, 0.01, 0.02]], [[1.0, 0.0, 0.0]], order, T.PAR, what="NaN in phi")
        assert w.status[0] == C.HIT
    # the hole over the surface and the one-point hole in front of it: LOST
    f, dx, mask = T._mask_case(band=8.1)
    pricked = mask.copy(order="F")
    pricked[3, 16, 16] = 0
    w = both(f, dx, [[-0.5 + 1.2 * dx, 0.004, 0.003]], [[1.0, 0.0, 0.0]], C.LINEAR, dict(T.PAR, skip=6.5, smax=0.5), mask=pricked, what="pricked mask")
    assert w.status[0] == C.LOST
    # rays that never meet the list
    w = both(f, dx, [[-1.0, 0.45, 0.44], [0.46, -1.0, -0.45]], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], C.CUBIC, T.PAR,
             mask=T._mask_case(band=4.1)[2], what="never on the list")
    assert list(w.status) == [C.MISS, C.MISS] and w.info[6] == 0


# ---------------------------------------------------------------------------------- 4: the Python name
@pytest.mark.parametrize("seam", ["host", "device"])
def test_python_report(lsf, seam):
    import torch

    phi, mask, q = K.fields()
    org, dir_ = K.rays(256)
    want = K.want(C.CUBIC, True, True, 256)
    if seam == "device":
        mk = _dev
        vec = lambda a: torch.from_numpy(np.array(a.T, order="C")).cuda().t()  # (nrays, 3) in Fortran order (a copy)
    else:
        mk = lambda a: a.copy(order="F")
        vec = lambda a: a
    rep = lsf.castRays(mk(phi), *N, DX, LO, vec(org), vec(dir_), order="cubic", mask=mk(mask), q=mk(q), **PAR)
    assert isinstance(rep, lsf.CastReport)
    home = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert tuple(rep.hit.shape) == (256, 3) and tuple(rep.grad.shape) == (256, 3)
    _assert_equal({k: home(getattr(rep, k)) for k in OUTS}, list(rep.info), want, "castRays")
    lean = lsf.castRays(mk(phi), *N, DX, LO, vec(org), vec(dir_), order="linear", want_hit=False, want_grad=False, **PAR)
    assert lean.hit is None and lean.grad is None and lean.qval is None
    w = K.want(C.LINEAR, False, False, 256)
    assert _bits(home(lean.thit), w.thit) and list(lean.info) == w.info
    with pytest.raises(ValueError):
        lsf.castRays(mk(phi), *N, DX, LO, vec(org), vec(dir_), order="quintic")
    with pytest.raises(ValueError):
        lsf.castRays(mk(phi), *N, DX, LO, vec(org), vec(dir_), max_steps=0)


# ---------------------------------------------------------------------------------- 5: the chain from the mesh
@pytest.mark.parametrize("seam", ["host", "device"])
def test_wall_thickness_from_the_nodes_of_the_mesh(lsf, seam):
    """extractSurface -> samplePoints (grad at the nodes) -> castRays from every node against its gradient with tmin = 2 dx: the
    thickness of a slab.  phi = |x - c| - h with c on a grid plane is piecewise linear with its kink on that plane, so the linear
    interpolant is the field itself and thit is 2 h to rounding (1e-12, the bound of the plane test); every output equals the
    statement fed with the same nodes and gradients, and the padding behind each output keeps its sentinel."""
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    n, dx, lo = (16, 12, 10), 0.0625, (-0.5, -0.25, 0.0)
    ax = [lo[A] + np.arange(n[A] + 1) * dx for A in range(3)]
    x = np.meshgrid(*ax, indexing="ij")[0]
    c, h = 0.0, 2.25 * dx
    phi = np.asfortranarray(np.abs(x - c) - h)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    home = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    p = mk(phi)
    sX, sE, sinfo = lsf.extractSurface(p, *n, dx, lo)
    smp = lsf.samplePoints(p, *n, dx, lo, sX, order="linear")
    nodes, grad = np.asfortranarray(home(sX)), np.asfortranarray(home(smp.grad))
    nr = len(nodes)
    assert nr > 200 and smp.info[0] == nr and np.all(np.abs(np.abs(grad[:, 0]) - 1.0) < 1e-12)
    par = dict(iso=0.0, tmin=2.0 * dx, tmax=1.0, safety=0.9, smin=0.05, smax=1.0, skip=1.0, refine=30, max_steps=100)
    want = C.cast_rays(phi, dx, lo, nodes, -grad, order=C.LINEAR, **par)
    assert want.info[0] == nr and np.all(np.abs(want.thit - 2.0 * h) <= 1e-12), (want.info, np.abs(want.thit - 2.0 * h).max())
    raw = np.array if seam == "host" else (lambda a: _dev(np.asarray(a)))
    o = raw(nodes.ravel(order="F"))
    d = raw((-grad).ravel(order="F"))
    pad = 5
    outs = _fresh_outs(seam, nr, [k for k in OUTS if k != "qval"], pad=pad)
    pp = raw(phi.ravel(order="F"))
    rc, info, msg = _raw(lib, seam, pp, None, None, n, dx, lo, o, d, nr, C.LINEAR, par, outs)
    assert rc == 0, msg
    got = {k: home(v) for k, v in outs.items()}
    for k, v in got.items():
        assert np.all(v[-pad:] == SENT), k  # untouched
    trimmed = {k: (v[:-pad].reshape((nr, 3), order="F") if k in ("hit", "grad") else v[:-pad]) for k, v in got.items()}
    _assert_equal(trimmed, info, want, "thickness")
    assert np.all(np.abs(trimmed["thit"] - 2.0 * h) <= 1e-12) and info[8] == nr  # every ray begins inside the slab


# ---------------------------------------------------------------------------------- 6: errors
@pytest.mark.parametrize("seam", ["host", "device"])
def test_invalid_arguments_leave_everything_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    _lib.check(lib.lsf_set_device(0))
    phi0, mask0, q0 = K.fields()
    nrays = 65
    org0, dir0 = K.rays(nrays)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    phi, mask, q, org, dir_ = mk(phi0), mk(mask0), mk(q0), mk(org0), mk(dir0)
    outs = _fresh_outs(seam, nrays)
    ok = dict(phi=phi, mask=mask, q=q, n=N, dx=DX, lo=LO, org=org, dir=dir_, nrays=nrays, order=C.CUBIC, par=PAR, outs=outs)
    nan, inf = float("nan"), float("inf")

    def swap(**kw):
        return dict(outs=dict(outs, **kw))

    def par(**kw):
        return dict(par=dict(PAR, **kw))

    cases = {
        "NULL phi": dict(phi=None), "NULL org": dict(org=None), "NULL dir": dict(dir=None), "NULL thit": swap(thit=None), "NULL xLo": dict(lo=None),
        "nrays = 0": dict(nrays=0), "nrays < 0": dict(nrays=-3),
        "nx = 0": dict(n=(0, N[1], N[2])), "nz < 0": dict(n=(N[0], N[1], -1)), "too many points": dict(n=(2047, 2047, 511)),
        "dx = 0": dict(dx=0.0), "dx < 0": dict(dx=-DX), "dx NaN": dict(dx=nan), "dx inf": dict(dx=inf),
        "xLo NaN": dict(lo=(LO[0], nan, LO[2])), "xLo inf": dict(lo=(inf, LO[1], LO[2])),
        "iso NaN": par(iso=nan), "iso inf": par(iso=-inf), "order 2": dict(order=2), "order -1": dict(order=-1),
        "tmin < 0": par(tmin=-0.5), "tmin NaN": par(tmin=nan), "tmin inf": par(tmin=inf), "tmax = tmin": par(tmin=1.0, tmax=1.0),
        "tmax < tmin": par(tmin=1.0, tmax=0.5), "tmax NaN": par(tmax=nan), "tmax inf": par(tmax=inf),
        "safety = 0": par(safety=0.0), "safety > 1": par(safety=1.0 + 2.0 ** -52), "safety NaN": par(safety=nan), "safety < 0": par(safety=-0.5),
        "smin = 0": par(smin=0.0), "smin NaN": par(smin=nan), "smin inf": par(smin=inf, smax=inf), "smax < smin": par(smin=0.5, smax=0.25),
        "smax NaN": par(smax=nan), "smax inf": par(smax=inf), "skip = 0": par(skip=0.0), "skip < 0": par(skip=-1.0), "skip NaN": par(skip=nan),
        "skip inf": par(skip=inf), "refine < 0": par(refine=-1), "max_steps = 0": par(max_steps=0), "max_steps < 0": par(max_steps=-5),
        "qval without q": dict(q=None),
        "thit is phi": swap(thit=phi), "grad is q": swap(grad=q), "status is mask": swap(status=mask), "hit is org": swap(hit=org),
        "grad is dir": swap(grad=dir_), "qval is thit": swap(qval=outs["thit"]), "hit is grad": swap(hit=outs["grad"]),
        "thit inside grad": swap(thit=outs["grad"][nrays:2 * nrays]), "qval is the tail of hit": swap(qval=outs["hit"][2 * nrays:3 * nrays]),
        "thit is the tail of dir": swap(thit=dir_[2 * nrays + 1:3 * nrays]),
    }
    for name, change in cases.items():
        rc, info, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg.startswith("lsf_cast_rays: ") and info == [-7] * 9, (name, msg)  # nothing reported
        for k, v in outs.items():
            assert np.all(back(v) == SENT), (name, k)  # nothing written
        assert _bits(back(phi), phi0.ravel(order="F")) and np.array_equal(back(mask), mask0.ravel(order="F")), name
        assert _bits(back(q), q0.ravel(order="F")) and _bits(back(org), org0.ravel(order="F")) and _bits(back(dir_), dir0.ravel(order="F")), name
    # a valid call follows the refusals; skip is checked but not used without a mask; safety = 1 and smin = smax are legal
    rc, info, msg = _raw(lib, seam, **ok)
    assert rc == 0, msg
    _assert_equal(_home(seam, outs, nrays), info, K.want(C.CUBIC, True, True, nrays), "after the refusals")
    edge = dict(PAR, safety=1.0, smin=0.5, smax=0.5, refine=0, max_steps=1)
    outs2 = _fresh_outs(seam, nrays, ["thit", "status"])
    rc, info, msg = _raw(lib, seam, **dict(ok, mask=None, q=None, par=edge, outs=outs2))
    assert rc == 0, msg
    _assert_equal(_home(seam, outs2, nrays), info, C.cast_rays(phi0, DX, LO, org0, dir0, order=C.CUBIC, **edge), "edge parameters")


def test_a_refused_call_leaves_an_unsynced_phi_twin_intact(lsf):
    """Under LSF_MIRROR_TRUST | LSF_MIRROR_LAZY a reinit leaves its result in phi's device twin and the host array stale.  A valid
    castRays reads the twin; a refused one touches nothing; the sync then brings the reinit's result home."""
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask0, q0 = K.fields()
    org, dir_ = K.rays(256)
    h = 0.3 * DX
    dev = _dev(phi0)
    lsf.reinit(dev, None, None, *N, 2, DX, h, tol=0.0, order="jacobi", arith="fast")
    moved = dev.cpu().numpy().reshape(SHAPE, order="F")
    assert not np.array_equal(moved, phi0)
    want = C.cast_rays(moved, DX, LO, org, dir_, order=C.CUBIC, **PAR)
    try:
        _lib.check(lib.lsf_mirror(3))  # LSF_MIRROR_TRUST | LSF_MIRROR_LAZY
        P = phi0.copy(order="F")
        lsf.reinit(P, None, None, *N, 2, DX, h, tol=0.0, order="jacobi", arith="fast")
        assert _bits(P, phi0)  # un-synced: the host copy is what it was
        rep = lsf.castRays(P, *N, DX, LO, org, dir_, order="cubic", **PAR)
        _assert_equal({k: getattr(rep, k) for k in ("thit", "hit", "grad", "status")}, list(rep.info), want, "from the twin")
        assert _bits(P, phi0)  # phi is an input only: still not home
        for kw in (dict(order=9), dict(par=dict(PAR, tmax=float("nan"))), dict(dx=-1.0)):
            outs = _fresh_outs("host", 256, ["thit", "hit", "grad", "status"])
            a = dict(dict(phi=P, mask=None, q=None, n=N, dx=DX, lo=LO, org=np.array(org.ravel(order="F")), dir=np.array(dir_.ravel(order="F")),
                          nrays=256, order=C.CUBIC, par=PAR, outs=outs), **kw)
            rc, info, msg = _raw(lib, "host", **a)
            assert rc == _lib.LSF_ERR_INVALID and info == [-7] * 9 and all(np.all(v == SENT) for v in outs.values()), (kw, msg)
            assert _bits(P, phi0)
        _lib.check(lib.lsf_mirror_sync(P.ctypes.data))
        assert _bits(P, moved)  # the earlier un-synced result, intact
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())


# ---------------------------------------------------------------------------------- 7: the Fortran shim
EXE = os.path.join(ROOT, "build", "dropin", "host_cast.exec")


@pytest.fixture(scope="module")
def host_cast_exe():
    path = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    if not os.path.exists(EXE):
        fc = shutil.which("amdflang", path=path)
        if fc is None:
            pytest.skip("no amdflang: tests/fortran/host_cast.f90 cannot be built")
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetfortran_amd", "fortran"), "cast", f"FC={fc}"], env=dict(os.environ, PATH=path),
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and os.path.exists(EXE), p.stdout[-3000:]
    return EXE


@pytest.mark.parametrize("resident", ["0", "2"])
def test_cast_rays_through_the_fortran_wrapper(lsf, host_cast_exe, tmp_path, resident):
    """tests/fortran/host_cast.f90: castRays of lsf_hip.f90 with a mask and q gives the statement's bits and prints its counts"""
    phi, mask, q = K.fields()
    nrays = 256
    org, dir_ = K.rays(nrays)
    want = K.want(C.CUBIC, True, True, nrays)
    with open(tmp_path / "cast_in.bin", "wb") as f:
        f.write(np.array([*N, nrays, C.CUBIC, PAR["refine"], PAR["max_steps"]], np.int32).tobytes())
        f.write(np.array([DX, *LO, *(PAR[k] for k in PAR_ORDER[:7])], np.float64).tobytes())
        for a in (phi, mask, q, org, dir_):
            f.write(a.tobytes(order="F"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSF_")}
    env.update(LSF_RESIDENT=resident)
    p = subprocess.run(f"ulimit -s unlimited; cd {tmp_path}; {host_cast_exe}", shell=True, env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    print(p.stdout)
    raw = open(tmp_path / "cast_out.bin", "rb").read()
    assert len(raw) == nrays * (8 * 8 + 4)
    d = np.frombuffer(raw, np.float64, 8 * nrays)
    got = {"thit": d[:nrays], "hit": d[nrays:4 * nrays].reshape((nrays, 3), order="F"), "grad": d[4 * nrays:7 * nrays].reshape((nrays, 3), order="F"),
           "qval": d[7 * nrays:], "status": np.frombuffer(raw, np.int32, nrays, 64 * nrays)}
    _assert_equal(got, want.info, want, "Fortran")
    import re

    line = " ".join(p.stdout.split())
    nums = [int(v) for v in re.findall(r"(?:rays|hit|miss|no grid|bad|lost|out of steps|samples|strides|began inside)\s+(\d+)", line)]
    assert nums == [nrays, *want.info], (nums, want.info)
