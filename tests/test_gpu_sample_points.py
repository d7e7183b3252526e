"""lsf_sample_points on the GPU against tests/sample_ref.py, the numpy statement of the contract in include/lsf.h, on both seams: val,
grad, qval, foot, status and info are compared with `==` on the bit patterns, NaNs by position.

Grid: nx, ny, nz = 12, 9, 7 cells (13 x 10 x 8 points): three different strides, cubic cells on every axis.  phi is a sphere plus a
smooth perturbation, q another smooth field, the mask every interior point but three holes (0, 7, -1) and 1s on the walls, which
no list holds.  dx and xLo are binary fractions, so that points exactly on grid points and walls can be made.
Points (npts in 1, 63, 65, 256, 2037: one lane, a ragged wave, a wave and a lane, a block, eight blocks the last ragged): random
points, grid points and wall points, and from the 71st on, one in fourteen, the special points of the CPU test (just outside, on
the wall, one ulp beyond it, NaN, +-inf, 1e300).  With a mask most points are drawn from the cells whose cubic stencil lies in the
interior, without one from anywhere: the statement alone leaves no more than 10 % of them OUTSIDE or OFFBAND, which the first test
asserts."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import sample_ref as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

N = (12, 9, 7)
SHAPE = tuple(n + 1 for n in N)
DX, LO = 0.125, (-0.75, 0.25, 1.0)
CENTRE, RADIUS = (0.0, 0.8125, 1.4375), 0.125  # the middle of the grid; the level set lies in the cells whose cubic stencil is interior
ISO, TOL, ITERS = 0.02, 1e-6, 4
NPTS = [1, 63, 65, 256, 2000 + 37]
INSTANCES = [(o, hq, hm, it) for o in (S.LINEAR, S.CUBIC) for hq in (False, True) for hm in (False, True) for it in (0, ITERS)]
SENT = -7.0


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _fields():
    """(phi, mask, q), shared and read-only"""
    ax = [LO[A] + np.arange(SHAPE[A]) * DX for A in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    r = np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2)
    phi = np.asfortranarray(r - RADIUS + 0.02 * np.sin(3.0 * x) * np.cos(2.0 * y + z))
    q = np.asfortranarray(1.25 + 0.5 * x - np.sin(2.0 * y) * (0.75 + z))
    mask = np.ones(SHAPE, np.int32, order="F")  # 1s on the walls too: they are in no list
    mask[1, 1, 1], mask[11, 8, 6], mask[1, 8, 1] = 0, 7, -1  # (near the corners: on so small a grid a hole in the middle empties it)
    for a in (phi, mask, q):
        a.setflags(write=False)
    return phi, mask, q


@functools.lru_cache(maxsize=None)
def _points(npts, masked):
    """(npts, 3) in Fortran order, read-only"""
    rng = np.random.default_rng(100 + npts + (1000 if masked else 0))
    lo, n = np.asarray(LO), np.asarray(N)
    anywhere = lambda m: lo + rng.random((m, 3)) * n * DX
    central = lambda m: lo + (2.0 + rng.random((m, 3)) * (n - 4.0)) * DX  # i0 in 2 .. n-3: the cubic stencil is interior
    grid = lambda m, a, b: lo + np.stack([rng.integers(a[A], b[A] + 1, m) for A in range(3)], axis=1) * DX
    special, _ = S.special_points(SHAPE, DX, LO)
    if masked:  # the points that a mask refuses wherever they fall near a wall are rationed like the special ones
        body = np.concatenate([central(1753), grid(200, (2, 2, 2), n - 3)])
        extra = np.concatenate([special, anywhere(40), grid(20, (0, 0, 0), n)])
    else:
        body = np.concatenate([anywhere(1563), grid(450, (0, 0, 0), n)])
        extra = special
    rng.shuffle(body)
    rng.shuffle(extra)
    assert len(body) + len(extra) == 2037
    # the extra points from the 71st on, one every 14 points: none in the three smallest sets, all of them in the largest
    out = list(body[:70])
    rest = list(body[70:])
    for p in extra:
        out.extend(rest[:13])
        rest = rest[13:]
        out.append(p)
    out.extend(rest)
    pts = np.asfortranarray(np.array(out)[:npts])
    assert pts.shape == (npts, 3)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _want(order, hasq, hasmask, iters, npts):
    phi, mask, q = _fields()
    return S.sample_points(phi, DX, LO, _points(npts, hasmask), order=order, mask=mask if hasmask else None, q=q if hasq else None, iso=ISO,
                           iters=iters, tol=TOL)


def test_the_inputs_are_what_the_docstring_says():
    special, want = S.special_points(SHAPE, DX, LO)
    for order, hasq, hasmask, iters in INSTANCES:
        for npts in NPTS:
            w = _want(order, hasq, hasmask, iters, npts)
            refused = w.info[1] + w.info[2]
            assert refused <= 0.10 * npts, (order, hasmask, iters, npts, w.info)  # the cap of the main cases
            assert sum(w.info[m] for m in (0, 1, 2, 4, 5)) == npts
        w = _want(order, hasq, hasmask, iters, 2037)
        assert w.info[1] >= np.count_nonzero(want == S.OUTSIDE) and w.info[0] > 0.85 * 2037
        assert (w.info[3] > 0) == (order == S.CUBIC and not hasmask)  # under a mask a linear fallback has a wall point in its stencil
        if hasmask:
            assert w.info[2] > 0
    pts = _points(2037, False)
    on_grid = np.all((pts - np.asarray(LO)) / DX == np.round((pts - np.asarray(LO)) / DX), axis=1)
    assert on_grid.sum() > 300 and np.isnan(pts).any() and np.isinf(pts).any() and (pts > 1e200).any()
    assert not np.isnan(_points(65, False)).any()


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


OUTS = ("val", "grad", "qval", "foot", "status")


def _raw(lib, seam, phi, mask, q, n, dx, lo, pts, npts, order, iso, iters, tol, outs, info="given", stream=None):
    """the C call; phi, mask, q, pts and outs[name] are numpy arrays (host seam), torch tensors (device seam) or None:
    (rc, info, message)"""
    inf = np.full(6, -7, np.int64)
    lo = None if lo is None else np.array(lo, dtype=np.float64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), ptr(q), n[0], n[1], n[2], dx, None if lo is None else lo.ctypes.data, ptr(pts), npts, order, iso, iters, tol,
            *(ptr(outs.get(k)) for k in OUTS), inf.ctypes.data if info == "given" else None)
    rc = lib.lsf_sample_points_device(*args, stream) if seam == "device" else lib.lsf_sample_points(*args)
    return rc, [int(v) for v in inf], (lib.lsf_last_error() or b"").decode()


def _fresh_outs(seam, npts, names=OUTS):
    mk = {"val": (npts, np.float64), "grad": (3 * npts, np.float64), "qval": (npts, np.float64), "foot": (3 * npts, np.float64),
          "status": (npts, np.int32)}
    outs = {k: np.full(mk[k][0], SENT, mk[k][1]) for k in names}
    return {k: _dev(v) for k, v in outs.items()} if seam == "device" else outs


def _home(seam, outs, npts):
    h = {k: (v.cpu().numpy() if seam == "device" else v) for k, v in outs.items()}
    return {k: (v.reshape((npts, 3), order="F") if k in ("grad", "foot") else v) for k, v in h.items()}


def _run(seam, order, hasq, hasmask, iters, npts, names=None, stream=None):
    """one call through one seam on fresh copies: (outs at home, info); asserts LSF_OK and that the inputs are unchanged"""
    import torch
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi, mask, q = _fields()
    pts = _points(npts, hasmask)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    p, m, qq, x = mk(phi), mk(mask) if hasmask else None, mk(q) if hasq else None, mk(pts)
    if names is None:
        names = [k for k in OUTS if (k != "qval" or hasq) and (k != "foot" or iters)]
    outs = _fresh_outs(seam, npts, names)
    if seam == "device":
        _lib.check(lib.lsf_set_device(0))
        torch.cuda.synchronize()
    st = None if stream is None else stream.cuda_stream
    rc, info, msg = _raw(lib, seam, p, m, qq, N, DX, LO, x, npts, order, ISO, iters, TOL, outs, stream=st)
    assert rc == 0, msg
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert _bits(back(p), phi.ravel(order="F")) and _bits(back(x), pts.ravel(order="F"))  # read, never written
    assert m is None or np.array_equal(back(m), mask.ravel(order="F"))
    assert qq is None or _bits(back(qq), q.ravel(order="F"))
    return _home(seam, outs, npts), info


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
@pytest.mark.parametrize("iters", [0, ITERS])
@pytest.mark.parametrize("hasmask", [False, True])
@pytest.mark.parametrize("hasq", [False, True])
@pytest.mark.parametrize("order", [S.LINEAR, S.CUBIC], ids=["linear", "cubic"])
def test_every_output_equals_the_statement(lsf, order, hasq, hasmask, iters):
    import torch

    for npts in NPTS:
        want = _want(order, hasq, hasmask, iters, npts)
        dev, dinfo = _run("device", order, hasq, hasmask, iters, npts)
        assert sorted(dev) == sorted(k for k in OUTS if (k != "qval" or hasq) and (k != "foot" or iters))
        _assert_equal(dev, dinfo, want, f"npts={npts} device")
        host, hinfo = _run("host", order, hasq, hasmask, iters, npts)
        _assert_equal(host, hinfo, want, f"npts={npts} host")
    again, ainfo = _run("device", order, hasq, hasmask, iters, NPTS[-1], stream=torch.cuda.Stream())  # a second run, on a side stream
    _assert_equal(again, ainfo, _want(order, hasq, hasmask, iters, NPTS[-1]), "side stream")


# ---------------------------------------------------------------------------------- 2: optional outputs NULL, one at a time
@pytest.mark.parametrize("seam", ["host", "device"])
def test_optional_outputs_may_be_null_one_at_a_time(lsf, seam):
    from levelsetfortran_amd import _lib

    inst = (S.CUBIC, True, True, ITERS)
    want = _want(*inst, 256)
    for drop in ("grad", "qval", "foot", "status", "info"):
        names = [k for k in OUTS if k != drop]
        got, info = _run(seam, *inst, 256, names=names)
        assert sorted(got) == sorted(names)
        _assert_equal(got, info, want, f"without {drop}")
    # ... info too
    lib = _lib.load()
    phi, mask, q = _fields()
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    outs = _fresh_outs(seam, 256)
    rc, info, msg = _raw(lib, seam, mk(phi), mk(mask), mk(q), N, DX, LO, mk(_points(256, True)), 256, S.CUBIC, ISO, ITERS, TOL, outs, info=None)
    assert rc == 0 and info == [-7] * 6, msg
    _assert_equal(_home(seam, outs, 256), want.info, want, "without info")
    # q without qval is legal, and q without a mask is read wherever the stencil goes
    got, info = _run(seam, S.CUBIC, True, False, 0, 65, names=["val", "status"])
    _assert_equal(got, info, _want(S.CUBIC, True, False, 0, 65), "q, no qval")


# ---------------------------------------------------------------------------------- 3: the status cases
@functools.lru_cache(maxsize=None)
def _status_case(name):
    """(phi, mask, pts, kwargs of the statement) of the status cases of tests/test_sample_points_cpu.py on this grid"""
    phi, mask, q = _fields()
    mid = np.array([LO[A] + (N[A] / 2 + 0.3) * DX for A in range(3)])
    if name == "special":
        pts, _ = S.special_points(SHAPE, DX, LO)
        return phi, None, pts, dict(order=S.CUBIC, iters=2)
    if name == "mask rule":  # the cells around the three holes, the wall cells and the cells next to them, under the mask
        i = np.array([(a, b, c) for a in range(N[0]) for b in range(N[1]) for c in range(N[2])], dtype=np.float64)
        return phi, mask, np.asarray(LO) + (i + 0.5) * DX, dict(order=S.CUBIC)
    if name == "mask rule linear":
        i = np.array([(a, b, c) for a in range(N[0]) for b in range(N[1]) for c in range(N[2])], dtype=np.float64)
        return phi, mask, np.asarray(LO) + (i + 0.25) * DX, dict(order=S.LINEAR)
    if name == "flat":
        return np.full(SHAPE, 0.5, order="F"), None, np.stack([mid, mid + 0.1]), dict(order=S.LINEAR, iters=3)
    if name == "not converged":  # one move from the corner region, far from the sphere
        far = np.asarray(LO) + np.array([[1.3, 1.2, 1.4], [10.6, 7.5, 5.5]]) * DX
        return phi, None, far, dict(order=S.LINEAR, iters=1, tol=1e-12)
    if name == "walks out of the mask":
        m = np.asfortranarray((phi > 1.2 * DX).astype(np.int32))
        rng = np.random.default_rng(5)
        pts = np.asarray(LO) + (1.0 + rng.random((400, 3)) * (np.asarray(N) - 2.0)) * DX
        return phi, m, pts, dict(order=S.LINEAR, iters=6, tol=1e-9, iso=0.0)
    assert name == "walks out of the grid"
    ax = LO[0] + np.arange(SHAPE[0]) * DX
    ramp = np.asfortranarray(np.broadcast_to(ax[:, None, None], SHAPE) + 0.0)
    return ramp, None, np.stack([mid, mid - 0.2]), dict(order=S.CUBIC, iters=3, iso=-5.0)


STATUS_CASES = {"special": S.OUTSIDE, "mask rule": S.OFFBAND, "mask rule linear": S.OFFBAND, "flat": S.FLAT, "not converged": S.NOT_CONVERGED,
                "walks out of the mask": S.OFFBAND, "walks out of the grid": S.OUTSIDE}


@pytest.mark.parametrize("seam", ["host", "device"])
@pytest.mark.parametrize("name", sorted(STATUS_CASES))
def test_status_cases(lsf, name, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi, mask, pts, kw = _status_case(name)
    kw = dict(dict(iso=ISO, iters=0, tol=TOL), **kw)
    pts = np.asfortranarray(pts)
    want = S.sample_points(phi, DX, LO, pts, mask=mask, **kw)
    assert STATUS_CASES[name] in want.status, want.info
    if name.startswith("walks"):  # the own sample of some of those points was taken: val is theirs, foot the last y
        walked = (want.status == STATUS_CASES[name]) & ~np.isnan(want.val)
        assert walked.any() and not np.isnan(want.foot[walked]).any() and not np.array_equal(want.foot[walked], pts[walked])
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    npts = len(pts)
    outs = _fresh_outs(seam, npts, [k for k in OUTS if k != "qval" and (k != "foot" or kw["iters"])])
    rc, info, msg = _raw(lib, seam, mk(phi), None if mask is None else mk(mask), None, N, DX, LO, mk(pts), npts, kw["order"], kw["iso"], kw["iters"],
                         kw["tol"], outs)
    assert rc == 0, msg
    _assert_equal(_home(seam, outs, npts), info, want, name)


@pytest.mark.parametrize("seam", ["host", "device"])
def test_offband_by_the_outer_ring_alone(lsf, seam):
    """cubic under the mask, in cells whose eight corners are on the list while a point of the outer ring of the 4 x 4 x 4 stencil
    is not (the hole at (1, 1, 1)), and in their neighbours: the corners pass the band rule, the ring decides"""
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi, mask, q = _fields()
    pts, want = S.ring_points(phi, mask, DX, LO)  # (asserts that both kinds of point are there)
    npts = len(pts)
    for hasq, iters in ((False, 0), (True, ITERS)):
        w = S.sample_points(phi, DX, LO, pts, order=S.CUBIC, mask=mask, q=q if hasq else None, iso=ISO, iters=iters, tol=TOL)
        assert np.array_equal(w.status == S.OFFBAND, want.status == S.OFFBAND)
        mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
        outs = _fresh_outs(seam, npts, [k for k in OUTS if (k != "qval" or hasq) and (k != "foot" or iters)])
        rc, info, msg = _raw(lib, seam, mk(phi), mk(mask), mk(q) if hasq else None, N, DX, LO, mk(pts), npts, S.CUBIC, ISO, iters, TOL, outs)
        assert rc == 0, msg
        _assert_equal(_home(seam, outs, npts), info, w, f"outer ring, q {hasq}, iters {iters}")


# ---------------------------------------------------------------------------------- 4: the Python name
@pytest.mark.parametrize("seam", ["host", "device"])
def test_python_report(lsf, seam):
    import torch

    phi, mask, q = _fields()
    pts = _points(256, True)
    want = _want(S.CUBIC, True, True, ITERS, 256)
    if seam == "device":
        mk = _dev
        x = torch.from_numpy(np.array(pts.T, order="C")).cuda().t()  # (npts, 3) in Fortran order (a copy: the shared points are read-only)
    else:
        mk = lambda a: a.copy(order="F")
        x = pts
    rep = lsf.samplePoints(mk(phi), *N, DX, LO, x, order="cubic", mask=mk(mask), q=mk(q), iso=ISO, iters=ITERS, tol=TOL)
    assert isinstance(rep, lsf.SampleReport)
    home = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert tuple(rep.grad.shape) == (256, 3) and tuple(rep.foot.shape) == (256, 3)
    _assert_equal({k: home(getattr(rep, k)) for k in OUTS}, list(rep.info), want, "samplePoints")
    lean = lsf.samplePoints(mk(phi), *N, DX, LO, x, order="linear", want_grad=False)  # the optional arguments may be left out
    assert lean.grad is None and lean.qval is None and lean.foot is None
    w = S.sample_points(phi, DX, LO, pts, order=S.LINEAR)
    assert _bits(home(lean.val), w.val) and list(lean.info) == w.info
    with pytest.raises(ValueError):
        lsf.samplePoints(mk(phi), *N, DX, LO, x, order="quintic")
    with pytest.raises(ValueError):
        lsf.samplePoints(mk(phi), *N, DX, LO, x, iters=-1)


# ---------------------------------------------------------------------------------- 5: the chains
@pytest.mark.parametrize("seam", ["host", "device"])
def test_extracted_nodes_sample_to_iso_and_kappa_plugs_in(lsf, seam):
    """extractSurface -> samplePoints (linear): |val - iso| within sample_ref.node_value_bound, the bound derived there from the
    rounding of the node coordinate (and, for the nodes on the diagonals of the Kuhn tetrahedra, from the mixed differences of the
    cell), which the statement meets on the CPU in tests/test_sample_points_cpu.py.  extractSurface -> curvatureBand ->
    samplePoints(q = kappa, mask |phi| < 4.1 dx): no OFFBAND, qval the statements composed, its mean within the statement's own
    figure of 2/R."""
    import curvature_ref as C
    from test_sample_points_cpu import KAPPA_FIGURE, chain_case

    phi, dx, lo, nodes, radius = chain_case()
    n = tuple(v - 1 for v in phi.shape)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    home = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    p = mk(phi)
    sX, sE, sinfo = lsf.extractSurface(p, *n, dx, lo)
    assert _bits(home(sX), nodes)  # the nodes of the extraction statement
    lin = lsf.samplePoints(p, *n, dx, lo, sX, order="linear")
    bound, axis_edge = S.node_value_bound(phi, dx, lo, nodes)
    err = np.abs(home(lin.val))
    print(f"largest |val - iso|: {err[axis_edge].max():.3g} on axis edges (bound {bound[axis_edge].max():.3g}), "
          f"{err[~axis_edge].max():.3g} on diagonals (bound {bound[~axis_edge].max():.3g})")
    assert lin.info[0] == len(nodes) and np.all(err <= bound)
    mask = np.asfortranarray((np.abs(phi) < 4.1 * dx).astype(np.int32))
    m, k = mk(mask), mk(np.full(phi.shape, np.nan, order="F"))
    lsf.curvatureBand(p, m, *n, dx, k)
    rep = lsf.samplePoints(p, *n, dx, lo, sX, order="cubic", mask=m, q=k)
    kappa = C.curvature_band(phi, mask, dx, np.full(phi.shape, np.nan, order="F")).kappa
    want = S.sample_points(phi, dx, lo, nodes, order=S.CUBIC, mask=mask, q=kappa)
    assert rep.info[2] == 0 and list(rep.info) == want.info and _bits(home(rep.qval), want.qval)
    mean = float(home(rep.qval).mean())
    print(f"mean kappa at the nodes {mean!r}, 2/R {2 / radius!r}")
    assert abs(mean / (2.0 / radius) - 1.0) <= KAPPA_FIGURE


# ---------------------------------------------------------------------------------- 6: errors
@pytest.mark.parametrize("seam", ["host", "device"])
def test_invalid_arguments_leave_everything_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    _lib.check(lib.lsf_set_device(0))
    phi0, mask0, q0 = _fields()
    npts = 65
    pts0 = _points(npts, True)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    phi, mask, q, pts = mk(phi0), mk(mask0), mk(q0), mk(pts0)
    outs = _fresh_outs(seam, npts)
    ok = dict(phi=phi, mask=mask, q=q, n=N, dx=DX, lo=LO, pts=pts, npts=npts, order=S.CUBIC, iso=ISO, iters=ITERS, tol=TOL, outs=outs)
    nan, inf = float("nan"), float("inf")

    def swap(**kw):
        return dict(outs=dict(outs, **kw))

    def part(t, a, b):
        """entries a .. b of a float64 array as an array of its own (a view: the same bytes)"""
        return t[a:b]

    cases = {
        "NULL phi": dict(phi=None), "NULL pts": dict(pts=None), "NULL val": swap(val=None), "NULL xLo": dict(lo=None),
        "npts = 0": dict(npts=0), "npts < 0": dict(npts=-3),
        "nx = 0": dict(n=(0, N[1], N[2])), "nz < 0": dict(n=(N[0], N[1], -1)), "too many points": dict(n=(2047, 2047, 511)),
        "dx = 0": dict(dx=0.0), "dx < 0": dict(dx=-DX), "dx NaN": dict(dx=nan), "dx inf": dict(dx=inf),
        "xLo NaN": dict(lo=(LO[0], nan, LO[2])), "xLo inf": dict(lo=(inf, LO[1], LO[2])),
        "iso NaN": dict(iso=nan), "iso inf": dict(iso=-inf),
        "order 2": dict(order=2), "order -1": dict(order=-1),
        "iters < 0": dict(iters=-1),
        "tol < 0": dict(tol=-1e-6), "tol NaN": dict(tol=nan), "tol inf": dict(tol=inf),
        "qval without q": dict(q=None),
        "foot with iters == 0": dict(iters=0),
        "val is phi": swap(val=phi), "grad is q": swap(grad=q), "status is mask": swap(status=mask), "foot is pts": swap(foot=pts),
        "qval is val": swap(qval=outs["val"]), "foot is grad": swap(foot=outs["grad"]),
        "val inside grad": swap(val=part(outs["grad"], npts, 2 * npts)), "qval is the tail of foot": swap(qval=part(outs["foot"], 2 * npts, 3 * npts)),
        "val is the tail of pts": swap(val=part(pts, 2 * npts + 1, 3 * npts)),
    }
    for name, change in cases.items():
        rc, info, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg.startswith("lsf_sample_points: ") and info == [-7] * 6, (name, msg)  # nothing reported
        for k, v in outs.items():
            assert np.all(back(v) == SENT), (name, k)  # nothing written
        assert _bits(back(phi), phi0.ravel(order="F")) and np.array_equal(back(mask), mask0.ravel(order="F")), name
        assert _bits(back(q), q0.ravel(order="F")) and _bits(back(pts), pts0.ravel(order="F")), name
    # tol is not looked at without a projection, and a valid call follows the refusals
    valid = dict(ok, iters=0, tol=nan, outs={k: v for k, v in outs.items() if k != "foot"})
    rc, info, msg = _raw(lib, seam, **valid)
    assert rc == 0, msg
    _assert_equal(_home(seam, valid["outs"], npts), info, _want(S.CUBIC, True, True, 0, npts), "after the refusals")
    # a non-finite phi or q VALUE is no error: it flows into the outputs
    bad_phi, bad_q = phi0.copy(order="F"), q0.copy(order="F")
    bad_phi[6, 4, 3], bad_q[5, 5, 3] = nan, inf
    want = S.sample_points(bad_phi, DX, LO, pts0, order=S.CUBIC, mask=mask0, q=bad_q, iso=ISO, iters=ITERS, tol=TOL)
    assert np.isnan(want.val[want.status != S.OFFBAND]).any() and np.isinf(want.qval).any()
    outs2 = _fresh_outs(seam, npts)
    rc, info, msg = _raw(lib, seam, **dict(ok, phi=mk(bad_phi), q=mk(bad_q), outs=outs2))
    assert rc == 0, msg
    _assert_equal(_home(seam, outs2, npts), info, want, "non-finite values")


def test_a_refused_call_leaves_an_unsynced_phi_twin_intact(lsf):
    """Under LSF_MIRROR_TRUST | LSF_MIRROR_LAZY a reinit leaves its result in phi's device twin and the host array stale.  A valid
    samplePoints reads the twin; a refused one touches nothing; the sync then brings the reinit's result home."""
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi0, mask0, q0 = _fields()
    pts = _points(256, False)
    h = 0.3 * DX
    dev = _dev(phi0)
    lsf.reinit(dev, None, None, *N, 2, DX, h, tol=0.0, order="jacobi", arith="fast")
    moved = dev.cpu().numpy().reshape(SHAPE, order="F")
    assert not np.array_equal(moved, phi0)
    want = S.sample_points(moved, DX, LO, pts, order=S.CUBIC, iso=ISO, iters=ITERS, tol=TOL)
    try:
        _lib.check(lib.lsf_mirror(3))  # LSF_MIRROR_TRUST | LSF_MIRROR_LAZY
        P = phi0.copy(order="F")
        lsf.reinit(P, None, None, *N, 2, DX, h, tol=0.0, order="jacobi", arith="fast")
        assert _bits(P, phi0)  # un-synced: the host copy is what it was
        rep = lsf.samplePoints(P, *N, DX, LO, pts, order="cubic", iso=ISO, iters=ITERS, tol=TOL)
        _assert_equal({k: getattr(rep, k) for k in ("val", "grad", "foot", "status")}, list(rep.info), want, "from the twin")
        assert _bits(P, phi0)  # phi is an input only: still not home
        for kw in (dict(order=9), dict(iso=float("nan")), dict(dx=-1.0)):
            outs = _fresh_outs("host", 256, ["val", "grad", "foot", "status"])
            a = dict(dict(phi=P, mask=None, q=None, n=N, dx=DX, lo=LO, pts=np.array(pts.ravel(order="F")), npts=256,
                          order=S.CUBIC, iso=ISO, iters=ITERS, tol=TOL, outs=outs), **kw)
            rc, info, msg = _raw(lib, "host", **a)
            assert rc == _lib.LSF_ERR_INVALID and info == [-7] * 6 and all(np.all(v == SENT) for v in outs.values()), (kw, msg)
            assert _bits(P, phi0)
        _lib.check(lib.lsf_mirror_sync(P.ctypes.data))
        assert _bits(P, moved)  # the earlier un-synced result, intact
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())


# ---------------------------------------------------------------------------------- 7: the Fortran shim
EXE = os.path.join(ROOT, "build", "dropin", "host_sample.exec")


@pytest.fixture(scope="module")
def host_sample_exe():
    path = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    if not os.path.exists(EXE):
        fc = shutil.which("amdflang", path=path)
        if fc is None:
            pytest.skip("no amdflang: tests/fortran/host_sample.f90 cannot be built")
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetfortran_amd", "fortran"), "sample", f"FC={fc}"], env=dict(os.environ, PATH=path),
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and os.path.exists(EXE), p.stdout[-3000:]
    return EXE


@pytest.mark.parametrize("resident", ["0", "2"])
def test_sample_points_through_the_fortran_wrapper(lsf, host_sample_exe, tmp_path, resident):
    """tests/fortran/host_sample.f90: samplePoints of lsf_hip.f90 with a mask and q gives the statement's bits and prints its counts"""
    phi, mask, q = _fields()
    npts = 256
    pts = _points(npts, True)
    want = _want(S.CUBIC, True, True, ITERS, npts)
    with open(tmp_path / "sample_in.bin", "wb") as f:
        f.write(np.array([*N, npts, S.CUBIC, ITERS], np.int32).tobytes())
        f.write(np.array([DX, *LO, ISO, TOL], np.float64).tobytes())
        for a in (phi, mask, q, pts):
            f.write(a.tobytes(order="F"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSF_")}
    env.update(LSF_RESIDENT=resident)
    p = subprocess.run(f"ulimit -s unlimited; cd {tmp_path}; {host_sample_exe}", shell=True, env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    print(p.stdout)
    raw = open(tmp_path / "sample_out.bin", "rb").read()
    assert len(raw) == npts * (8 * 8 + 4)
    d = np.frombuffer(raw, np.float64, 8 * npts)
    got = {"val": d[:npts], "grad": d[npts:4 * npts].reshape((npts, 3), order="F"), "qval": d[4 * npts:5 * npts],
           "foot": d[5 * npts:].reshape((npts, 3), order="F"), "status": np.frombuffer(raw, np.int32, npts, 64 * npts)}
    _assert_equal(got, want.info, want, "Fortran")
    import re

    line = " ".join(p.stdout.split())
    nums = [int(v) for v in re.findall(r"(?:points|ok|outside|off the band|linear fallbacks|flat|not converged)\s+(\d+)", line)]
    assert nums == [npts, *want.info], (nums, want.info)
