"""lsf_correct_field on the GPU against tests/points_ref.py, the numpy statement of the contract in include/lsf.h, on both seams: phi
whole, status, change and info are compared with `==` on the bit patterns, NaNs by position.

Grid and mask: tests/points_inputs.py (12 x 9 x 7 cells, dx = 0.125; holes 0, 7 and -1, 1s on the walls).  phi is the sphere field with a
NaN at one grid point and -0.0 at another; the markers are seeded by the statement's rule from the sphere shifted by 0.8 dx, so that
between a tenth and a half of them escape (asserted on the statement first), with rad 0, NaN and +-inf, the special points of
tests/sample_ref.py and a marker whose candidate at the -0.0 is +0.0 planted among them (points_inputs.correct_inputs).  Then the
Fortran program, and the chain: the vortex configuration of tests/test_points_cpu.py through the public Python calls on the device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import points_inputs as I
import points_ref as P
from conftest import ROOT

pytestmark = pytest.mark.gpu

N = tuple(s - 1 for s in I.SHAPE)
SENT = -7


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


def _raw(lib, seam, phi, mask, n, dx, lo, pts, rad, npts, slack, status, want_change=True, want_info=True, stream=None):
    """the C call; phi, mask, pts, rad and status are numpy arrays (host seam), torch tensors (device seam) or None:
    (rc, change, info, message)"""
    inf = np.full(P.CORRECT_INFO_LEN, SENT, np.int64)
    change = ctypes.c_double(float(SENT))
    lo = None if lo is None else np.array(lo, dtype=np.float64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), n[0], n[1], n[2], dx, None if lo is None else lo.ctypes.data, ptr(pts), ptr(rad), npts, slack, ptr(status),
            ctypes.byref(change) if want_change else None, inf.ctypes.data if want_info else None)
    rc = lib.lsf_correct_field_device(*args, stream) if seam == "device" else lib.lsf_correct_field(*args)
    return rc, change.value, [int(v) for v in inf], (lib.lsf_last_error() or b"").decode()


def _run(seam, masked, slack, order=None, with_status=True, want_change=True, want_info=True, stream=None):
    """one call through one seam on fresh copies, the particles in the order `order`: (phi at home, status or None, change, info);
    asserts LSF_OK and that the inputs are unchanged"""
    import torch
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    phi, pts, rad = I.correct_inputs()
    mask = I.small_fields()[5]
    if order is not None:
        pts, rad = np.asfortranarray(pts[order]), rad[order]
    npts = len(rad)
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    p, m, x, r = mk(phi), mk(mask) if masked else None, mk(pts), mk(rad)
    status = mk(np.full(npts, SENT, np.int32)) if with_status else None
    if seam == "device":
        _lib.check(lib.lsf_set_device(0))
        torch.cuda.synchronize()
    rc, change, info, msg = _raw(lib, seam, p, m, N, I.DX, I.LO, x, r, npts, slack, status, want_change, want_info,
                                 None if stream is None else stream.cuda_stream)
    assert rc == 0, msg
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert _bits(back(x), pts.ravel(order="F")) and _bits(back(r), rad) and (m is None or np.array_equal(back(m), mask.ravel(order="F")))
    return back(p).reshape(I.SHAPE, order="F"), None if status is None else back(status), change, info


def _assert_equal(got, want, what):
    phi, status, change, info = got
    print(f"{what}: phi differs at {int(np.count_nonzero(~((phi == want.phi) | (np.isnan(phi) & np.isnan(want.phi)))))} points, "
          f"change {change!r} want {want.change!r}, info {info} want {want.info}")
    assert _bits(phi, want.phi), what
    assert np.array_equal(np.signbit(phi), np.signbit(want.phi)), what
    if status is not None:
        assert np.array_equal(status, want.status), what
    assert np.float64(change).view(np.uint64) == np.float64(want.change).view(np.uint64), what
    assert info == want.info, what


def test_the_inputs_are_what_the_docstring_says():
    phi, pts, rad = I.correct_inputs()
    assert len(rad) > 2 * 256 and np.isnan(phi).sum() == 1 and np.signbit(phi[I.ZERO_AT]) and phi[I.ZERO_AT] == 0.0
    for masked in (False, True):
        for slack in (0.0, 1.0):
            w = I.correct_want(masked, slack)
            assert 0.1 * len(rad) <= w.info[1] <= 0.5 * len(rad), w.info  # between a tenth and a half escape
            assert w.info[2] >= 18 and w.info[4] > 0 and w.info[5] == 4 and (w.info[3] > 0) == masked and sum(w.info[:6]) == len(rad)
            assert w.status[60] == P.ESCAPED and w.phi[I.ZERO_AT] == 0.0 and not np.signbit(w.phi[I.ZERO_AT])  # +0.0 beat -0.0
            assert np.isnan(w.phi[I.NAN_AT]) and w.info[6] > 0 and w.change > 0.0


# ---------------------------------------------------------------------------------- 1: mask x slack x seam
@pytest.mark.parametrize("seam", ["host", "device"])
@pytest.mark.parametrize("slack", [0.0, 1.0])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_every_output_equals_the_statement(lsf, masked, slack, seam):
    import torch

    want = I.correct_want(masked, slack)
    got = _run(seam, masked, slack)
    _assert_equal(got, want, seam)
    if masked:  # nothing is written off the list
        phi0 = I.correct_inputs()[0]
        mask = I.small_fields()[5]
        lst = np.zeros(I.SHAPE, bool)
        lst[1:-1, 1:-1, 1:-1] = mask[1:-1, 1:-1, 1:-1] == 1
        assert _bits(got[0][~lst], phi0[~lst])
    if seam == "device":
        _assert_equal(_run(seam, masked, slack, stream=torch.cuda.Stream()), want, "side stream")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_reversed_particles_give_the_same_bits(lsf, masked):
    """two device runs with the particles in reversed order are bit-identical: maxima and minima of integers"""
    n = len(I.correct_inputs()[2])
    a = _run("device", masked, 1.0)
    b = _run("device", masked, 1.0, order=np.arange(n)[::-1])
    assert _bits(a[0], b[0]) and np.array_equal(np.signbit(a[0]), np.signbit(b[0])) and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[1][::-1], b[1])
    _assert_equal(a, I.correct_want(masked, 1.0), "forward")


@pytest.mark.parametrize("seam", ["host", "device"])
def test_optional_outputs_may_be_null_one_at_a_time(lsf, seam):
    want = I.correct_want(True, 1.0)
    got = _run(seam, True, 1.0, with_status=False)
    assert got[1] is None
    _assert_equal(got, want, "without status")
    phi, status, change, info = _run(seam, True, 1.0, want_change=False)
    assert change == float(SENT)
    _assert_equal((phi, status, want.change, info), want, "without change")
    phi, status, change, info = _run(seam, True, 1.0, want_info=False)
    assert info == [SENT] * P.CORRECT_INFO_LEN
    _assert_equal((phi, status, change, want.info), want, "without info")


# ---------------------------------------------------------------------------------- 2: refusals
@pytest.mark.parametrize("seam", ["host", "device"])
def test_invalid_arguments_write_nothing(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    mk = _dev if seam == "device" else (lambda a: np.array(a.ravel(order="F")))
    back = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    phi0, pts0, rad0 = I.correct_inputs()
    mask = I.small_fields()[5]
    npts = len(rad0)
    base = dict(n=N, dx=I.DX, lo=I.LO, npts=npts, slack=1.0)
    nan, inf = float("nan"), float("inf")
    bad = [("phi NULL", dict(null="phi")), ("pts NULL", dict(null="pts")), ("rad NULL", dict(null="rad")), ("xLo NULL", dict(lo=None)),
           ("npts 0", dict(npts=0)), ("nz 0", dict(n=(N[0], N[1], 0))), ("dx 0", dict(dx=0.0)), ("dx inf", dict(dx=inf)),
           ("xLo NaN", dict(lo=(nan, 0.0, 0.0))), ("slack < 0", dict(slack=-0.5)), ("slack NaN", dict(slack=nan)), ("slack inf", dict(slack=inf)),
           ("status is rad", dict(alias="status=rad")), ("status is phi", dict(alias="status=phi")), ("phi is pts", dict(alias="phi=pts"))]
    for name, ch in bad:
        a = dict(phi=mk(phi0), mask=mk(mask), pts=mk(pts0), rad=mk(rad0), status=mk(np.full(npts, SENT, np.int32)))
        kw = dict(base, **{k: v for k, v in ch.items() if k in base})
        use = dict(a)
        if "null" in ch:
            use[ch["null"]] = None
        if "alias" in ch:
            dst, src = ch["alias"].split("=")
            use[dst] = a[src]
        rc, change, info, msg = _raw(lib, seam, use["phi"], use["mask"], kw["n"], kw["dx"], kw["lo"], use["pts"], use["rad"], kw["npts"], kw["slack"],
                                     use["status"])
        assert rc == _lib.LSF_ERR_INVALID and msg.startswith("lsf_correct_field: "), (name, rc, msg)
        assert _bits(back(a["phi"]), phi0.ravel(order="F")) and np.all(back(a["status"]) == SENT) and change == float(SENT), name
        assert info == [SENT] * P.CORRECT_INFO_LEN and _bits(back(a["pts"]), pts0.ravel(order="F")) and _bits(back(a["rad"]), rad0), name
    _assert_equal(_run(seam, True, 0.0), I.correct_want(True, 0.0), "after the refusals")  # ... then a valid call


# ---------------------------------------------------------------------------------- 3: the Python report and the seeding helper
@pytest.mark.parametrize("seam", ["host", "device"])
def test_python_report(lsf, seam):
    import torch

    phi0, pts0, rad0 = I.correct_inputs()
    mask0 = I.small_fields()[5]
    want = I.correct_want(True, 1.0)
    if seam == "device":
        phi, mask, rad = _dev(phi0), _dev(mask0), torch.from_numpy(rad0.copy()).cuda()
        pts = torch.from_numpy(np.array(pts0.T, order="C")).cuda().t()
    else:
        phi, mask, pts, rad = np.array(phi0, order="F"), np.array(mask0, order="F"), np.array(pts0, order="F"), rad0.copy()
    rep = lsf.correctField(phi, *N, I.DX, I.LO, pts, rad, mask=mask, slack=1.0)
    home = (lambda t: t.cpu().numpy()) if seam == "device" else (lambda t: t)
    assert isinstance(rep, lsf.CorrectReport) and rep.info == tuple(want.info) and rep.change == want.change
    assert np.array_equal(home(rep.status), want.status) and _bits(home(phi).reshape(I.SHAPE, order="F"), want.phi)


def test_seed_particles_is_the_statements_rule(lsf):
    """seedParticles samples through the library: the same points and radii as the statement's rule, with and without the mask"""
    phi = np.array(I.small_fields()[0], order="F")
    mask = np.array(I.small_fields()[5], order="F")
    for m in (None, mask):
        pts, rad = lsf.seedParticles(phi, *N, I.DX, I.LO, mask=m, per_cell=4, seed=11)
        wp, wr = P.seed_particles(phi, I.DX, I.LO, mask=m, per_cell=4, seed=11)
        assert len(rad) > 100 and pts.flags.f_contiguous and _bits(pts, wp) and _bits(rad, wr)
        assert np.all(np.abs(rad) >= 0.1 * I.DX) and np.all(np.abs(rad) <= 0.5 * I.DX)


# ---------------------------------------------------------------------------------- 4: the Fortran shim
EXE = os.path.join(ROOT, "build", "dropin", "host_particles.exec")


@pytest.fixture(scope="module")
def host_particles_exe():
    path = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    if not os.path.exists(EXE):
        fc = shutil.which("amdflang", path=path)
        if fc is None:
            pytest.skip("no amdflang: tests/fortran/host_particles.f90 cannot be built")
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetfortran_amd", "fortran"), "particles", f"FC={fc}"],
                           env=dict(os.environ, PATH=path), text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and os.path.exists(EXE), p.stdout[-3000:]
    return EXE


@pytest.mark.parametrize("resident", ["0", "2"])
def test_both_calls_through_the_fortran_wrappers(lsf, host_particles_exe, tmp_path, resident):
    """tests/fortran/host_particles.f90: correctField, then advectPoints through the corrected phi, give the statement's bits"""
    phi0, pts0, rad0 = I.correct_inputs()
    _, u, v, w, f, mask = I.small_fields()
    npts = len(rad0)
    dt, nsteps, slack = 0.4 * I.DX, 3, 1.0
    wc = I.correct_want(True, slack)
    wa = P.advect_points(pts0, I.DX, I.LO, dt, nsteps, velocity=(u, v, w), speed=f, phi=wc.phi, mask=mask, order=P.CUBIC, scheme=P.RK3)
    with open(tmp_path / "particles_in.bin", "wb") as fh:
        fh.write(np.array([*N, npts, P.CUBIC, P.RK3, nsteps], np.int32).tobytes())
        fh.write(np.array([I.DX, *I.LO, dt, slack], np.float64).tobytes())
        for a in (phi0, u, v, w, f, mask, pts0, rad0):
            fh.write(a.tobytes(order="F"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSF_")}
    env.update(LSF_RESIDENT=resident)
    p = subprocess.run(f"ulimit -s unlimited; cd {tmp_path}; {host_particles_exe}", shell=True, env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    print(p.stdout)
    raw = open(tmp_path / "particles_out.bin", "rb").read()
    n = int(np.prod(I.SHAPE))
    assert len(raw) == 8 * n + 4 * npts + 8 + 24 * npts + 4 * npts + 8
    o = 0
    phi = np.frombuffer(raw, np.float64, n, o).reshape(I.SHAPE, order="F"); o += 8 * n
    cstatus = np.frombuffer(raw, np.int32, npts, o); o += 4 * npts
    change = np.frombuffer(raw, np.float64, 1, o)[0]; o += 8
    pts = np.frombuffer(raw, np.float64, 3 * npts, o).reshape((npts, 3), order="F"); o += 24 * npts
    astatus = np.frombuffer(raw, np.int32, npts, o); o += 4 * npts
    cfl = np.frombuffer(raw, np.float64, 1, o)[0]
    assert _bits(phi, wc.phi) and np.array_equal(cstatus, wc.status) and change == wc.change
    assert _bits(pts, wa.pts) and np.array_equal(astatus, wa.status) and cfl == wa.cfl
    import re

    line = " ".join(p.stdout.split())
    nums = [int(x) for x in re.findall(r"(?:markers|in place|escaped|outside|off the band|non-finite|bad radius|points changed)\s+(\d+)",
                                       line.split("Points:")[0])]
    assert nums == [npts, *wc.info], (nums, wc.info)


# ---------------------------------------------------------------------------------- 5: the chain
def test_the_vortex_chain_equals_the_statements_loop(lsf):
    """128 x (advectField STRICT, one step; advectPoints, one step, cubic; correctField) on the device seam through the public Python
    calls, the velocity negated after 64 steps, markers from seedParticles: phi, pts and every per-step info equal the statement's
    loop with `==`, both fed the same velocity arrays; measureBand of the end state lies within its summation bound of the
    statement's volume"""
    import torch

    import measure_ref as M

    want = I.vortex_run(True)  # (computed once per process)
    phi0, vel = I.vortex_fields()
    n = (I.VN - 1,) * 3
    pts, rad = lsf.seedParticles(np.array(phi0, order="F"), *n, I.VDX, I.VLO)
    wp, wr = P.seed_particles(phi0, I.VDX, I.VLO)
    assert _bits(pts, wp) and _bits(rad, wr)
    fwd = tuple(_dev(a) for a in vel)
    bwd = tuple(_dev(np.asfortranarray(-a)) for a in vel)
    phi = _dev(phi0)
    dpts = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda().t()
    drad = torch.from_numpy(rad.copy()).cuda()
    for step in range(2 * I.VSTEPS):
        V = fwd if step < I.VSTEPS else bwd
        lsf.advectField(phi, *n, I.VDX, I.VDT, 1, velocity=V, arith="strict")
        a = lsf.advectPoints(dpts, *n, I.VDX, I.VLO, I.VDT, 1, velocity=V, order="cubic", scheme="rk3")
        dpts = a.pts
        c = lsf.correctField(phi, *n, I.VDX, I.VLO, dpts, drad, slack=1.0)
        assert (a.info, c.info) == want["infos"][step], (step, a.info, c.info, want["infos"][step])
    got = phi.cpu().numpy().reshape(phi0.shape, order="F")
    assert _bits(got, want["phi"]) and _bits(dpts.cpu().numpy(), want["pts"])
    mask = torch.ones(phi.numel(), dtype=torch.int32, device=phi.device)
    rep = lsf.measureBand(phi, mask, *n, I.VDX, I.VLO)
    ref = M.measure_band(want["phi"], np.ones(phi0.shape, np.int32), I.VDX, I.VLO)
    bound = M.summation_bound(ref, 1)
    print(f"chain: volume {rep.volume!r}, the statement's {ref.M[1]!r}, |difference| {abs(rep.volume - ref.M[1]):.3g}, bound {bound:.3g}; "
          f"{want['escapes']} escapes used")
    assert abs(rep.volume - ref.M[1]) <= bound
