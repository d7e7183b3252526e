"""lsf_extend_field_band on the GPU against tests/extend_band_ref.py, the serial statement of the contract in include/lsf.h: the
whole q array -- bit pattern by bit pattern -- passes, trace and info are compared with `==`, on both seams, in band form and in
`known` form, at max_passes 1, 3 and 256.

Cases (extend_band_ref.inputs), the smallest on which each piece can go wrong (a chunk is 256 list entries, MB_CH in
csrc/lsf_minmax_band.hpp; the host reads the counts of 8 passes at a time, CHECK_EVERY in csrc/lsf_api.hip):
  small     (10,10,10), |phi| < 2.1 dx: 246 cells -- one ragged chunk; 4 passes
  general   (40,33,27), |phi| < 4.1 dx: 6 170 cells, 25 chunks, the last ragged; 12 passes: the stop falls inside the second batch
  onecell   a list of one frozen cell and one neighbour
  values    (12,11,10): a mask carrying 0, 7, -1 and 1s on wall points
  interior  (25,25,25), every interior point: chosen neighbours on all six walls (never in the list); 30 passes, four batches
  onesided  general with `known` on the side phi > 0 only: 136 cells stay NaN
  stop8     general with |phi| < 2.6 dx: 3 850 cells; 8 passes: the stop is the last pass of the first batch
  stop9     general with |phi| < 3.1 dx: 4 612 cells; 9 passes: the stop is the first pass of the second batch
The edges of a batch: "interior" and "general" at max_passes 7, 8, 9, 16 and 17, and stop8 / stop9 uncapped and capped at their stop."""
import ctypes
import functools

import numpy as np
import pytest

import advect_band_ref as B
import curvature_ref as C
import extend_band_ref as X

pytestmark = pytest.mark.gpu

CHUNK, CHECK_EVERY = 256, 8
RUNS = [(c, f) for c in ("small", "general", "onecell", "values", "interior") for f in X.FORMS] + [("onesided", "known")]
CAPS = [1, 3, 256]
SEAMS = ["host", "device"]
# the edges of a batch: caps next to the multiples of CHECK_EVERY, and natural stops on the last pass of a batch and the first of the next
EDGE_RUNS = [(c, f, cap) for c, f in (("interior", "band"), ("general", "band"), ("general", "known")) for cap in (7, 8, 9, 16, 17)]
EDGE_RUNS += [("stop8", "band", 256), ("stop8", "band", 8), ("stop9", "band", 256), ("stop9", "band", 9)]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


def test_the_cases_are_what_the_docstring_says():
    assert X.want("small", "band").info[:2] == [246, 104] and 246 < CHUNK and X.want("small", "band").passes == 4
    g = X.want("general", "band")
    assert g.cells == 6170 and (g.cells + CHUNK - 1) // CHUNK == 25 and g.cells % CHUNK and CHECK_EVERY < g.passes == 12 < 2 * CHECK_EVERY
    assert X.want("onecell", "band").info == [2, 1, 1, 0] and X.want("onecell", "band").trace == [1, 0]
    mask = X.inputs("values")[2]
    inner = mask[1:-1, 1:-1, 1:-1]
    assert (inner == 0).any() and (inner == 7).any() and (inner == -1).any() and B.list_of(mask).sum() < mask[mask == 1].size
    assert X.want("interior", "band").passes == 30 > 3 * CHECK_EVERY and X.want("interior", "band").cells == 23 ** 3
    assert X.want("onesided", "known").unreached == 136
    s8, s9 = X.want("stop8", "band"), X.want("stop9", "band")
    assert (s8.cells, s8.passes, s8.trace[-2:]) == (3850, CHECK_EVERY, [6, 0]) and (s9.cells, s9.passes, s9.trace[-2:]) == (4612, CHECK_EVERY + 1, [24, 0])
    for case, form in RUNS + [("stop8", "band"), ("stop9", "band")]:
        q, phi, mask, known, dx, band = X.inputs(case)
        lst = B.list_of(mask)
        assert X.check(q, phi, mask, dx, band=band, known=known if form == "known" else None)[2:] == (0, 0)
        assert np.all(known[~lst] == 1) and np.isnan(q[~lst]).any() and (q[~lst] == -7.0).any()


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda().reshape(a.shape[::-1])  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(-1).reshape(shape, order="F")


def _bits(a, b):
    """bit for bit, NaN payloads and the sign of zero included"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _run(lsf, seam, case, form, cap, stream=None):
    """extendFieldBand on fresh copies through one seam; returns (q as a numpy array, report); asserts that the inputs are unchanged"""
    import torch

    q0, phi0, mask0, known0, dx, band = X.inputs(case)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t, ref: _host(t, ref.shape)) if seam == "device" else (lambda t, ref: t)
    q, phi, mask = mk(q0), mk(phi0), mk(mask0)
    known = mk(known0) if form == "known" else None
    kw = dict(known=known) if form == "known" else dict(band=band)
    try:
        if stream is not None:
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                out, rep = lsf.extendFieldBand(q, phi, mask, dx, max_passes=cap, **kw)
            torch.cuda.synchronize()
        else:
            out, rep = lsf.extendFieldBand(q, phi, mask, dx, max_passes=cap, **kw)
        assert out is q
    finally:
        assert _bits(back(phi, phi0), phi0) and np.array_equal(back(mask, mask0), mask0)  # read, never written
        assert known is None or np.array_equal(back(known, known0), known0)
    return back(q, q0), rep


def _assert_equal(got, rep, want, cap):
    assert _bits(got, want.field), int(np.count_nonzero(got.view(np.int64) != want.field.view(np.int64)))
    assert (rep.passes, rep.trace) == (want.passes, want.trace)
    assert [rep.cells, rep.frozen, rep.reached, rep.unreached] == want.info
    assert rep.converged == want.converged == (want.trace[-1] == 0)


# ---------------------------------------------------------------------------------- 1: == the statement, after every number of passes
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("case,form", RUNS)
def test_bit_identical_to_the_statement(lsf, case, form, cap, seam):
    want = X.want(case, form, cap)
    got, rep = _run(lsf, seam, case, form, cap)
    print(f"{case} {form} cap {cap} {seam}: {rep.passes} passes, trace {rep.trace}, info {[rep.cells, rep.frozen, rep.reached, rep.unreached]}; "
          f"want {want.passes}, {want.trace}, {want.info}; q differs at {int(np.count_nonzero(got.view(np.int64) != want.field.view(np.int64)))} points")
    _assert_equal(got, rep, want, cap)
    q0, mask = X.inputs(case)[0], X.inputs(case)[2]
    lst = B.list_of(mask)
    assert _bits(got[~lst], q0[~lst])  # off the list: the caller's bits
    assert int(np.isnan(got[lst]).sum()) == want.unreached


@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("case,form,cap", EDGE_RUNS)
def test_batch_edges_bit_identical_to_the_statement(lsf, case, form, cap, seam):
    """a cap or a stop on the last pass of a batch of CHECK_EVERY, or on the first pass of the next"""
    want = X.want(case, form, cap)
    got, rep = _run(lsf, seam, case, form, cap)
    print(f"{case} {form} cap {cap} {seam}: {rep.passes} passes, trace {rep.trace}; want {want.passes}, {want.trace}; "
          f"q differs at {int(np.count_nonzero(got.view(np.int64) != want.field.view(np.int64)))} points")
    assert want.passes == min(cap, X.want(case, form).passes)
    _assert_equal(got, rep, want, cap)


# ---------------------------------------------------------------------------------- 2: streams, run to run
@pytest.mark.parametrize("form", X.FORMS)
def test_side_stream_and_run_to_run(lsf, form):
    import torch

    want = X.want("general", form)
    for _ in range(2):  # the second run of a call equals the first
        got, rep = _run(lsf, "device", "general", form, 256, stream=torch.cuda.Stream())
        _assert_equal(got, rep, want, 256)


# ---------------------------------------------------------------------------------- 3: errors
def _raw(lib, seam, q, phi, mask, known, n, dx, band, max_passes=256, trace_cap=4):
    info = np.full(4, -7, np.int64)
    trace = np.full(4, -7, np.int64)
    done = ctypes.c_int(-7)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(q), ptr(phi), ptr(mask), ptr(known), n[0], n[1], n[2], dx, band, max_passes, ctypes.byref(done), trace.ctypes.data, trace_cap,
            info.ctypes.data)
    rc = lib.lsf_extend_field_band_device(*args, None) if seam == "device" else lib.lsf_extend_field_band(*args)
    return rc, list(info), list(trace), done.value, (lib.lsf_last_error() or b"").decode()


@pytest.mark.parametrize("seam", SEAMS)
def test_invalid_arguments_leave_everything_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    q0, phi0, mask0, known0, dx, band = X.inputs("values")
    npts = phi0.shape
    n = tuple(v - 1 for v in npts)
    lst = B.list_of(mask0)
    fz = X.frozen_of(phi0, lst, dx, band)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t: _host(t, npts)) if seam == "device" else (lambda t: t)

    def changed(a, cell, value):
        b = a.copy(order="F")
        b[cell] = value
        return mk(b)

    cell = tuple(np.argwhere(lst & ~fz)[5])  # a non-frozen list cell with all six neighbours inside the field
    six = sum(int(lst[tuple(np.add(cell, d))]) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
    frozen_cells = np.argwhere(fz)
    walls = np.zeros(npts, np.int32, order="F")
    walls[0, :, :], walls[:, -1, :] = 1, 1
    q, phi, mask, known = mk(q0), mk(phi0), mk(mask0), mk(known0)
    ok = dict(q=q, phi=phi, mask=mask, known=None, n=n, dx=dx, band=band)
    badq = q0.copy(order="F")
    badq[tuple(frozen_cells[0])], badq[tuple(frozen_cells[-1])] = np.nan, np.inf
    cases = {
        "NULL q": (dict(q=None), ""),
        "NULL phi": (dict(phi=None), ""),
        "NULL mask": (dict(mask=None), ""),
        "nx < 2": (dict(n=(1, n[1], n[2])), ""),
        "nz < 2": (dict(n=(n[0], n[1], 0)), ""),
        "dx = 0": (dict(dx=0.0), ""),
        "dx < 0": (dict(dx=-dx), ""),
        "dx NaN": (dict(dx=float("nan")), ""),
        "dx inf": (dict(dx=float("inf")), ""),
        "band = 0": (dict(band=0.0), ""),
        "band < 0": (dict(band=-1.0), ""),
        "band NaN": (dict(band=float("nan")), ""),
        "band inf": (dict(band=float("inf")), ""),
        "max_passes < 1": (dict(max_passes=0), ""),
        "trace_cap < 0": (dict(trace_cap=-1), ""),
        "q is phi": (dict(q=phi), "overlaps"),
        "empty list": (dict(mask=mk(walls)), "empty"),
        "no frozen cell (band)": (dict(band=1e-9), "no frozen"),
        "no frozen cell (known)": (dict(known=mk(np.asfortranarray(np.where(lst, 0, 1).astype(np.int32)))), "no frozen"),
        "non-finite frozen q": (dict(q=mk(badq)), ": 2 frozen cell"),
        "NaN phi": (dict(phi=changed(phi0, cell, np.nan)), f": {1 + six} list cell"),
        "inf phi next to the list": (dict(phi=changed(phi0, cell, np.inf), known=known), f": {1 + six} list cell"),
    }
    for name, (change, word) in cases.items():
        args = dict(ok, **change)
        before = None if args["q"] is None else back(args["q"]).copy()
        rc, info, trace, done, msg = _raw(lib, seam, **args)
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and word in msg, (name, msg)
        assert info == [-7] * 4 and trace == [-7] * 4 and done == -7, name  # nothing reported
        assert before is None or _bits(back(args["q"]), before), name  # nothing written
        assert _bits(back(phi), phi0) and np.array_equal(back(mask), mask0), name
    # with `known` the band is ignored, whatever it holds
    want = X.want("values", "known")
    for b in (0.0, float("nan")):
        qq = mk(q0)
        rc, info, trace, done, _ = _raw(lib, seam, qq, phi, mask, known, n, dx, b)
        assert rc == 0 and info == want.info and done == want.passes and trace[:done] == want.trace[:4] and _bits(back(qq), want.field)
    # a valid call follows: the library is in working order, and the Python layer raises the same error
    rc, info, trace, done, _ = _raw(lib, seam, **ok)
    want = X.want("values", "band")
    assert rc == 0 and info == want.info and done == want.passes == 3 and trace == want.trace + [-7] and _bits(back(q), want.field)
    with pytest.raises(lsf.LsfError) as e:
        lsf.extendFieldBand(mk(q0), phi, mk(walls), dx, band=band)
    assert e.value.code == _lib.LSF_ERR_INVALID and "empty" in str(e.value)


# ---------------------------------------------------------------------------------- 4: curvature -> extension -> transport on one mask
@functools.lru_cache(maxsize=None)
def _composition_want():
    _, phi, mask, _, dx, _ = X.inputs("general")
    npts = phi.shape
    lst = B.list_of(mask)
    kappa = C.curvature_band(phi, mask, dx, np.full(npts, np.nan, order="F"), clamp=1.0).kappa
    assert np.isnan(kappa[~lst]).all() and np.isfinite(kappa[lst]).all()
    known = np.asfortranarray((np.abs(phi) < 1.5 * dx).astype(np.int32))
    ext = X.extend_band(-kappa, phi, mask, dx, known=known)
    assert ext.converged and ext.unreached == 0 and np.isnan(ext.field[~lst]).all()
    dt = 0.25 * dx * dx  # |speed| <= 1/dx: CFL <= 0.25
    adv = B.advect_band(phi, mask, None, ext.field, dx, dt, 2, "rk3")
    assert adv.steps == 2 and 0 < adv.cfl <= 0.25 and not adv.nan
    return known, ext, adv, dt


@pytest.mark.parametrize("seam", SEAMS)
def test_curvature_extension_transport_on_one_mask(lsf, seam):
    """kappa on the cells of a mask, NaN elsewhere; F = -kappa kept on the cells next to the surface and carried to every other list
    cell; the surface moved by it for 2 RK3 steps in STRICT arithmetic: equal to the three statements composed."""
    _, phi0, mask0, _, dx, _ = X.inputs("general")
    npts = phi0.shape
    nx, ny, nz = (v - 1 for v in npts)
    known0, ext, adv, dt = _composition_want()
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t: _host(t, npts)) if seam == "device" else (lambda t: t)
    phi, mask, known, kappa = mk(phi0), mk(mask0), mk(known0), mk(np.full(npts, np.nan, order="F"))
    lsf.curvatureBand(phi, mask, nx, ny, nz, dx, kappa, clamp=1.0)
    speed = -kappa  # a fresh array of the same kind, NaN off the list
    _, rep = lsf.extendFieldBand(speed, phi, mask, dx, known=known)
    assert (rep.passes, rep.trace, [rep.cells, rep.frozen, rep.reached, rep.unreached]) == (ext.passes, ext.trace, ext.info) and rep.converged
    assert _bits(back(speed), ext.field)
    arep = lsf.advectFieldBand(phi, mask, nx, ny, nz, dx, dt, 2, speed=speed, arith="strict")
    assert arep.steps == 2 and arep.cfl == adv.cfl and arep.change == adv.change
    assert np.array_equal(back(phi), adv.field) and not np.array_equal(back(phi)[B.list_of(mask0)], phi0[B.list_of(mask0)])
