"""lsf_measure_band on the GPU against tests/measure_ref.py, the serial statement of the contract in include/lsf.h, on both seams:
cell_area -- the whole array, bit pattern by bit pattern -- and info are compared with `==`; each of the nine totals lies within
N * 2^-53 * sum|contribution| of math.fsum of the statement's per-cell contributions, N the crossed measured cells: the largest
distance any order of summation can have from the exact sum (measure_ref.summation_bound), derived and not measured.

Grids and masks, those of tests/test_gpu_curvature_band.py, the smallest on which each piece can go wrong (a chunk is 256 list
entries, MB_CH in csrc/lsf_minmax_band.hpp):
  small     (10,10,10), |phi| < 2.1 dx: 246 cells -- one ragged chunk
  general   (40,33,27), |phi| < 4.1 dx: about 6 000 cells, 25 chunks, the last ragged; x not a multiple of anything
  interior  (25,25,25), every interior point: cells whose upper corners are wall points
  onecell   a list of one cell of (10,10,10), all of it inside the sphere: uncrossed
  values    (12,11,10): a mask carrying 0, 7, -1 and 1s on wall points
  cut       (25,25,25), the half-space i < 13 through the sphere: an open piece, info[3] > 0
  zeros     (9,8,7), every interior point, phi = x - x[4]: phi == iso on the grid points of a plane, triangles of area 0.0"""
import functools
import math

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R
import curvature_ref as C
import measure_ref as MR

pytestmark = pytest.mark.gpu

CHUNK = 256  # MB_CH
CASES = ["small", "general", "interior", "onecell", "values", "cut", "zeros"]
SEAMS = ["host", "device"]
ISOS = [0.0, 0.0625]
CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6
LO = (-1.5, -1.5, -1.5)
NAMES = ("area", "volume", "x dV", "y dV", "z dV", "x dS", "y dS", "z dS", "q dS")


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _geometry(case):
    """(phi, mask, q, npts, dx) of a case; shared and read-only"""
    from levelsetfortran_amd import fields

    npts = {"small": (10, 10, 10), "onecell": (10, 10, 10), "general": (40, 33, 27), "interior": (25, 25, 25), "values": (12, 11, 10),
            "cut": (25, 25, 25), "zeros": (9, 8, 7)}[case]
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    x, y, z, _ = fields.grid_axes(npts)
    if case == "small":
        mask = (np.abs(phi) < 2.1 * dx).astype(np.int32)
    elif case == "onecell":
        mask = np.zeros(npts, np.int32)
        mask[4, 4, 4] = 1
    elif case == "general":
        mask = (np.abs(phi) < 4.1 * dx).astype(np.int32)
    elif case == "interior":
        mask = np.ones(npts, np.int32)
    elif case == "cut":
        mask = np.zeros(npts, np.int32)
        mask[:13] = 1
    elif case == "zeros":
        mask = np.ones(npts, np.int32)
        phi = np.asfortranarray(np.broadcast_to((x - x[4])[:, None, None], npts))
    else:
        band = np.abs(phi) < 1.3 * dx
        mask = np.where(band, 1, 0).astype(np.int32)
        mask[~band & (phi > 3.5 * dx)] = 7  # not 1: not in the list
        mask[~band & (phi < 0)] = -1
        for a in range(3):  # 1s on all six walls: ignored
            sl = [slice(None)] * 3
            for side in (0, -1):
                sl[a] = side
                mask[tuple(sl)] = 1
    mask = np.asfortranarray(mask)
    q = np.asfortranarray(1.25 + 0.5 * x[:, None, None] - np.sin(2.0 * y[None, :, None]) * (0.75 + z[None, None, :]))
    for a in (phi, mask, q):
        a.setflags(write=False)
    return phi, mask, q, npts, dx


def _prefill(npts):
    """cell_area as the caller hands it in: NaN and -7 alternating"""
    a = np.full(int(np.prod(npts)), np.nan)
    a[::2] = -7.0
    return np.asfortranarray(a.reshape(npts, order="F"))


@functools.lru_cache(maxsize=None)
def _want(case, hasq, iso):
    phi, mask, q, npts, dx = _geometry(case)
    r = MR.measure_band(phi, mask, dx, LO, iso=iso, q=q if hasq else None, cell_area=_prefill(npts))
    r.cell_area.setflags(write=False)
    return r


def test_the_cases_are_what_the_docstring_says():
    phi, mask, q, npts, dx = _geometry("small")
    assert B.list_of(mask).sum() == 246 < CHUNK
    n = int(B.list_of(_geometry("general")[1]).sum())
    assert (n + CHUNK - 1) // CHUNK == 25 and n % CHUNK != 0, n
    assert B.list_of(_geometry("interior")[1]).sum() == 23 ** 3
    w = _want("interior", False, 0.0)
    assert w.open == 0 and w.crossed == 420 and w.triangles == 2508
    assert B.list_of(_geometry("interior")[1])[23, 1:-1, 1:-1].all()  # list cells whose upper corners (index 24) are wall points
    one = _want("onecell", True, 0.0)
    assert one.info == [1, 0, 0, 0, 0] and one.M == (0.0,) * 9 and one.cell_area[4, 4, 4] == 0.0
    phi, mask, q, npts, dx = _geometry("values")
    inner = mask[1:-1, 1:-1, 1:-1]
    assert (inner == 0).any() and (inner == 7).any() and (inner == -1).any()
    assert B.list_of(mask).sum() == np.count_nonzero(np.abs(phi[1:-1, 1:-1, 1:-1]) < 1.3 * dx) < mask[mask == 1].size
    assert 0 < _want("values", False, 0.0).crossed
    cut, full = _want("cut", False, 0.0), _want("interior", False, 0.0)
    assert cut.open > 0 and 0 < cut.M[0] < full.M[0]
    z = _want("zeros", False, 0.0)
    assert z.degenerate > 0 and z.crossed == 6 * 5 and np.count_nonzero(_geometry("zeros")[0] == 0.0) == 8 * 7
    assert all(_want(c, False, 0.0).degenerate == 0 for c in CASES if c != "zeros")
    assert all(_want(c, True, iso).crossed > 0 for c in CASES if c != "onecell" for iso in ISOS)  # every variant measures something


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _bits(a, b):
    """bit for bit, NaN payloads and the sign of zero included"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _raw(lib, seam, phi, mask, q, cell, n, dx, lo, iso, M="given", stream=None):
    """the C call with sentinels in M and info: (rc, M, info, message)"""
    Mv = np.full(9, -7.0)
    info = np.full(5, -7, np.int64)
    lo = None if lo is None else np.array(lo, dtype=np.float64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), ptr(q), ptr(cell), n[0], n[1], n[2], dx, None if lo is None else lo.ctypes.data, iso,
            Mv.ctypes.data if M == "given" else None, info.ctypes.data)
    rc = lib.lsf_measure_band_device(*args, stream) if seam == "device" else lib.lsf_measure_band(*args)
    return rc, [float(v) for v in Mv], [int(v) for v in info], (lib.lsf_last_error() or b"").decode()


def _run(seam, phi, mask, q, npts, dx, iso, stream=None):
    """one call through one seam on fresh copies: (M, info, cell_area); asserts LSF_OK and that phi, mask and q are unchanged"""
    import torch
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t, ref: _host(t, ref.shape)) if seam == "device" else (lambda t, ref: t)
    p, m, c = mk(phi), mk(mask), mk(_prefill(npts))
    qq = None if q is None else mk(q)
    n = tuple(v - 1 for v in npts)
    if seam == "device":
        _lib.check(lib.lsf_set_device(0))
        torch.cuda.synchronize()
    st = None if stream is None else stream.cuda_stream
    rc, M, info, msg = _raw(lib, seam, p, m, qq, c, n, dx, LO, iso, stream=st)
    assert rc == 0, msg
    assert _bits(back(p, phi), phi) and np.array_equal(back(m, mask), mask) and (q is None or _bits(back(qq, q), q))  # read, never written
    return M, info, back(c, phi)


def _assert_totals(M, want, what):
    for k in range(9):
        bound = MR.summation_bound(want, k)
        err = abs(M[k] - want.M[k])
        print(f"{what} {NAMES[k]}: got {M[k]!r}, fsum {want.M[k]!r}, |difference| {err:.3g}, bound {bound:.3g}, ratio {err / bound if bound else 0.0:.3g}")
        assert err <= bound, (what, NAMES[k])


# ---------------------------------------------------------------------------------- 1: the statement
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("iso", ISOS)
@pytest.mark.parametrize("hasq", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_cell_area_and_info_equal_the_statement_and_the_totals_lie_within_the_bound(lsf, case, hasq, iso, seam):
    phi, mask, q, npts, dx = _geometry(case)
    want = _want(case, hasq, iso)
    M, info, cell = _run(seam, phi, mask, q if hasq else None, npts, dx, iso)
    lst = B.list_of(mask)
    print(f"{case} q={hasq} iso={iso} {seam}: info {info}, want {want.info}; cell_area differs at "
          f"{int(np.count_nonzero(cell.view(np.uint64) != want.cell_area.view(np.uint64)))} of {lst.sum()} list cells")
    assert _bits(cell, want.cell_area)
    assert _bits(cell[~lst], _prefill(npts)[~lst]) and np.all(cell[lst] >= 0.0)  # the list points, and nothing else
    assert info == want.info
    _assert_totals(M, want, f"{case} q={hasq} iso={iso} {seam}")
    if not hasq:
        assert M[8] == 0.0 and not np.signbit(M[8])


# ---------------------------------------------------------------------------------- 2: streams, run to run, seam to seam
@pytest.mark.parametrize("hasq", [False, True])
def test_side_stream_run_to_run_and_both_seams_give_the_same_bits(lsf, hasq):
    import torch

    phi, mask, q, npts, dx = _geometry("general")
    qq = q if hasq else None
    first = _run("device", phi, mask, qq, npts, dx, 0.0)
    for _ in range(2):  # a side stream, twice
        again = _run("device", phi, mask, qq, npts, dx, 0.0, stream=torch.cuda.Stream())
        assert again[0] == first[0] and again[1] == first[1] and _bits(again[2], first[2])
    host = _run("host", phi, mask, qq, npts, dx, 0.0)
    assert host[0] == first[0] and host[1] == first[1] and _bits(host[2], first[2])


# ---------------------------------------------------------------------------------- 3: the Python name
@pytest.mark.parametrize("seam", SEAMS)
def test_python_report_names_the_totals(lsf, seam):
    phi, mask, q, npts, dx = _geometry("interior")  # the sphere of radius 0.6 + iso lies wholly inside this grid
    n = tuple(v - 1 for v in npts)
    M, info, cell = _run(seam, phi, mask, q, npts, dx, 0.0625)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    c = mk(_prefill(npts))
    rep = lsf.measureBand(mk(phi), mk(mask), *n, dx, LO, iso=0.0625, q=mk(q), cell_area=c)
    assert isinstance(rep, lsf.MeasureReport)
    assert (rep.area, rep.volume, rep.q_integral) == (M[0], M[1], M[8])
    assert rep.centroid == tuple(v / M[1] for v in M[2:5]) and rep.surface_centroid == tuple(v / M[0] for v in M[5:8])
    assert [rep.cells, rep.crossed, rep.triangles, rep.open, rep.degenerate] == info
    assert _bits(c if seam == "host" else _host(c, npts), cell)
    assert max(abs(a - b) for a, b in zip(rep.centroid, CENTRE)) < 1e-4 and abs(rep.area / (4 * math.pi * (RADIUS + 0.0625) ** 2) - 1) < 0.012 and rep.open == 0
    assert lsf.measureBand(mk(phi), mk(mask), *n, dx, LO).q_integral == 0.0  # the optional arguments may be left out


# ---------------------------------------------------------------------------------- 4: compositions
@pytest.mark.parametrize("seam", SEAMS)
def test_counts_and_volume_agree_with_the_extracted_mesh(lsf, seam):
    """lsf_extract_surface on the same field: the same crossed cells and triangles (the mask holds every crossed cell), and
    lsf_mesh_check's signed volume of the fetched mesh within the bound of the statement's volume contributions"""
    phi, mask, q, npts, dx = _geometry("general")
    n = tuple(v - 1 for v in npts)
    want = _want("general", False, 0.0)
    M, info, _ = _run(seam, phi, mask, None, npts, dx, 0.0)
    p = _dev(phi) if seam == "device" else phi.copy(order="F")
    sX, sE, sinfo = lsf.extractSurface(p, *n, dx, LO)
    assert info[1] == sinfo.cells_crossed and info[2] == sinfo.triangles == len(sE)
    if seam == "device":
        sX, sE = sX.cpu().numpy(), sE.cpu().numpy()
    vol = lsf.meshCheck(sX, sE).signed_volume
    bound = MR.summation_bound(want, 1)
    print(f"signed volume of the mesh {vol!r}, M[1] {M[1]!r}, |difference| {abs(vol - M[1]):.3g}, bound {bound:.3g}")
    assert vol > 0 and abs(vol - M[1]) <= bound


@pytest.mark.parametrize("seam", SEAMS)
def test_gauss_of_curvature_band_plugs_in_as_q(lsf, seam):
    """gauss written by curvatureBand on the cells of a mask, NaN everywhere else, handed to measureBand as q on the same mask: the
    integral of the Gaussian curvature, equal to the two statements composed and near 4 pi"""
    phi, _, _, npts, dx = _geometry("interior")  # (the sphere of `general` reaches the wall k = nz, whose points are in no list)
    mask = np.asfortranarray((np.abs(phi) < 2.1 * dx).astype(np.int32))
    n = tuple(v - 1 for v in npts)
    nan = lambda: np.full(npts, np.nan, order="F")
    K = C.curvature_band(phi, mask, dx, nan(), nan()).gauss
    assert np.isnan(K[~B.list_of(mask)]).all()
    want = MR.measure_band(phi, mask, dx, LO, q=K)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    p, m, k, g = mk(phi), mk(mask), mk(nan()), mk(nan())
    lsf.curvatureBand(p, m, *n, dx, k, gauss=g)
    rep = lsf.measureBand(p, m, *n, dx, LO, q=g)
    bound = MR.summation_bound(want, 8)
    print(f"integral of K / 4 pi: {rep.q_integral / (4 * math.pi)!r}; statements {want.M[8]!r}, got {rep.q_integral!r}, bound {bound:.3g}")
    assert abs(rep.q_integral - want.M[8]) <= bound and [rep.cells, rep.crossed, rep.triangles, rep.open, rep.degenerate] == want.info
    assert abs(rep.q_integral / (4 * math.pi) - 1.0) < 0.01


# ---------------------------------------------------------------------------------- 5: errors
@pytest.mark.parametrize("seam", SEAMS)
def test_invalid_arguments_leave_everything_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    _lib.check(lib.lsf_set_device(0))
    phi0, mask0, q0, npts, dx = _geometry("small")
    n = tuple(v - 1 for v in npts)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t, ref: _host(t, ref.shape)) if seam == "device" else (lambda t, ref: t)
    sent = np.full(npts, -7.0, order="F")
    phi, mask, q, cell = mk(phi0), mk(mask0), mk(q0), mk(sent)
    ok = dict(phi=phi, mask=mask, q=q, cell=cell, n=n, dx=dx, lo=LO, iso=0.0)
    # a non-finite value on an endpoint of a crossed edge of a measured cell, with the statement's count
    res = MR.measure_band(phi0, mask0, dx, LO)
    c0 = tuple(res.cells_c0[len(res.cells_c0) // 2])
    bad_phi, bad_q = phi0.copy(order="F"), q0.copy(order="F")
    bad_phi[c0], bad_q[c0] = np.nan, np.inf
    counts = {}
    for name, kw in (("phi", dict(phi=bad_phi)), ("q", dict(q=bad_q))):
        with pytest.raises(MR.Invalid) as e:
            MR.measure_band(**dict(dict(phi=phi0, mask=mask0, dx=dx, xLo=LO, q=q0), **kw))
        counts[name] = e.value.count
    assert counts["phi"] >= 1 and counts["q"] >= 1
    cases = {
        "NULL phi": dict(phi=None),
        "NULL mask": dict(mask=None),
        "NULL xLo": dict(lo=None),
        "NULL M": dict(M=None),
        "cell_area is phi": dict(cell=phi),
        "cell_area is q": dict(cell=q),
        "cell_area is mask": dict(cell=mask),
        "nx < 2": dict(n=(1, n[1], n[2])),
        "nz < 2": dict(n=(n[0], n[1], 0)),
        "dx = 0": dict(dx=0.0),
        "dx < 0": dict(dx=-dx),
        "dx NaN": dict(dx=float("nan")),
        "dx inf": dict(dx=float("inf")),
        "iso NaN": dict(iso=float("nan")),
        "iso inf": dict(iso=float("inf")),
        "xLo NaN": dict(lo=(-1.5, float("nan"), -1.5)),
        "xLo inf": dict(lo=(float("inf"), -1.5, -1.5)),
        "NaN phi on a crossed edge": dict(phi=mk(bad_phi)),
        "inf q on a crossed edge": dict(q=mk(bad_q)),
        "NaN phi and inf q": dict(phi=mk(bad_phi), q=mk(bad_q)),
    }
    for name, change in cases.items():
        rc, M, info, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and M == [-7.0] * 9 and info == [-7] * 5, name  # nothing reported
        assert np.array_equal(back(cell, sent), sent), name  # nothing written
        assert _bits(back(phi, phi0), phi0) and np.array_equal(back(mask, mask0), mask0) and _bits(back(q, q0), q0), name
        if "phi on" in name or "and" in name:
            assert msg.startswith(f"lsf_measure_band: {counts['phi']} crossed edge") and "phi - iso" in msg, msg
        elif "q on" in name:
            assert msg.startswith(f"lsf_measure_band: {counts['q']} crossed edge") and "non-finite q" in msg, msg
    # a NaN where no crossed edge of a measured cell ends is legal, in phi and in q
    far = tuple(np.argwhere(np.abs(phi0[1:-1, 1:-1, 1:-1]) > 3.9 * dx)[0] + 1)
    assert not B.list_of(mask0)[far]
    fp, fq = phi0.copy(order="F"), q0.copy(order="F")
    fp[far] = fq[far] = np.nan
    want = MR.measure_band(fp, mask0, dx, LO, q=fq, cell_area=sent)
    rc, M, info, msg = _raw(lib, seam, **dict(ok, phi=mk(fp), q=mk(fq)))
    assert rc == 0 and info == want.info and _bits(back(cell, sent), want.cell_area), msg
    _assert_totals(M, want, f"valid call after the refusals, {seam}")
    # the Python layer raises the same error
    with pytest.raises(lsf.LsfError) as e:
        lsf.measureBand(phi, mask, *n, dx, LO, q=q, cell_area=q)
    assert e.value.code == _lib.LSF_ERR_INVALID and "overlaps" in str(e.value)


# ---------------------------------------------------------------------------------- 6: the empty list
@pytest.mark.parametrize("seam", SEAMS)
def test_empty_list_gives_zeros_and_writes_nothing(lsf, seam):
    phi, _, q, npts, dx = _geometry("general")
    walls = np.zeros(npts, np.int32, order="F")
    walls[0, :, :], walls[:, -1, :] = 1, 1  # 1s on wall points only
    walls[5, 5, 5] = 2
    M, info, cell = _run(seam, phi, walls, q, npts, dx, 0.0)
    assert M == [0.0] * 9 and info == [0] * 5 and _bits(cell, _prefill(npts))
