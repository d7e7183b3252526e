"""lsf_cut_cells_band on the GPU against tests/cut_cells_ref.py, the serial statement of the contract in include/lsf.h, on both
seams: every per-cell output -- the whole array, bit pattern by bit pattern, over a NaN-and--7 prefill --, info and vof_min are
compared with `==`; volume lies within N * 2^-53 * sum|vof| of math.fsum of the statement's cells, N the non-zero fractions: the
largest distance any order of summation can have from the exact sum (cut_cells_ref.volume_bound, derived and not measured; the
factor dx^3 rounds once on each side).

Grids and masks, the smallest on which each piece can go wrong (a chunk is 256 list entries, MB_CH in csrc/lsf_minmax_band.hpp):
  general   (19,17,15) wavy sphere, every interior point listed: 3315 cells, 13 chunks, the last ragged; 250 cut cells with all seven
            edge types and, between the two levels, every tetrahedron pattern (tests/test_cut_cells_cpu.py)
  band      the same field, |phi| < 2.1 dx: cut cells at the rim of the list
  inside    the same field, phi < 2.1 dx: the inside plus a rim -- volume is the body's
  onecell   a list of one cut cell of the same field
  cut       the same field, the half-space i < 9 through the body: info[3] > 0
  zeros     (9,8,7), every interior point, phi = x - x[4]: phi == iso on the grid points of a plane
  sliver    (7,6,6), one grid point inside by 1e-12 dx: fractions of 1e-35 .. 1e-23, raw values below 0 that are clamped
  plane     (12,11,10), the oblique plane n = (1,2,3)/sqrt(14)"""
import contextlib
import functools
import math

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R
import cut_cells_ref as CC
import extract_ref as X
import measure_ref as MR

pytestmark = pytest.mark.gpu

CHUNK = 256  # MB_CH
CASES = ["general", "band", "inside", "onecell", "cut", "zeros", "sliver", "plane"]
SEAMS = ["host", "device"]
ISOS = [0.0, 0.0625]
SUBSETS = {"all": (True, True, True, True), "vof": (True, False, False, False), "apertures": (False, True, False, False),
           "volume": (False, False, False, True)}  # vof, {ax, ay, az}, {bx, by, bz}, volume / vof_min / info
CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6
LO = (-1.5, -1.5, -1.5)
NAMES = ("vof", "ax", "ay", "az", "bx", "by", "bz")
TRUST, LAZY = 1, 3  # LSF_MIRROR_TRUST, LSF_MIRROR_TRUST | LSF_MIRROR_LAZY


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@functools.lru_cache(maxsize=None)
def _geometry(case):
    """(phi, mask, npts, dx) of a case; shared and read-only"""
    from levelsetfortran_amd import fields

    npts = {"zeros": (9, 8, 7), "sliver": (7, 6, 6), "plane": (12, 11, 10)}.get(case, (19, 17, 15))
    x, y, z, dx = fields.grid_axes(npts)
    mask = np.ones(npts, np.int32)
    if case == "zeros":
        phi = np.broadcast_to((x - x[4])[:, None, None], npts)
    elif case == "sliver":
        dx = 0.25
        phi = np.full(npts, 0.3 * dx)
        phi[3, 3, 3] = -1e-12 * dx
    elif case == "plane":
        n = tuple(v / math.sqrt(14.) for v in (1., 2., 3.))
        phi = n[0] * (x[:, None, None] - 0.013) + n[1] * (y[None, :, None] + 0.021) + n[2] * (z[None, None, :] - 0.017)
    else:
        phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
        phi = phi + X.wavy(npts, dx)
        if case == "band":
            mask = (np.abs(phi) < 2.1 * dx).astype(np.int32)
        elif case == "inside":
            mask = (phi < 2.1 * dx).astype(np.int32)
        elif case == "onecell":
            mask = np.zeros(npts, np.int32)
            mask[tuple(_want("general", 0.0).cells_c0[125])] = 1
        elif case == "cut":
            mask = np.zeros(npts, np.int32)
            mask[:9] = 1
    phi, mask = np.asfortranarray(phi, dtype=np.float64), np.asfortranarray(mask)
    for a in (phi, mask):
        a.setflags(write=False)
    return phi, mask, npts, dx


def _prefill(npts, shift=0):
    """an output as the caller hands it in: NaN and -7 alternating"""
    a = np.full(int(np.prod(npts)), np.nan)
    a[shift % 2::2] = -7.0
    return np.asfortranarray(a.reshape(npts, order="F"))


@functools.lru_cache(maxsize=None)
def _want(case, iso):
    phi, mask, npts, dx = _geometry(case)
    o = [_prefill(npts, q) for q in range(7)]
    r = CC.cut_cells_band(phi, mask, dx, iso=iso, vof=o[0], aperture=o[1:4], area_vector=o[4:7])
    for a in (r.vof,) + r.aperture + r.area_vector:
        a.setflags(write=False)
    return r


def _d3(case):
    dx = _geometry(case)[3]
    return (dx * dx) * dx


def _outs(want):
    return (want.vof,) + want.aperture + want.area_vector


def test_the_cases_are_what_the_docstring_says():
    g = _want("general", 0.0)
    n = int(B.list_of(_geometry("general")[1]).sum())
    assert n == 3315 and (n + CHUNK - 1) // CHUNK == 13 and n % CHUNK != 0
    assert g.info == [3315, 250, 96, 0, 0]
    band, inside = _want("band", 0.0), _want("inside", 0.0)
    assert band.open > 0 and band.cut <= g.cut and band.cells < inside.cells < g.cells
    # `inside` holds every cut cell and every full one: its volume is the body's
    assert inside.cut == g.cut and inside.full == g.full and np.array_equal(inside.cells_c0, g.cells_c0) and inside.volume == g.volume
    one = _want("onecell", 0.0)
    assert one.info == [1, 1, 0, 1, 0] and 0.0 < one.vof_min < 1.0 and one.volume == one.vof_min * _d3("onecell")
    cut = _want("cut", 0.0)
    assert cut.open > 0 and 0 < cut.cut < g.cut and 0 < cut.volume < g.volume
    z = _want("zeros", 0.0)
    assert z.cut == 6 * 5 and z.full == 2 * 6 * 5 and np.count_nonzero(_geometry("zeros")[0] == 0.0) == 8 * 7
    s = _want("sliver", 0.0)
    assert s.cut == 8 and s.clamped > 0 and s.vof_min == 0.0 and 0.0 < s.volume < 1e-20
    p = _want("plane", 0.0)
    assert p.cut > 100 and p.full > 100 and p.clamped == 0
    assert all(_want(c, iso).cells > 0 for c in CASES for iso in ISOS)
    assert all(_want(c, iso).cut > 0 for c in CASES if c != "onecell" for iso in ISOS)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _bits(a, b):
    """bit for bit, NaN payloads and the sign of zero included"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _raw(lib, seam, phi, mask, outs, n, dx, iso, totals=True, stream=None):
    """the C call with sentinels in volume, vof_min and info: (rc, volume, vof_min, info, message).  outs: seven arrays or None each;
    totals False: volume, vof_min and info are NULL"""
    tot = np.full(2, -7.0)
    info = np.full(5, -7, np.int64)
    ptr = (lambda a: None if a is None else a.data_ptr()) if seam == "device" else (lambda a: None if a is None else a.ctypes.data)
    args = (ptr(phi), ptr(mask), n[0], n[1], n[2], dx, iso, *(ptr(a) for a in outs), tot.ctypes.data if totals else None,
            tot.ctypes.data + 8 if totals else None, info.ctypes.data if totals else None)
    rc = lib.lsf_cut_cells_band_device(*args, stream) if seam == "device" else lib.lsf_cut_cells_band(*args)
    return rc, float(tot[0]), float(tot[1]), [int(v) for v in info], (lib.lsf_last_error() or b"").decode()


def _run(seam, phi, mask, npts, dx, iso, subset="all", stream=None):
    """one call through one seam on fresh copies: (volume, vof_min, info, the seven outputs or None each); asserts LSF_OK and that phi
    and mask are unchanged"""
    import torch
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t, ref: _host(t, ref.shape)) if seam == "device" else (lambda t, ref: t)
    hv, ha, hb, ht = SUBSETS[subset]
    given = [hv, ha, ha, ha, hb, hb, hb]
    p, m = mk(phi), mk(mask)
    outs = [mk(_prefill(npts, q)) if g else None for q, g in enumerate(given)]
    n = tuple(v - 1 for v in npts)
    if seam == "device":
        _lib.check(lib.lsf_set_device(0))
        torch.cuda.synchronize()
    st = None if stream is None else stream.cuda_stream
    rc, vol, vmin, info, msg = _raw(lib, seam, p, m, outs, n, dx, iso, totals=ht, stream=st)
    assert rc == 0, msg
    assert _bits(back(p, phi), phi) and np.array_equal(back(m, mask), mask)  # read, never written
    return vol, vmin, info, [None if a is None else back(a, phi) for a in outs]


def _assert_volume(vol, want, dx, what):
    bound = CC.volume_bound(want, vol, dx)
    err = abs(vol - want.volume)
    print(f"{what}: volume {vol!r}, fsum {want.volume!r}, |difference| {err:.3g}, bound {bound:.3g}, ratio {err / bound if bound else 0.0:.3g}")
    assert err <= bound, what


# ---------------------------------------------------------------------------------- 1: the statement
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("iso", ISOS)
@pytest.mark.parametrize("case", CASES)
def test_outputs_info_and_vof_min_equal_the_statement_and_volume_lies_within_the_bound(lsf, case, iso, subset, seam):
    phi, mask, npts, dx = _geometry(case)
    want = _want(case, iso)
    vol, vmin, info, outs = _run(seam, phi, mask, npts, dx, iso, subset)
    lst = B.list_of(mask)
    for q, (got, ref) in enumerate(zip(outs, _outs(want))):
        if got is None:
            continue
        diff = int(np.count_nonzero(got.view(np.uint64) != ref.view(np.uint64)))
        print(f"{case} iso={iso} {subset} {seam}: {NAMES[q]} differs at {diff} of {lst.sum()} list cells")
        assert _bits(got, ref), NAMES[q]
        assert _bits(got[~lst], _prefill(npts, q)[~lst]) and np.isfinite(got[lst]).all()  # the list points, and nothing else
    assert sum(a is not None for a in outs) == {"all": 7, "vof": 1, "apertures": 3, "volume": 0}[subset]
    if SUBSETS[subset][3]:
        print(f"{case} iso={iso} {subset} {seam}: info {info}, want {want.info}; vof_min {vmin!r}, want {want.vof_min!r}")
        assert info == want.info
        assert np.float64(vmin).view(np.uint64) == np.float64(want.vof_min).view(np.uint64)
        _assert_volume(vol, want, dx, f"{case} iso={iso} {subset} {seam}")
    else:
        assert (vol, vmin, info) == (-7.0, -7.0, [-7] * 5)  # NULL: nothing to write to


# ---------------------------------------------------------------------------------- 2: streams, run to run, seam to seam
def test_side_stream_run_to_run_and_both_seams_give_the_same_bits(lsf):
    import torch

    phi, mask, npts, dx = _geometry("general")
    first = _run("device", phi, mask, npts, dx, 0.0)
    same = lambda a, b: a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and all(_bits(p, q) for p, q in zip(a[3], b[3]))
    for _ in range(2):  # a side stream, twice
        assert same(_run("device", phi, mask, npts, dx, 0.0, stream=torch.cuda.Stream()), first)
    assert same(_run("host", phi, mask, npts, dx, 0.0), first)
    assert _run("device", phi, mask, npts, dx, 0.0, "volume")[:3] == first[:3]  # the totals do not depend on which outputs are stored


# ---------------------------------------------------------------------------------- 3: the Python name, and measureBand
@pytest.mark.parametrize("seam", SEAMS)
def test_python_report_and_the_volume_of_measure_band(lsf, seam):
    """on `inside` the list holds the whole body: the summed fractions and the divergence-theorem volume of measureBand are the same
    polyhedron's.  They differ by at most both summation bounds plus the per-term bound of tests/test_cut_cells_cpu.py: 8 u per
    triangle term of the surface integral on its absolute sum, 8 u per non-zero fraction and the cap per cut cell on the cell sum."""
    phi, mask, npts, dx = _geometry("inside")
    n = tuple(v - 1 for v in npts)
    want = _want("inside", 0.0)
    vol, vmin, info, outs = _run(seam, phi, mask, npts, dx, 0.0)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    o = [mk(_prefill(npts, q)) for q in range(7)]
    rep = lsf.cutCellsBand(mk(phi), mk(mask), *n, dx, vof=o[0], aperture=tuple(o[1:4]), area_vector=tuple(o[4:7]))
    assert isinstance(rep, lsf.CutCellsReport)
    assert (rep.volume, rep.vof_min) == (vol, vmin) and [rep.cells, rep.cut, rep.full, rep.open, rep.clamped] == info
    assert all(_bits(a if seam == "host" else _host(a, npts), b) for a, b in zip(o, outs))
    assert lsf.cutCellsBand(mk(phi), mk(mask), *n, dx).volume == vol  # the optional arguments may be left out
    m = lsf.measureBand(mk(phi), mk(mask), *n, dx, LO)
    mw = MR.measure_band(phi, mask, dx, LO)
    assert m.crossed == rep.cut == _want("general", 0.0).cut  # every crossed cell is in the list
    Xn, E, _ = X.extract(phi, dx, LO)
    P = [Xn[E[:, v].astype(np.int64) - 1] for v in range(3)]
    terms = (P[0] * np.cross(P[1], P[2])).sum(axis=1) / 6.
    d3 = (dx * dx) * dx
    per_term = 8 * len(E) * CC.U * math.fsum(np.abs(terms)) + (8 * np.count_nonzero(want.stored) * CC.U * want.abs_sum + want.cut * CC.CAP) * d3
    bound = MR.summation_bound(mw, 1) + CC.volume_bound(want, vol, dx) + per_term
    print(f"cutCellsBand volume {rep.volume!r}, measureBand volume {m.volume!r}, |difference| {abs(rep.volume - m.volume):.3g}, bound {bound:.3g}")
    assert abs(rep.volume - m.volume) <= bound


# ---------------------------------------------------------------------------------- 4: errors
@pytest.mark.parametrize("seam", SEAMS)
def test_invalid_arguments_leave_everything_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    _lib.check(lib.lsf_set_device(0))
    phi0, mask0, npts, dx = _geometry("band")
    n = tuple(v - 1 for v in npts)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    back = (lambda t, ref: _host(t, ref.shape)) if seam == "device" else (lambda t, ref: t)
    sent = np.full(npts, -7.0, order="F")
    phi, mask = mk(phi0), mk(mask0)
    outs = [mk(sent) for _ in range(7)]
    ok = dict(phi=phi, mask=mask, outs=outs, n=n, dx=dx, iso=0.0)
    # a non-finite value on an endpoint of a crossed edge of a listed cell, with the statement's count
    res = _want("band", 0.0)
    c0 = tuple(res.cells_c0[len(res.cells_c0) // 2])
    bad_phi = phi0.copy(order="F")
    bad_phi[c0] = np.nan
    with pytest.raises(MR.Invalid) as e:
        CC.cut_cells_band(bad_phi, mask0, dx)
    count = e.value.count
    assert count >= 1
    swap = lambda q, a: outs[:q] + [a] + outs[q + 1:]
    none = lambda *qs: [None if q in qs else a for q, a in enumerate(outs)]
    cases = {
        "NULL phi": dict(phi=None),
        "NULL mask": dict(mask=None),
        "nx < 2": dict(n=(1, n[1], n[2])),
        "nz < 2": dict(n=(n[0], n[1], 0)),
        "dx = 0": dict(dx=0.0),
        "dx < 0": dict(dx=-dx),
        "dx NaN": dict(dx=float("nan")),
        "dx inf": dict(dx=float("inf")),
        "iso NaN": dict(iso=float("nan")),
        "iso inf": dict(iso=float("inf")),
        "apertures 2 of 3": dict(outs=none(2)),
        "apertures 1 of 3": dict(outs=none(1, 3)),
        "area vector 2 of 3": dict(outs=none(6)),
        "area vector 1 of 3": dict(outs=none(4, 5)),
        "nothing requested": dict(outs=[None] * 7, totals=False),
        "vof is phi": dict(outs=swap(0, phi)),
        "vof is the mask": dict(outs=swap(0, mask)),
        "ay is ax": dict(outs=swap(2, outs[1])),
        "bz is vof": dict(outs=swap(6, outs[0])),
        "bx is phi": dict(outs=swap(4, phi)),
        "NaN phi on a crossed edge": dict(phi=mk(bad_phi)),
    }
    for name, change in cases.items():
        rc, vol, vmin, info, msg = _raw(lib, seam, **dict(ok, **change))
        assert rc == _lib.LSF_ERR_INVALID, (name, rc, msg)
        assert msg and (vol, vmin) == (-7.0, -7.0) and info == [-7] * 5, name  # nothing reported
        assert all(np.array_equal(back(a, sent), sent) for a in outs), name  # nothing written
        assert _bits(back(phi, phi0), phi0) and np.array_equal(back(mask, mask0), mask0), name
        if "crossed edge" in name:
            assert msg.startswith(f"lsf_cut_cells_band: {count} crossed edge") and "phi - iso" in msg, msg
        if "of 3" in name:
            assert f"({name[-6:]} given)" in msg, msg
    # a NaN where no crossed edge of a listed cell ends is legal
    far = tuple(np.argwhere(np.abs(phi0[1:-1, 1:-1, 1:-1]) > 4.9 * dx)[0] + 1)
    assert not B.list_of(mask0)[far]
    fp = phi0.copy(order="F")
    fp[far] = np.nan
    s = [sent.copy(order="F") for _ in range(7)]
    want = CC.cut_cells_band(fp, mask0, dx, vof=s[0], aperture=s[1:4], area_vector=s[4:7])
    rc, vol, vmin, info, msg = _raw(lib, seam, **dict(ok, phi=mk(fp)))
    assert rc == 0 and info == want.info and vmin == want.vof_min, msg
    assert all(_bits(back(a, sent), b) for a, b in zip(outs, _outs(want)))
    _assert_volume(vol, want, dx, f"valid call after the refusals, {seam}")
    # the Python layer raises the same error
    with pytest.raises(lsf.LsfError) as e:
        lsf.cutCellsBand(phi, mask, *n, dx, vof=outs[0], aperture=(outs[0], outs[2], outs[3]))
    assert e.value.code == _lib.LSF_ERR_INVALID and "overlaps" in str(e.value)


# ---------------------------------------------------------------------------------- 5: the empty list
@pytest.mark.parametrize("seam", SEAMS)
def test_empty_list_gives_zeros_and_writes_nothing(lsf, seam):
    phi, _, npts, dx = _geometry("general")
    walls = np.zeros(npts, np.int32, order="F")
    walls[0, :, :], walls[:, -1, :] = 1, 1  # 1s on wall points only
    walls[5, 5, 5] = 2
    vol, vmin, info, outs = _run(seam, phi, walls, npts, dx, 0.0)
    assert vol == 0.0 and vmin == math.inf and info == [0] * 5 and all(_bits(a, _prefill(npts, q)) for q, a in enumerate(outs))


# ---------------------------------------------------------------------------------- 6: the host seam under lsf_mirror
@contextlib.contextmanager
def _mirror(flags):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    # no twin of an earlier test may be left: a fresh array can get the address of a freed one (the all-zero mask of the test before),
    # and under TRUST a current twin of that address would be taken for it
    _lib.check(lib.lsf_release_workspace())
    try:
        _lib.check(lib.lsf_mirror(flags))
        yield lib
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())


@pytest.mark.parametrize("flags", [TRUST, LAZY], ids=["trust", "lazy"])
def test_the_host_seam_reads_phi_from_a_current_twin_and_brings_outputs_home_on_ok_only(lsf, flags):
    """as tests/test_gpu_host_chain.py checks for its READERS: after a reinit sweep under lsf_mirror the latest phi lives in its twin
    (under LAZY in the twin only: the host copy is stale); the call reads that, writes its outputs at list points only, brings them
    home on LSF_OK and leaves them alone on a refusal; with lsf_mirror(0) it reads the host copy."""
    from levelsetfortran_amd import _lib, fields

    phi0, _, npts, dx = _geometry("general")
    n = tuple(v - 1 for v in npts)
    F = lambda a: a.copy(order="F")
    h = fields.reinit_step(dx)
    a1 = _dev(phi0)
    lsf.reinit(a1, None, None, *n, 1, dx, h, tol=0.0, order="jacobi", arith="strict")
    phi1 = _host(a1, npts)
    assert not _bits(phi1, phi0) and np.isfinite(phi1).all()
    mask = np.asfortranarray((np.abs(phi1) < 2.1 * dx).astype(np.int32))
    lst = B.list_of(mask)
    pre = [_prefill(npts, q) for q in range(7)]
    want = CC.cut_cells_band(phi1, mask, dx, vof=pre[0], aperture=pre[1:4], area_vector=pre[4:7])
    stale = CC.cut_cells_band(phi0, mask, dx, vof=pre[0], aperture=pre[1:4], area_vector=pre[4:7])
    assert want.info != stale.info or not _bits(want.vof, stale.vof)  # the two fields give different results: the test bites
    call = lambda p, m, o: lsf.cutCellsBand(p, m, *n, dx, vof=o[0], aperture=tuple(o[1:4]), area_vector=tuple(o[4:7]))
    check = lambda rep, o, w: ([rep.cells, rep.cut, rep.full, rep.open, rep.clamped] == w.info and rep.vof_min == w.vof_min
                               and all(_bits(a, b) for a, b in zip(o, _outs(w))))
    with _mirror(flags) as lib:
        A, m = F(phi0), F(mask)
        lsf.reinit(A, None, None, *n, 1, dx, h, tol=0.0, order="jacobi", arith="strict")
        assert _bits(A, phi0 if flags == LAZY else phi1)  # under LAZY the host copy is stale
        if flags == TRUST:
            A[...] = phi0  # what the caller promised not to do: the twin is trusted, so the call below cannot see it
        o = [F(a) for a in pre]
        rep = call(A, m, o)
        assert check(rep, o, want)
        assert all(_bits(a[~lst], b[~lst]) for a, b in zip(o, pre))  # off the list what they held
        _assert_volume(rep.volume, want, dx, f"mirror {flags}")
        assert np.array_equal(m, mask)
        # a refusal: nothing comes home
        bad = F(phi1)
        bad[tuple(want.cells_c0[0])] = np.nan
        o2 = [F(a) for a in pre]
        with pytest.raises(lsf.LsfError) as e:
            call(bad, m, o2)
        assert e.value.code == _lib.LSF_ERR_INVALID and "crossed edge" in str(e.value)
        assert all(_bits(a, b) for a, b in zip(o2, pre)) and np.isnan(bad[tuple(want.cells_c0[0])])
        # ... and a valid call afterwards
        o3 = [F(a) for a in pre]
        assert check(call(F(phi1), m, o3), o3, want)
    with _mirror(0):  # without lsf_mirror the host copy is the truth
        A = F(phi0)
        lsf.reinit(A, None, None, *n, 1, dx, h, tol=0.0, order="jacobi", arith="strict")
        assert _bits(A, phi1)
        A[...] = phi0  # same address, same size, new content
        o = [F(a) for a in pre]
        assert check(call(A, F(mask), o), o, stale)
