"""tests/reseed_ref.py, the numpy statement of lsf_reseed_points (include/lsf.h), checked on the CPU: the pinned random numbers, the
attraction on a plane, every status from a named point, the precedence, the radius refresh, the counts and the top-up, the order of
the output, the seeded defects, the argument checks of the library (tests/host_args/reseed_args_main.cpp) and the library without a
device.

Figures of the statement on the vortex configuration of DESIGN.md section 4.24 (33^3 points, 64 steps out and 64 back; printed by
test_vortex_with_reseeding, recorded in DESIGN.md section 4.26), volume at the start 0.013833:
    no markers            volume 0.010747   mean error 0.336 dx
    markers, no reseed    volume 0.012081   mean error 0.191 dx   21 347 markers at the end
    reseed every 16       volume 0.012201   mean error 0.187 dx   32 027 markers at the end
"""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import reseed_inputs as I
import reseed_ref as R
import sample_ref as S

RECORDED_GAP = 0.003086 - 0.001752  # the volume losses without and with (un-reseeded) markers, DESIGN.md section 4.24

# a plane phi = x - c on a small grid
PSHAPE, PDX, PLO, PC = (13, 9, 8), 0.125, (-0.75, 0.25, 1.0), 0.03


def plane():
    X = PLO[0] + np.arange(PSHAPE[0]) * PDX
    return np.asfortranarray(np.broadcast_to((X - PC)[:, None, None], PSHAPE).copy())


KW = dict(per_cell=4, rmin=0.1, rmax=0.5, band=1.5, order=R.CUBIC, iters=4, tol=1e-3, seed=9)


def at(i, j, k, fx=0.5, fy=0.5, fz=0.5):
    return [PLO[0] + (i + fx) * PDX, PLO[1] + (j + fy) * PDX, PLO[2] + (k + fz) * PDX]


# ---------------------------------------------------------------------------------- the random numbers
PINS = [(0x0, 0x0, 0xe220a8397b1dcdaf), (0x0, 0x1, 0x6e789e6aa1b965f4), (0x5, 0x0, 0x63033b0ca389c35a),
        (0x123456789abcdef, 0x1c00e, 0x13cc6e8dbd481da), (0xffffffffffffffff, 0xfffffffffffffffe, 0xde0a564cbcd060c4),
        (0x2a, 0x1fffffffbfff, 0x15438185f23b64)]  # (seed, ctr, word): computed once with Python integers


def test_the_random_numbers_are_pinned():
    for seed, ctr, word in PINS:
        assert R.splitmix_int(seed, ctr) == word
        p, j, d = ctr // 4 // 4096, (ctr // 4) % 4096, ctr % 4
        if p < 2 ** 31:
            u = R.draw(seed, [p], [j], d)[0]
            assert u == float(word >> 11) * 2.0 ** -53 and 0.0 <= u < 1.0
    # the array arithmetic wraps like the integers do
    big = (1 << 64) - 1
    assert R.draw(big, [2 ** 31 - 2], [4095], 3)[0] == float(R.splitmix_int(big, ((2 ** 31 - 2) * 4096 + 4095) * 4 + 3) >> 11) * 2.0 ** -53


# ---------------------------------------------------------------------------------- named checks of the statement
def check_plane_attraction(defect=None):
    """npts = 0, iters large and tol tiny on a plane: every accepted marker sits on its goal, on its own side, with a legal radius"""
    phi = plane()
    kw = dict(KW, iters=40, tol=1e-9)
    r = R.reseed_points(phi, PDX, PLO, defect=defect, **kw)
    assert r.info[7] > 0 and r.info[8] >= 0.9 * r.info[7] and r.info[6] * kw["per_cell"] == r.info[7]
    val = S.sample_once(phi, None, None, PDX, np.array(PLO), np.array(r.pts), S.LINEAR)[1]
    # the goal of each accepted candidate, redrawn
    elig = R.eligible_cells(phi, None, kw["band"] * PDX)
    ci, cj, ck = np.nonzero(elig.transpose(2, 1, 0))[::-1]
    p = np.repeat(ci + PSHAPE[0] * (cj + PSHAPE[1] * ck), kw["per_cell"])
    j = np.tile(np.arange(kw["per_cell"]), ci.size)
    u3 = R.draw(kw["seed"], p, j, 3)
    goal = (kw["rmin"] + (kw["band"] - kw["rmin"]) * u3) * PDX
    assert len(r.rad) <= len(goal)
    side = np.where(r.rad < 0., -1., 1.)
    assert np.all(np.sign(val) == side) and set(side) == {-1., 1.}
    assert np.all(np.abs(r.rad) >= kw["rmin"] * PDX) and np.all(np.abs(r.rad) <= kw["rmax"] * PDX)
    if r.info[8] == r.info[7]:
        assert np.all(np.abs(np.abs(val) - goal) <= kw["tol"] * PDX + 1e-15)
    else:  # every |val| is one of the goals, to the tolerance
        assert np.all(np.abs(np.abs(val)[:, None] - goal[None, :]).min(axis=1) <= kw["tol"] * PDX + 1e-15)
    assert np.all(r.src == 0) and r.status.size == 0


def _named_markers():
    """(pts, rad, expected status): one marker per status and per step of the precedence"""
    nan = float("nan")
    rows = [
        (at(6, 4, 3), 0.02, R.KEPT),
        (at(6, 4, 3), -0.02, R.KEPT),  # an escaped one: phi > 0 there
        (at(6, 4, 3), 0.0, R.BADRADIUS),
        ([nan, 0.5, 1.3], nan, R.BADRADIUS),  # BADRADIUS before OUTSIDE
        ([1e300, 0.5, 1.3], 0.02, R.OUTSIDE),
        (at(12, 4, 3, fx=0.01), 0.02, R.OUTSIDE),
        (at(2, 4, 3), 0.02, R.OFFBAND),  # OFFBAND before FAR: the hole of the mask, far from the plane
        (at(9, 6, 5), 0.02, R.NONFINITE),  # NONFINITE before FAR: a NaN corner
        (at(10, 2, 2), 0.02, R.FAR),
        (at(1, 4, 3), np.inf, R.BADRADIUS),  # BADRADIUS before OFFBAND and FAR
    ]
    return np.asfortranarray(np.array([r[0] for r in rows])), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32)


def _named_fields():
    phi = plane()
    phi[10, 7, 6] = np.nan  # a corner of cell (9, 6, 5), 3.8 dx from the plane: FAR would apply if the value were finite
    mask = np.ones(PSHAPE, np.int32)
    mask[2, 4, 3] = 0
    return phi, np.asfortranarray(mask)


def check_statuses_and_precedence(defect=None):
    phi, mask = _named_fields()
    pts, rad, want = _named_markers()
    r = R.reseed_points(phi, PDX, PLO, pts, rad, mask=mask, defect=defect, **KW)
    assert np.array_equal(r.status, want), (r.status, want)
    assert r.info[:6] == [int(np.count_nonzero(want == c)) for c in range(6)] and sum(r.info[:6]) == len(rad)
    assert r.info[8] + r.info[9] + r.info[10] == r.info[7] and len(r.rad) == r.info[0] + r.info[8]
    # without the mask the OFFBAND one is FAR
    r2 = R.reseed_points(phi, PDX, PLO, pts, rad, defect=defect, **KW)
    assert r2.status[6] == R.FAR and np.array_equal(np.delete(r2.status, 6), np.delete(want, 6))


def check_kept_markers(defect=None):
    """position bit for bit, the refreshed radius, the escaped marker's rmin*dx with its side, src, kept first"""
    phi, mask = _named_fields()
    pts, rad, want = _named_markers()
    r = R.reseed_points(phi, PDX, PLO, pts, rad, mask=mask, defect=defect, **KW)
    assert np.array_equal(r.src[:2], [1, 2]) and np.all(r.src[2:] == 0)
    assert np.array_equal(np.array(r.pts[:2]).view(np.uint64), pts[:2].view(np.uint64))
    val = (PLO[0] + 6.5 * PDX) - PC  # 0.0325 = 0.26 dx
    assert r.rad[0] == min(max(val, KW["rmin"] * PDX), KW["rmax"] * PDX) and r.rad[0] == val
    assert r.rad[1] == -(KW["rmin"] * PDX) and r.info[13] == 1  # escaped: the smallest radius, its side kept
    far = R.reseed_points(phi, PDX, PLO, np.asfortranarray(np.array([at(7, 2, 2, fx=0.1)])), np.array([0.001]), **KW)
    assert far.status[0] == R.KEPT and far.rad[0] == KW["rmax"] * PDX  # 0.86 dx from the plane: clipped to rmax = 0.5


def check_counts_and_top_up(defect=None):
    """a full cell gets no candidate, a cell with per_cell - 1 exactly one, FAR markers are not counted, over-full cells are reported"""
    phi = plane()
    pc = KW["per_cell"]
    cellA, cellB, cellC = (6, 4, 3), (6, 2, 2), (5, 5, 5)
    rows = [at(*cellA, fx=0.1 + 0.2 * m) for m in range(pc)] + [at(*cellB, fy=0.1 + 0.2 * m) for m in range(pc - 1)]
    rows += [at(*cellC, fz=0.1 + 0.1 * m) for m in range(pc + 3)]
    farcell = (10, 2, 2)
    rows += [at(*farcell)] * 2
    pts = np.asfortranarray(np.array(rows))
    rad = np.full(len(rows), 0.02)
    r = R.reseed_points(phi, PDX, PLO, pts, rad, defect=defect, **KW)
    assert r.info[0] == 3 * pc + 2 and r.info[5] == 2
    elig = int(np.count_nonzero(R.eligible_cells(phi, None, KW["band"] * PDX)))
    assert r.info[6] == elig and r.info[7] == (elig - 3) * pc + 1  # A and C get none, B one
    assert r.info[11] == 1 and r.info[12] == pc + 3


def check_far_markers_are_not_counted(defect=None):
    """FAR markers add nothing to a count.  (A trilinear value lies between the corner values, so a FAR marker never sits in an
    eligible cell and no need can show the difference: the counts themselves do, through info[11] and info[12].)"""
    phi = plane()
    pts = np.asfortranarray(np.array([at(10, 2, 2)] * 3 + [at(6, 4, 3)]))
    r = R.reseed_points(phi, PDX, PLO, pts, np.full(4, 0.02), defect=defect, **KW)
    assert r.info[5] == 3 and r.info[0] == 1 and r.info[12] == 1 and r.info[11] == 0


def check_distinct_draws_in_a_cell(defect=None):
    """the candidates of one cell are distinct points (ctr holds j)"""
    phi = plane()
    r = R.reseed_points(phi, PDX, PLO, defect=defect, **dict(KW, iters=1, tol=10.0))  # tol so wide that no candidate moves
    assert r.info[8] > 0
    x = np.array(r.pts)
    assert len(np.unique(x.view(np.uint64).reshape(-1, 3), axis=0)) == len(x)


def check_goal_side(defect=None):
    """markers on both sides end up at |val| >= rmin*dx on their own side; most candidates are accepted"""
    phi = plane()
    r = R.reseed_points(phi, PDX, PLO, defect=defect, **KW)
    assert r.info[8] >= 0.9 * r.info[7]


def check_final_value_is_linear(defect=None):
    """on a sphere the cubic and the linear value differ: the radius is the LINEAR one"""
    phi, _ = I.fields()
    r = R.reseed_points(phi, I.DX, I.LO, order=R.CUBIC, seed=5, defect=defect, **I.MAIN)
    val = S.sample_once(phi, None, None, I.DX, np.array(I.LO), np.array(r.pts), S.LINEAR)[1]
    want = np.where(val < 0., -1., 1.) * np.minimum(np.maximum(np.abs(val), I.MAIN["rmin"] * I.DX), I.MAIN["rmax"] * I.DX)
    assert np.array_equal(r.rad, want) and np.all(np.abs(val) >= I.MAIN["rmin"] * I.DX)


def check_permutation(defect=None):
    phi, mask = I.fields()
    pts, rad = I.markers(2037)
    a = R.reseed_points(phi, I.DX, I.LO, pts, rad, mask=mask, seed=5, defect=defect, **I.MAIN)
    perm = np.random.default_rng(2).permutation(2037)
    b = R.reseed_points(phi, I.DX, I.LO, np.asfortranarray(pts[perm]), rad[perm], mask=mask, seed=5, defect=defect, **I.MAIN)
    nk = a.info[0]
    assert a.info == b.info and nk > 0 and np.all(a.src[:nk] > 0) and np.all(a.src[nk:] == 0)
    assert np.array_equal(np.array(a.pts[nk:]).view(np.uint64), np.array(b.pts[nk:]).view(np.uint64)) and np.array_equal(a.rad[nk:], b.rad[nk:])
    assert np.array_equal(perm[b.src[:nk] - 1], np.sort(a.src[:nk] - 1)[np.argsort(np.argsort(perm[b.src[:nk] - 1]))])  # the same set of kept
    assert np.array_equal(np.array(b.pts[:nk]).view(np.uint64), np.asfortranarray(pts[perm])[b.src[:nk] - 1].view(np.uint64))
    assert np.array_equal(a.status[perm], b.status)


CHECKS = {f.__name__[6:]: f for f in (check_plane_attraction, check_statuses_and_precedence, check_kept_markers, check_counts_and_top_up,
                                      check_far_markers_are_not_counted, check_distinct_draws_in_a_cell, check_goal_side,
                                      check_final_value_is_linear, check_permutation)}
# the named check each seeded defect fails
FAILS = {"goal_no_side": "goal_side", "final_on_order": "final_value_is_linear", "count_before_far": "far_markers_are_not_counted",
         "ctr_no_j": "distinct_draws_in_a_cell", "new_first": "kept_markers"}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_the_statement_passes(name):
    CHECKS[name]()


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_seeded_defect_fails_a_check(defect):
    assert set(FAILS) == set(R.DEFECTS)
    with pytest.raises(AssertionError):
        CHECKS[FAILS[defect]](defect)


def test_invalid_arguments_are_refused_by_the_statement():
    phi = plane()
    nan = float("nan")
    for kw in (dict(per_cell=0), dict(per_cell=4097), dict(rmin=0.0), dict(rmin=0.6), dict(band=0.1), dict(rmax=float("inf")), dict(band=nan),
               dict(order=2), dict(iters=0), dict(iters=65), dict(tol=-1.0), dict(tol=nan)):
        with pytest.raises(R.Invalid):
            R.reseed_points(phi, PDX, PLO, **dict(KW, **kw))
    for dx, lo in ((0.0, PLO), (nan, PLO), (PDX, (0.0, nan, 0.0))):
        with pytest.raises(R.Invalid):
            R.reseed_points(phi, dx, lo, **KW)


def test_the_inputs_of_the_gpu_tests_are_what_they_say():
    import test_gpu_reseed_points as G

    G.test_the_inputs_are_what_the_docstring_says()


def test_vortex_with_reseeding():
    import points_inputs as PI

    phi0, _ = PI.vortex_fields()
    v0 = PI.volume(phi0)
    plain, marked, reseeded = PI.vortex_run(False), PI.vortex_run(True), I.vortex_reseed_run(16)
    va, vb, vc = PI.volume(plain["phi"]), PI.volume(marked["phi"]), PI.volume(reseeded["phi"])
    ea, eb, ec = (PI.band_error(r["phi"], phi0) for r in (plain, marked, reseeded))
    print(f"vortex 33^3: volume at the start {v0:.6f}; no markers {va:.6f}, mean error {ea:.3f} dx; {len(marked['rad'])} markers, no reseed "
          f"{vb:.6f}, {eb:.3f} dx; reseed every 16: {vc:.6f}, {ec:.3f} dx, {len(reseeded['rad'])} markers at the end")
    rs = [i[2] for i in reseeded["infos"] if i[2] is not None]
    assert len(rs) == 8 and all(sum(i[:6]) == i[0] + i[5] for i in rs)  # only KEPT and FAR occur on this grid
    assert all(i[8] + i[9] + i[10] == i[7] for i in rs) and len(reseeded["rad"]) == rs[-1][0] + rs[-1][8]
    assert (v0 - vc) <= (v0 - va) - 0.5 * RECORDED_GAP
    assert len(reseeded["rad"]) > len(marked["rad"])


# ---------------------------------------------------------------------------------- the library without a device
@functools.lru_cache(maxsize=None)
def _args_table():
    from conftest import ROOT

    src = os.path.join(ROOT, "tests", "host_args", "reseed_args_main.cpp")
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    assert cxx, "no host C++ compiler (c++, or ROCm's clang++)"
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "reseed_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wno-unused-function", "-o", exe, src], check=True)
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_every_refusal_through_reseed_points_args_ok():
    """return code and message of every case of tests/host_args/reseed_args_main.cpp; every refusal the header lists is among them,
    and the valid lists pass"""
    rows = [tuple(p.strip() for p in line.split("|")) for line in _args_table()]
    assert len(rows) == 42
    for name, rc, msg in rows:
        valid = name.startswith("valid") or "may " in name
        assert int(rc) == (0 if valid else 2), name
        assert (msg == "") == valid and (valid or msg.startswith("lsf_reseed_points: ")), name
    got = {name: msg for name, _, msg in rows}
    for name, needle in (("phi NULL", "phi is NULL"), ("xLo NULL", "xLo is NULL"), ("nout NULL", "nout is NULL"), ("npts negative", "npts must be >= 0"),
                         ("pts NULL", "pts is NULL with npts > 0"), ("rad NULL", "rad is NULL with npts > 0"), ("nx 0", "nx, ny, nz must be >= 1"),
                         ("nz negative", "nx, ny, nz must be >= 1"), ("too many points", "more than 2^31 - 1 points"),
                         ("dx 0", "dx must be finite and > 0"), ("dx NaN", "dx must be finite"), ("dx inf", "dx must be finite"),
                         ("xLo NaN", "three finite values"), ("xLo inf", "three finite values"), ("per_cell 0", "per_cell must be in 1..4096"),
                         ("per_cell beyond the cap", "per_cell must be in 1..4096"), ("rmin NaN", "must be finite"), ("rmax inf", "must be finite"),
                         ("band NaN", "must be finite"), ("rmin 0", "0 < rmin <= rmax"), ("rmin negative", "0 < rmin <= rmax"),
                         ("rmin above rmax", "0 < rmin <= rmax"), ("band equals rmin", "rmin < band"), ("order 2", "unknown order"),
                         ("order -1", "unknown order"), ("iters 0", "iters must be in 1..64"), ("iters beyond the cap", "iters must be in 1..64"),
                         ("tol negative", "tol must be finite and >= 0"), ("tol NaN", "tol must be finite"), ("tol inf", "tol must be finite"),
                         ("status is phi", "status overlaps phi"), ("status in the last byte of the mask", "status overlaps mask"),
                         ("status is pts", "status overlaps pts"), ("status ends in rad", "status overlaps rad")):
        assert needle in got[name], (name, got[name])


def test_the_interface_is_there_in_every_layer():
    import levelsetfortran_amd as lsf
    from conftest import ROOT
    from levelsetfortran_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "lsf.h")).read()
    names = ("lsf_reseed_points", "lsf_reseed_points_device", "lsf_reseed_get", "lsf_reseed_get_device")
    for name in names:
        assert re.search(r"\bint %s\(" % name, hdr), name
    defines = dict(re.findall(r"#define (LSF_RESEED_[A-Z_]+) (\d+)", hdr))
    assert len(defines) == 9
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    assert (R.KEPT, R.OUTSIDE, R.OFFBAND, R.NONFINITE, R.BADRADIUS, R.FAR) == tuple(
        getattr(_lib, "LSF_RESEED_" + n) for n in ("KEPT", "OUTSIDE", "OFFBAND", "NONFINITE", "BADRADIUS", "FAR"))
    assert (R.INFO_LEN, R.MAX_PER_CELL, R.MAX_ITERS) == (_lib.LSF_RESEED_INFO_LEN, _lib.LSF_RESEED_MAX_PER_CELL, _lib.LSF_RESEED_MAX_ITERS)
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["lsf_reseed_points_device"][1]) == len(_lib.SIGNATURES["lsf_reseed_points"][1]) + 1 == 22
    assert len(_lib.SIGNATURES["lsf_reseed_get_device"][1]) == len(_lib.SIGNATURES["lsf_reseed_get"][1]) + 1 == 4
    assert callable(lsf.reseedParticles) and lsf.ReseedReport._fields == ("pts", "rad", "src", "status", "info")
    assert "seed" in lsf.reseedParticles.__doc__ and "same seed redraws the same offsets" in lsf.reseedParticles.__doc__
    f90 = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    assert "BIND(C,NAME='lsf_reseed_points')" in f90 and "PUBLIC :: reseedPoints" in f90
    assert "BIND(C,NAME='lsf_reseed_get')" in f90 and "PUBLIC :: reseedGet" in f90 and "INTEGER(c_int64_t), VALUE :: seed" in f90
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "host_reseed.f90"))
    csrc = os.path.join(ROOT, "levelsetfortran_amd", "csrc")
    for h in ("lsf_reseed_points.hpp", "lsf_host_reseed.hpp"):
        assert os.path.exists(os.path.join(csrc, h)), h
    k = open(os.path.join(csrc, "lsf_reseed_points.hpp")).read()
    assert "xs_block_scan<" in k and "void xs_block_scan" not in k  # reused, not copied


def test_python_checks_come_before_the_library():
    import levelsetfortran_amd as lsf

    phi = plane()
    n = tuple(s - 1 for s in PSHAPE)
    pts, rad, _ = _named_markers()
    for kw in (dict(order="quintic"), dict(per_cell=0), dict(per_cell=4097), dict(iters=0), dict(iters=65), dict(rmin=0.0), dict(rmin=0.6),
               dict(band=0.1), dict(tol=-1.0), dict(tol=float("nan")), dict(rad=None), dict(rad=rad[:3])):
        a = dict(pts=pts, rad=rad)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        with pytest.raises(ValueError):
            lsf.reseedParticles(phi, *n, PDX, PLO, a["pts"], a["rad"], **kw)
    with pytest.raises(ValueError):
        lsf.reseedParticles(phi, *n, 0.0, PLO)
    with pytest.raises(TypeError):
        lsf.reseedParticles(phi, *n, PDX, PLO, np.ascontiguousarray(pts), rad)  # C order
    with pytest.raises(TypeError):
        lsf.reseedParticles(phi, *n, PDX, PLO, pts, rad.astype(np.float32))


def test_no_cpu_fallback_without_device():
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    if lib.lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = plane()
    n = tuple(s - 1 for s in PSHAPE)
    pts, rad, _ = _named_markers()
    keep = (phi.copy(), pts.copy(), rad.copy())
    lo = np.array(PLO)
    status, info, nout = np.full(len(rad), -7, np.int32), np.full(R.INFO_LEN, -7, np.int64), ctypes.c_int(-7)
    rc = lib.lsf_reseed_points(phi.ctypes.data, None, *n, PDX, lo.ctypes.data, pts.ctypes.data, rad.ctypes.data, len(rad), 4, 0.1, 0.5, 1.5, R.CUBIC, 4,
                               1e-3, ctypes.c_uint64(9), status.ctypes.data, ctypes.byref(nout), info.ctypes.data)
    assert rc == _lib.LSF_ERR_NO_DEVICE and np.all(status == -7) and np.all(info == -7) and nout.value == -7
    assert np.array_equal(phi, keep[0]) and np.array_equal(pts, keep[1], equal_nan=True) and np.array_equal(rad, keep[2], equal_nan=True)
    out = np.full(3, -7.0)
    assert lib.lsf_reseed_get(out.ctypes.data, out.ctypes.data, None) == _lib.LSF_ERR_INVALID and np.all(out == -7.0)  # nothing was kept
    with pytest.raises(_lib.LsfError) as e:
        __import__("levelsetfortran_amd").reseedParticles(phi, *n, PDX, PLO)
    assert e.value.code == _lib.LSF_ERR_NO_DEVICE
