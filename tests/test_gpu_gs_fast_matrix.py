"""The FAST arithmetic of the exact Gauss-Seidel reinit, every tile shape and executor, against the oracle.

Every exact-GS kernel is a template with a STRICT parameter (lsf_skew.hpp: skew_tile / k_reinit_gs_persist / k_reinit_gs_skew,
lsf_boxtile.hpp: k_reinit_gs_box), so the FAST instance of each tile shape and executor is machine code of its own.  The rest of the
suite pins the STRICT instances bit for bit and, in FAST, the default family only (three lanes per cell, 2 x 2 wavefronts).  Here every
FAST instance runs 9 sweeps (a raster cycle plus one, tol = 0, h = reinit_step(dx), device seam) and is compared with `oracle.reinit`
in GS_LEX order on the same input.

Grids (points):
  G1  80 x 78 x 41   no interior extent a multiple of a tile extent; for each of c1x1 .. c1x4 it holds WIDE tiles (lsf_skew.hpp: `widex`,
                     load_wide and the 16-byte stores) in all 8 raster directions, as the field is and x <-> y transposed, next to
                     partial tiles and tiles at the walls -- test_g1_holds_wide_partial_and_wall_tiles_for_every_one_lane_shape
  G2  23 x 19 x 15   grid b of test_gpu_gs_march_bits.py: deep, partial and wall tiles of the 1 x 1 three-lane shape; no wide tile
  G3   3 x 20 x 17   nx = 2: the skewed tiles need three cells per axis (lsf_host_gs.hpp), so the default call runs on box tiles
Fields: `spheres` (fields.two_sphere_phi0) and `rough` (test_gpu_gs_march_bits.rough_phi0: mantissa noise, planted +-0, flipped signs).

The bound per point is derived from the reference alone.  FAST is the same mathematics with other rounding; lsf_cell.hpp states 4e-15
relative (about 2^-48) for its reciprocal square root.  E = max |oracle(phi0 (1 +- 2^-48)) - oracle(phi0)|, the signs from a fixed hash of
the point index, is what 9 sweeps of the reference make of one such disturbance at every point; the bound is 8 E: FAST rounds anew in
every sweep, not once, and the rsqrt term enters scaled by h.  E is 3.6e-15 .. 7.8e-15 on the six (grid, field) pairs; 8 E <= 1e-12 is
asserted, so the per-point check is never looser than the project's RMS tolerance.  test_bound_has_teeth: the oracle's own Jacobi
result and its GS_LEX result started one raster direction later (a stale halo, a wrong sweep direction) lie above 8 E at most points.

Per FAST instance: rep.count == 9; |got - oracle| <= 8 E at every point, walls included; RMS < 1e-12; the oracle's sign wherever its
value is not zero, zero where it is; rep.rms equal to the oracle's trace to rtol 1e-9 (another summation order); and the kernel
instance the library reports (lsf_profile_kernel) is the one the switches ask for.  Shapes that differ only in WY, WZ or the launch form
run the same per-cell code: inside a family the bit patterns must be equal (A: == the default 2 x 2 dataflow, B: == c1x4 dataflow,
C: slots == planes for one (TA, NY), D: == the same shape with its tables).  Between families nothing is asserted -- A forms the Godunov
term with axis_term, B with axis_pair + axis_godunov -- but test_families_are_compared_for_the_record prints what was found.

Every GPU test prints one line that starts with "gs_fast_matrix |": instance, kernel, largest |FAST - oracle|, bound, ratio.
profiles/gs_fast_matrix.txt is that output of a run on an MI355X.
"""
import itertools

import numpy as np
import pytest

from test_gpu_gs_march_bits import _hash01, cdiv, rough_phi0, tile_classes

SWEEPS = 9
TA = 16
FAST_RMS_TOL = 1.0e-12  # tests/test_gpu_parity.py
FACTOR = 8.0            # bound = FACTOR * E (see the module's text)
GRIDS = {"G1": (80, 78, 41), "G2": (23, 19, 15), "G3": (3, 20, 17)}
FIELDS = ("spheres", "rough")
SWITCHES = ("LSF_GS_SKEW_W", "LSF_GS_SCHEDULE", "LSF_GS_MARCH", "LSF_GS_NBUF", "LSF_GS_NO_TABLES", "LSF_GS_NY", "LSF_GS_TA")
LANES3 = ("1x1", "2x1", "4x1", "1x2", "2x2", "4x2", "2x4")  # three lanes per cell (BY = 5); 2x2 is the default
LANES1 = ("c1x1", "c1x2", "c1x3", "c1x4")                  # one lane per cell (BY = 16)
RASTER = tuple(itertools.product((1, -1), repeat=3))


def shape_of(waves):
    """LSF_GS_SKEW_W (None: the default) -> (WY, WZ, BY)"""
    if waves is None:
        return 2, 2, 5
    cell = waves[0] == "c"
    wy, wz = (int(v) for v in waves.lstrip("c").split("x"))
    return wy, wz, 16 if cell else 5


# ---------------------------------------------------------------------------------------------------------------------
# inputs, reference and bound: once per (grid, field), never changed
# ---------------------------------------------------------------------------------------------------------------------
_inputs, _refs = {}, {}


def inputs(grid, field):
    """(phi0 Fortran-ordered, dx, h)"""
    if (grid, field) not in _inputs:
        from levelsetfortran_amd import fields

        npts = GRIDS[grid]
        phi0, dx = rough_phi0(npts) if field == "rough" else fields.two_sphere_phi0(npts)
        phi0.setflags(write=False)
        _inputs[grid, field] = (phi0, dx, fields.reinit_step(dx))
    return _inputs[grid, field]


def _oracle_run(oracle, phi0, npts, dx, h, order=None, first_raster=0):
    nx, ny, nz = (n - 1 for n in npts)
    out = phi0.copy(order="F")
    rc, n, trace = oracle.reinit(out, nx, ny, nz, SWEEPS - 1, dx, h, tol=0.0, order=oracle.GS_LEX if order is None else order,
                                 first_raster=first_raster)
    assert rc == 0 and n == SWEEPS and np.isfinite(out).all()
    return out.ravel(order="F"), trace


def reference(oracle, grid, field):
    """(oracle's field after 9 sweeps as a 1-D array, i fastest; its RMS trace; E)"""
    if (grid, field) not in _refs:
        phi0, dx, h = inputs(grid, field)
        npts = GRIDS[grid]
        ref, trace = _oracle_run(oracle, phi0, npts, dx, h)
        sign = np.where(_hash01(phi0.size, 3) < 0.5, -1.0, 1.0).reshape(npts, order="F")
        nudged, _ = _oracle_run(oracle, np.asfortranarray(phi0 * (1.0 + sign * 2.0 ** -48)), npts, dx, h)
        e = float(np.abs(nudged - ref).max())
        ref.setflags(write=False)
        _refs[grid, field] = (ref, trace, e)
    return _refs[grid, field]


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the grids hold what they were chosen for, the bound has teeth, the bound is no looser than the RMS tolerance
# ---------------------------------------------------------------------------------------------------------------------
def skew_tile_census(knx, kny, nz, wy, wz, by, sj, sk, image_fits):
    """Tiles of one sweep as skew_tile classifies them (lsf_skew.hpp, with the lookup tables in place): (deep, wide, partial, at a
    y or z wall).  knx, kny: the kernel's view of the grid (cells); the tile list is get_skew_tiles' (lsf_api.hip)."""
    nyt, nzt = by * wy, 4 * wz
    n_tj, n_tk, nxi = cdiv(kny - 1, nyt), cdiv(nz - 1, nzt), knx - 1
    deep = wide = partial = wall = 0
    for f_c, f_b in itertools.product(range(n_tk), range(n_tj)):
        tj, tk = (f_b if sj > 0 else n_tj - 1 - f_b), (f_c if sk > 0 else n_tk - 1 - f_c)
        j_lo, k_lo = 1 + tj * nyt, 1 + tk * nzt
        nj, nk = min(nyt, kny - j_lo), min(nzt, nz - k_lo)
        full = nj == nyt and nk == nzt
        # `deep`: full, and every row of the LDS image (three halo rows on each side included) is an interior row
        is_deep = full and j_lo >= 4 and j_lo + nyt + 2 <= kny - 1 and k_lo >= 4 and k_lo + nzt + 2 <= nz - 1
        at_wall = j_lo == 1 or j_lo + nj == kny or k_lo == 1 or k_lo + nk == nz
        m_lo, m_hi = (nyt * f_b + nzt * f_c) // TA, (nyt * f_b + nyt - 1 + nzt * f_c + nzt - 1 + nxi - 1) // TA
        for m in range(m_lo, m_hi + 1):
            x0 = TA * m - nyt * f_b - nzt * f_c
            # `widex`: one lane per cell, deep, entries 0 .. 22 of every row interior cells, the image inside the buffer descriptor
            is_wide = by == 16 and is_deep and x0 - (nyt + nzt + 4) >= 0 and x0 + 22 <= nxi - 1 and image_fits
            deep, wide, partial, wall = deep + is_deep, wide + is_wide, partial + (not full), wall + at_wall
    return deep, wide, partial, wall


def test_g1_holds_wide_partial_and_wall_tiles_for_every_one_lane_shape():
    """as the field is (slot launches, LSF_GS_MARCH=x) and x <-> y transposed (the dataflow launch), in all 8 raster directions"""
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    nx, ny, nz = (n - 1 for n in GRIDS["G1"])
    wide_per_direction = {"c1x4": 3, "c1x3": 9, "c1x2": 12, "c1x1": 48}  # what the kernel's conditions give on this grid
    for waves in LANES1:
        wy, wz, by = shape_of(waves)
        assert (ny - 1) % (by * wy) and (nx - 1) % (by * wy) and (nz - 1) % (4 * wz) and (nx - 1) % TA and (ny - 1) % TA
        for knx, kny in ((nx, ny), (ny, nx)):
            fits = lib.lsf_skew_wide_fits(knx, kny, 4 * wz) == 1
            for _, sj, sk in RASTER:
                deep, wide, partial, wall = skew_tile_census(knx, kny, nz, wy, wz, by, sj, sk, fits)
                assert wide == wide_per_direction[waves] and deep > wide, (waves, knx, kny, sj, sk, deep, wide)
                assert partial >= 1 and wall >= 1, (waves, knx, kny, sj, sk, partial, wall)
    # G2 holds no wide tile for any one-lane shape: what runs there in family B is the narrow path alone
    nx, ny, nz = (n - 1 for n in GRIDS["G2"])
    for waves in LANES1:
        wy, wz, by = shape_of(waves)
        for (knx, kny), (_, sj, sk) in itertools.product(((nx, ny), (ny, nx)), RASTER):
            assert skew_tile_census(knx, kny, nz, wy, wz, by, sj, sk, True)[1] == 0


def test_grids_hold_deep_partial_and_wall_tiles_of_the_three_lane_shapes():
    """G1: every three-lane shape.  G2: the 1 x 1 shape it was chosen for (test_gpu_gs_march_bits.py, grid b).  A deep tile is never
    the first of its row (j_lo >= 4) and has three more rows behind it, so an axis must hold 2 NYT + 3 (2 NZT + 3) interior rows: the
    larger shapes cannot have one on G2, whichever way the field lies; they have partial and wall tiles there, deep ones on G1."""
    for grid, waves in itertools.product(("G1", "G2"), LANES3):
        nx, ny, nz = (n - 1 for n in GRIDS[grid])
        wy, wz, by = shape_of(waves)
        for kny in (ny, nx):  # the kernel's y: the caller's x when the field is transposed
            deep, partial, wall = tile_classes(kny, nz, by * wy, 4 * wz)
            assert partial >= 1 and wall >= 1, (grid, waves, kny, partial, wall)
            if grid == "G1" or waves == "1x1":
                assert deep >= 1, (grid, waves, kny)
            else:
                assert deep == 0 and (kny - 1 < 2 * by * wy + 3 or nz - 1 < 8 * wz + 3), (grid, waves, kny)
            # the census above and tile_classes state the same conditions
            for _, sj, sk in RASTER:
                d2, _, p2, w2 = skew_tile_census(nx if kny == ny else ny, kny, nz, wy, wz, by, sj, sk, True)
                assert (d2 > 0, p2 > 0, w2 > 0) == (deep > 0, partial > 0, wall > 0)


def test_g3_is_below_the_skewed_tiles():
    assert GRIDS["G3"][0] - 1 == 2  # skew needs nx, ny, nz >= 3 (lsf_host_gs.hpp: reinit_slot_core)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_bound_is_no_looser_than_the_rms_tolerance(oracle, grid, field):
    _, _, e = reference(oracle, grid, field)
    print(f"gs_fast_matrix_bound | {grid} | {field} | E {e:.3e} | bound {FACTOR * e:.3e}")
    assert 0.0 < FACTOR * e <= 1.0e-12


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_bound_has_teeth(oracle, grid, field):
    """what a stale halo (the oracle's Jacobi sweep) or a wrong sweep direction (GS_LEX started one raster direction later) would
    produce lies above the bound at more than half of the points"""
    ref, _, e = reference(oracle, grid, field)
    phi0, dx, h = inputs(grid, field)
    for name, kw in (("jacobi", {"order": oracle.JACOBI}), ("first_raster=1", {"first_raster": 1})):
        wrong, _ = _oracle_run(oracle, phi0, GRIDS[grid], dx, h, **kw)
        d = np.abs(wrong - ref)
        share = float((d > FACTOR * e).mean())
        print(f"gs_fast_matrix_teeth | {grid} | {field} | {name} | above the bound at {100 * share:.1f} % of points | max {d.max():.3e}")
        assert share > 0.5, (grid, field, name, share)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


_runs = {}


def run(lsf, monkeypatch, grid, field, arith, env, seam="device"):
    """9 sweeps with exactly the switches of `env` set -> (field as a 1-D array, i fastest; RMS trace; kernel instance that ran).
    Kept per instance, so that the head of a family is computed once."""
    key = (grid, field, arith, tuple(sorted(env.items())), seam)
    if key in _runs:
        return _runs[key]
    import torch

    from levelsetfortran_amd import _lib

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        assert name in SWITCHES
        monkeypatch.setenv(name, value)
    phi0, dx, h = inputs(grid, field)
    nx, ny, nz = (n - 1 for n in phi0.shape)
    lib = _lib.load()
    lib.lsf_profile(1)  # the library then names the sweep kernel instance of the call
    try:
        if seam == "device":
            dev = torch.from_numpy(phi0.ravel(order="F").copy()).cuda()
            rep = lsf.reinit(dev, None, None, nx, ny, nz, SWEEPS - 1, dx, h, tol=0.0, order="gs", arith=arith)
            got = dev.cpu().numpy()
        else:
            host = phi0.copy(order="F")
            rep = lsf.reinit(host, None, None, nx, ny, nz, SWEEPS - 1, dx, h, tol=0.0, order="gs", arith=arith)
            got = host.ravel(order="F")
        kernel = (lib.lsf_profile_kernel() or b"").decode()
    finally:
        lib.lsf_profile(0)
    assert rep.count == SWEEPS
    got.setflags(write=False)
    _runs[key] = (got, np.array(rep.rms, dtype=np.float64), kernel)
    return _runs[key]


def same_bits(a, b):
    """bit patterns, so that -0 is not +0"""
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def kernel_name(env, arith, grid):
    """the instance reinit_slot_core launches for these switches (the name lsf_profile_kernel reports)"""
    st = "true" if arith == "strict" else "false"
    sched = env.get("LSF_GS_SCHEDULE", "dataflow")
    if sched in ("slots", "planes") or grid == "G3":
        return f"k_reinit_gs_box<{env.get('LSF_GS_TA', '16')},{env.get('LSF_GS_NY', '5')},{st}>"
    wy, wz, by = shape_of(env.get("LSF_GS_SKEW_W"))
    return f"{'k_reinit_gs_persist' if sched == 'dataflow' else 'k_reinit_gs_skew'}<16,{wy},{wz},{by},{st}>"


def label(env):
    return " ".join(f"{k[7:]}={v}" for k, v in env.items()) or "(nothing set)"


def check_fast(oracle, family, grid, field, env, result):
    """the five assertions of a FAST instance, after its line of the record"""
    got, rms, kernel = result
    ref, trace, e = reference(oracle, grid, field)
    d = np.abs(got - ref)
    bound = FACTOR * e
    print(f"gs_fast_matrix | {family} | {grid} | {field} | fast | {label(env)} | {kernel} | max |FAST - oracle| {d.max():.3e} | "
          f"bound {bound:.3e} | ratio {d.max() / bound:.4f}")
    assert kernel == kernel_name(env, "fast", grid), kernel
    assert got.shape == ref.shape and np.isfinite(got).all()
    worst = int(np.argmax(d))
    assert d.max() <= bound, (worst, np.unravel_index(worst, GRIDS[grid], order="F"), float(d.max()), bound, int((d > bound).sum()))
    assert float(np.sqrt(np.mean(d * d))) < FAST_RMS_TOL
    zero = ref == 0.0
    assert np.array_equal(np.signbit(got[~zero]), np.signbit(ref[~zero])) and (got[zero] == 0.0).all()
    assert rms.shape == (SWEEPS,) and np.allclose(rms, trace, rtol=1e-9, atol=0), (rms, trace)


def _ids(cases):
    return ["-".join([c[0], c[1]] + [f"{k[7:]}={v}" for k, v in c[2].items()]) for c in cases]


# ---- A: three lanes per cell ------------------------------------------------------------------------------------------
A_HEAD = {"LSF_GS_SCHEDULE": "dataflow"}  # 2 x 2 wavefronts, dataflow launch: what the library runs unasked
A_CASES = [(grid, field, dict(({"LSF_GS_SKEW_W": waves} if waves else {}), LSF_GS_SCHEDULE=sched))
           for grid in ("G1", "G2") for field in FIELDS for waves in (None, "1x1", "2x1", "4x1", "1x2", "4x2", "2x4")
           for sched in ("dataflow", "skew")]


@pytest.mark.gpu
@pytest.mark.parametrize("grid,field,env", A_CASES, ids=_ids(A_CASES))
def test_three_lane_shapes_fast(lsf, oracle, monkeypatch, grid, field, env):
    result = run(lsf, monkeypatch, grid, field, "fast", env)
    check_fast(oracle, "A", grid, field, env, result)
    head = run(lsf, monkeypatch, grid, field, "fast", A_HEAD)
    assert same_bits(result[0], head[0]), int((result[0] != head[0]).sum())
    # ... and the default is what a call with nothing set runs
    unset = run(lsf, monkeypatch, grid, field, "fast", {})
    assert unset[2] == head[2] and same_bits(unset[0], head[0])


# ---- B: one lane per cell ---------------------------------------------------------------------------------------------
B_HEAD = {"LSF_GS_SKEW_W": "c1x4", "LSF_GS_SCHEDULE": "dataflow"}
B_ENVS = [{"LSF_GS_SKEW_W": waves, "LSF_GS_SCHEDULE": sched} for waves in LANES1 for sched in ("dataflow", "skew")] + [
    dict(B_HEAD, LSF_GS_MARCH="x"), dict(B_HEAD, LSF_GS_NBUF="3")]
B_CASES = [(grid, field, env) for grid, field in (("G1", "spheres"), ("G1", "rough"), ("G2", "spheres")) for env in B_ENVS]


@pytest.mark.gpu
@pytest.mark.parametrize("grid,field,env", B_CASES, ids=_ids(B_CASES))
def test_one_lane_shapes_fast(lsf, oracle, monkeypatch, grid, field, env):
    """on G1 with wide tiles in every raster direction (as the field is: skew, MARCH=x; transposed: dataflow), on G2 without any"""
    result = run(lsf, monkeypatch, grid, field, "fast", env)
    check_fast(oracle, "B", grid, field, env, result)
    head = run(lsf, monkeypatch, grid, field, "fast", B_HEAD)
    assert same_bits(result[0], head[0]), int((result[0] != head[0]).sum())


# ---- C: box tiles -----------------------------------------------------------------------------------------------------
C_CASES = [(grid, field, {"LSF_GS_SCHEDULE": sched, "LSF_GS_TA": ta, "LSF_GS_NY": ny})
           for grid, field in (("G1", "spheres"), ("G3", "spheres"), ("G3", "rough"))
           for ta, ny in (("16", "5"), ("16", "4"), ("32", "5"), ("32", "4")) for sched in ("slots", "planes")]


@pytest.mark.gpu
@pytest.mark.parametrize("grid,field,env", C_CASES, ids=_ids(C_CASES))
def test_box_tiles_fast(lsf, oracle, monkeypatch, grid, field, env):
    result = run(lsf, monkeypatch, grid, field, "fast", env)
    check_fast(oracle, "C", grid, field, env, result)
    other = run(lsf, monkeypatch, grid, field, "fast", dict(env, LSF_GS_SCHEDULE="slots"))
    assert same_bits(result[0], other[0]), int((result[0] != other[0]).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_default_call_falls_back_to_box_tiles_below_three_cells_fast(lsf, oracle, monkeypatch, field):
    """G3 with nothing set.  The library reports the kernel instance of a call through lsf_profile_kernel: check_fast asserts that a
    box kernel ran (kernel_name), and its field is that of the `slots` executor on the same tiles."""
    result = run(lsf, monkeypatch, "G3", field, "fast", {})
    check_fast(oracle, "C", "G3", field, {}, result)
    assert result[2] == "k_reinit_gs_box<16,5,false>"
    slots = run(lsf, monkeypatch, "G3", field, "fast", {"LSF_GS_SCHEDULE": "slots", "LSF_GS_TA": "16", "LSF_GS_NY": "5"})
    assert same_bits(result[0], slots[0])


# ---- D: without the lookup tables -------------------------------------------------------------------------------------
D_HEADS = [A_HEAD, B_HEAD]


@pytest.mark.gpu
@pytest.mark.parametrize("head", D_HEADS, ids=["default", "c1x4"])
def test_no_tables_fast(lsf, oracle, monkeypatch, head):
    env = dict(head, LSF_GS_NO_TABLES="1")
    result = run(lsf, monkeypatch, "G1", "spheres", "fast", env)
    check_fast(oracle, "D", "G1", "spheres", env, result)
    with_tables = run(lsf, monkeypatch, "G1", "spheres", "fast", head)
    assert same_bits(result[0], with_tables[0]), int((result[0] != with_tables[0]).sum())
    assert np.array_equal(result[1].view(np.int64), with_tables[1].view(np.int64))  # same tiles, same order of summation


# ---- E: the host seam -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_seam_fast(lsf, oracle, monkeypatch):
    result = run(lsf, monkeypatch, "G1", "spheres", "fast", B_HEAD, seam="host")
    check_fast(oracle, "E (host seam)", "G1", "spheres", B_HEAD, result)
    device = run(lsf, monkeypatch, "G1", "spheres", "fast", B_HEAD)
    assert same_bits(result[0], device[0]) and np.array_equal(result[1].view(np.int64), device[1].view(np.int64))


# ---- between the families: recorded, not asserted ---------------------------------------------------------------------
@pytest.mark.gpu
def test_families_are_compared_for_the_record(lsf, oracle, monkeypatch):
    """A (axis_term) and B (axis_pair + axis_godunov) form the Godunov term by different routines, the box tiles have a lane map of
    their own: whether their FAST fields agree bit for bit is printed, not required.  Each is inside the bound by its own test."""
    box = {"LSF_GS_SCHEDULE": "slots", "LSF_GS_TA": "16"}
    pairs = [("G1", "spheres", "A 2x2", A_HEAD, "B c1x4", B_HEAD), ("G1", "rough", "A 2x2", A_HEAD, "B c1x4", B_HEAD),
             ("G2", "spheres", "A 2x2", A_HEAD, "B c1x4", B_HEAD),
             ("G1", "spheres", "A 2x2", A_HEAD, "C box 16,5", dict(box, LSF_GS_NY="5")),
             ("G1", "spheres", "B c1x4", B_HEAD, "C box 16,5", dict(box, LSF_GS_NY="5")),
             ("G1", "spheres", "C box 16,5", dict(box, LSF_GS_NY="5"), "C box 16,4", dict(box, LSF_GS_NY="4")),
             ("G1", "spheres", "C box 16,5", dict(box, LSF_GS_NY="5"), "C box 32,5", dict(box, LSF_GS_NY="5", LSF_GS_TA="32"))]
    for grid, field, na, ea, nb, eb in pairs:
        a, b = run(lsf, monkeypatch, grid, field, "fast", ea)[0], run(lsf, monkeypatch, grid, field, "fast", eb)[0]
        differ = int((a.view(np.int64) != b.view(np.int64)).sum())
        verdict = "bit-identical" if differ == 0 else f"differ at {differ} of {a.size} points, max |d| {np.abs(a - b).max():.3e}"
        print(f"gs_fast_matrix_families | {grid} | {field} | {na} against {nb} | {verdict}")
        assert a.shape == b.shape


# ---- STRICT complements: the wide path and the table-free path in the reference's arithmetic ---------------------------
S_CASES = [("G1", field, {"LSF_GS_SKEW_W": waves, "LSF_GS_SCHEDULE": sched}) for field in FIELDS for waves in LANES1
           for sched in ("dataflow", "skew")] + [("G1", "spheres", dict(head, LSF_GS_NO_TABLES="1")) for head in D_HEADS]


@pytest.mark.gpu
@pytest.mark.parametrize("grid,field,env", S_CASES, ids=_ids(S_CASES))
def test_one_lane_shapes_and_no_tables_strict(lsf, oracle, monkeypatch, grid, field, env):
    got, rms, kernel = run(lsf, monkeypatch, grid, field, "strict", env)
    ref, trace, _ = reference(oracle, grid, field)
    differ = int((got != ref).sum())
    print(f"gs_fast_matrix | S | {grid} | {field} | strict | {label(env)} | {kernel} | points that differ from the oracle: {differ}")
    assert kernel == kernel_name(env, "strict", grid), kernel
    assert got.shape == ref.shape and np.array_equal(got, ref), differ
    assert np.allclose(rms, trace, rtol=1e-9, atol=0)


@pytest.mark.gpu
def test_record_names_the_device(lsf):
    import torch

    p = torch.cuda.get_device_properties(0)
    print(f"gs_fast_matrix_device | {p.name} {getattr(p, 'gcnArchName', '')}, {p.multi_processor_count} CUs, HIP {torch.version.hip} | "
          f"library {lsf.__version__}")
