"""The three-lane march of the exact-GS tile (lsf_skew.hpp: skew_tile, BY = 5) keeps every bit of its results.

Field and RMS trace of `lsf.reinit(order="gs")`, 9 sweeps (a whole raster cycle plus one: every direction, so both DPP fetch
shifts of phiS against both march directions), FAST and STRICT, compared bit for bit with fixtures under tests/golden/:

    gs_march_bits_<grid>_<field>_<arith>.npy   the field after 9 sweeps
    gs_march_bits_rms.npy                      the RMS traces, [grid, field, arith, sweep]

The fixtures were recorded by tests/golden/make_gs_march_bits.py with the library of the commit BEFORE the march was changed
(phiS held in thirds and fetched by DPP, the Godunov term formed inside the WENO / first-order branch without its +-1 products):
that script runs `run_case` below, the very call the tests make, and stores what it returns.  The inputs are generated here.

Grids (points):
  a  45 x 37 x 31   2 x 2 wavefronts per tile (10 x 8 rows, 16 steps), the shape the library picks by itself below 700 (STRICT
                    500) cells across.  No extent is a multiple of the tile; the grid holds deep tiles (every row of the LDS image
                    an interior row: table-driven offsets) next to partial tiles and tiles at the walls -- checked without a
                    GPU by test_grid_holds_deep_partial_and_wall_tiles from the kernel's own conditions.
  b  23 x 19 x 15   1 x 1 wavefront per tile (5 x 4 rows).  The library's selector never picks that shape unasked, so the
                    test asks for it (LSF_GS_SKEW_W=1x1); it also holds deep, partial and wall tiles.
Fields:
  spheres   the two-sphere phi0 of fields.py
  rough     the same with every mantissa scaled by a pseudo-random factor in [1 - 2^-10, 1 + 2^-10) and, at about one point
            in 23, an exact +0, an exact -0 (both only outside the spheres) or a flipped sign (a third each): `phic > 0` against
            `phic == +-0` is where the Godunov term's select could differ from its +-1 products.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

SWEEPS = 9
GRIDS = {"a": ((45, 37, 31), None), "b": ((23, 19, 15), "1x1")}  # points, LSF_GS_SKEW_W
FIELDS = ("spheres", "rough")
ARITHS = ("fast", "strict")


def cdiv(a, b):
    return -(-a // b)


def _hash01(n, seed):
    """n pseudo-random doubles in [0, 1) (splitmix64 of the index: the same on every numpy)"""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def rough_phi0(npts):
    """the "rough" field on a grid of npts points (see the module's text): (phi0 Fortran-ordered, dx)"""
    from levelsetfortran_amd import fields

    phi0, dx = fields.two_sphere_phi0(npts)
    n = phi0.size
    flat = phi0.ravel(order="F").copy()
    flat *= 1.0 + (2.0 * _hash01(n, 1) - 1.0) * 2.0 ** -10
    pick = np.floor(_hash01(n, 2) * 23.0 * 3.0).astype(np.int64)  # 0, 1, 2: planted; everything else stays
    out = flat > 0.0  # a zero among negative neighbours has a zero gradient: the 0 / 0 of subs.f90:169, NaN by the book
    flat[(pick == 0) & out] = 0.0
    flat[(pick == 1) & out] = -0.0
    flat[pick == 2] *= -1.0
    return np.asfortranarray(flat.reshape(npts, order="F")), dx


def make_field(grid, field):
    """(phi0 Fortran-ordered, dx, h)"""
    from levelsetfortran_amd import fields

    npts = GRIDS[grid][0]
    phi0, dx = rough_phi0(npts) if field == "rough" else fields.two_sphere_phi0(npts)
    return phi0, dx, fields.reinit_step(dx)


def fixture_path(grid, field, arith):
    return os.path.join(GOLDEN, f"gs_march_bits_{grid}_{field}_{arith}.npy")


RMS_PATH = os.path.join(GOLDEN, "gs_march_bits_rms.npy")


def run_case(lsf, grid, field, arith):
    """9 sweeps through the device seam -> (field as a 1-D numpy array, i fastest; RMS trace)"""
    import torch

    phi0, dx, h = make_field(grid, field)
    nx, ny, nz = (n - 1 for n in phi0.shape)
    dev = torch.from_numpy(np.ascontiguousarray(phi0.ravel(order="F"))).cuda()
    rep = lsf.reinit(dev, None, None, nx, ny, nz, SWEEPS - 1, dx, h, tol=0.0, order="gs", arith=arith)
    assert rep.count == SWEEPS
    return dev.cpu().numpy(), np.array(rep.rms, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the grids hold the tiles they are meant to (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def skew_shape(ny, nz, strict):
    """gs_skew_w (lsf_api.hip) with LSF_GS_SKEW_W unset: (WY, WZ, BY)"""
    return (1, 4, 16) if min(ny, nz) >= (500 if strict else 700) else (2, 2, 5)


def tile_classes(kny, nz, nyt, nzt):
    """tiles of the cross-section as skew_tile classifies them: (deep, partial, at a wall)"""
    deep = partial = wall = 0
    for tj in range(cdiv(kny - 1, nyt)):
        for tk in range(cdiv(nz - 1, nzt)):
            j_lo, k_lo = 1 + tj * nyt, 1 + tk * nzt
            nj, nk = min(nyt, kny - j_lo), min(nzt, nz - k_lo)
            full = nj == nyt and nk == nzt
            deep += full and j_lo >= 4 and j_lo + nyt + 2 <= kny - 1 and k_lo >= 4 and k_lo + nzt + 2 <= nz - 1
            partial += not full
            wall += j_lo == 1 or j_lo + nj == kny or k_lo == 1 or k_lo + nk == nz
    return deep, partial, wall


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_grid_holds_deep_partial_and_wall_tiles(grid):
    npts, waves = GRIDS[grid]
    nx, ny, nz = (n - 1 for n in npts)
    for strict in (False, True):
        # (the library hands gs_skew_w min(nx, ny) and nz: the dataflow launch may run on the x <-> y transposed field)
        wy, wz, by = skew_shape(min(nx, ny), nz, strict) if waves is None else (1, 1, 5)
        assert (wy, wz, by) == ((2, 2, 5) if waves is None else (1, 1, 5))
        for kny in (nx, ny):  # the kernel's y: the caller's x when the field is transposed
            knx = ny if kny == nx else nx  # the march axis
            assert (kny - 1) % (by * wy) and (nz - 1) % (4 * wz) and (knx - 1) % 16  # no extent a multiple of the tile
            deep, partial, wall = tile_classes(kny, nz, by * wy, 4 * wz)
            assert deep >= 1 and partial >= 1 and wall >= 1, (grid, kny, deep, partial, wall)


def test_rough_field_has_zeros_of_both_signs_and_sign_changes():
    for grid in GRIDS:
        smooth, _, _ = make_field(grid, "spheres")
        rough, _, _ = make_field(grid, "rough")
        inner = (slice(1, -1),) * 3
        z = rough[inner] == 0.0
        assert (z & ~np.signbit(rough[inner])).sum() >= 8 and (z & np.signbit(rough[inner])).sum() >= 8
        assert ((np.signbit(rough[inner]) != np.signbit(smooth[inner])) & ~z).sum() >= 8
        assert np.isfinite(rough).all()


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit against the library before the change
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


@pytest.fixture(scope="module")
def rms_golden():
    return np.load(RMS_PATH, allow_pickle=False)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_march_keeps_every_bit(lsf, rms_golden, monkeypatch, grid, field, arith):
    import torch

    waves = GRIDS[grid][1]
    if waves:
        monkeypatch.setenv("LSF_GS_SKEW_W", waves)
    else:
        monkeypatch.delenv("LSF_GS_SKEW_W", raising=False)
    got, rms = run_case(lsf, grid, field, arith)
    want = np.load(fixture_path(grid, field, arith), allow_pickle=False)
    want_rms = rms_golden[sorted(GRIDS).index(grid), FIELDS.index(field), ARITHS.index(arith)]
    assert np.isfinite(want).all() and want.shape == got.shape
    # bit patterns, so that -0 is not +0
    assert torch.equal(torch.from_numpy(got).view(torch.int64), torch.from_numpy(want).view(torch.int64))
    assert rms.shape == (SWEEPS,) and np.array_equal(rms.view(np.int64), want_rms.view(np.int64)), (rms, want_rms)
