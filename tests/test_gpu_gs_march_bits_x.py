"""The three-lane march of the exact-GS tile keeps every bit of its results when it marches along x (LSF_GS_MARCH=x).

tests/test_gpu_gs_march_bits.py runs the dataflow launch as the library runs it by itself: on the x <-> y transposed field, so the
p5 = 0 quirk of the reference's y derivative sits on the x lanes of the tile (the lanes that also run the tail of the update).  With
LSF_GS_MARCH=x the field is not transposed, the tile marches along the caller's x and the quirk sits on the y lanes: another lane of
every cell takes the `yquirk` side of the epsilon, and the constants, step masks, clamps and addresses of the march meet the field in
its other orientation.  No other fixture covers that.

The same `run_case` call as the other test, 9 sweeps (a whole raster cycle plus one), on grid a (45 x 37 x 31 points: 2 x 2 wavefronts
per tile, no extent a multiple of the tile, deep tiles next to partial tiles and tiles at the walls in either orientation -- see
test_grid_holds_deep_partial_and_wall_tiles there), both fields, FAST and STRICT, compared bit for bit with

    gs_march_bits_x_a_<field>_<arith>.npy   the field after 9 sweeps
    gs_march_bits_x_rms.npy                 the RMS traces, [field, arith, sweep]

recorded by tests/golden/make_gs_march_bits_x.py with the library of the commit BEFORE the constants of the FAST WENO axis moved to
scalar registers and the step masks to a carry chain.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_gs_march_bits import ARITHS, FIELDS, SWEEPS, run_case

GRID = "a"


def fixture_path(field, arith):
    return os.path.join(GOLDEN, f"gs_march_bits_x_{GRID}_{field}_{arith}.npy")


RMS_PATH = os.path.join(GOLDEN, "gs_march_bits_x_rms.npy")


def set_switches(setenv, delenv):
    """the environment of a case: the march along x, the tile shape left to the library"""
    setenv("LSF_GS_MARCH", "x")
    delenv("LSF_GS_SKEW_W")


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
def test_march_along_x_keeps_every_bit(lsf, rms_golden, monkeypatch, field, arith):
    import torch

    set_switches(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    got, rms = run_case(lsf, GRID, field, arith)
    want = np.load(fixture_path(field, arith), allow_pickle=False)
    want_rms = rms_golden[FIELDS.index(field), ARITHS.index(arith)]
    assert np.isfinite(want).all() and want.shape == got.shape
    # bit patterns, so that -0 is not +0
    assert torch.equal(torch.from_numpy(got).view(torch.int64), torch.from_numpy(want).view(torch.int64))
    assert rms.shape == (SWEEPS,) and np.array_equal(rms.view(np.int64), want_rms.view(np.int64)), (rms, want_rms)
