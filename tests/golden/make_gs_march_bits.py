#!/usr/bin/env python3
"""Records the fixtures of tests/test_gpu_gs_march_bits.py: field and RMS trace of every case of that test, as the library
that is loaded returns them.  Run on a GPU with the library of the commit whose results are to be kept, e.g.

    LSF_LIB_PATH=/path/to/that/liblsf_hip.so python3 tests/golden/make_gs_march_bits.py [OUTDIR]

(OUTDIR defaults to tests/golden).  The committed files come from the commit before the three-lane march was changed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_gpu_gs_march_bits as t  # noqa: E402

import levelsetfortran_amd as lsf  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else HERE
os.makedirs(out, exist_ok=True)
grids = sorted(t.GRIDS)
rms = np.zeros((len(grids), len(t.FIELDS), len(t.ARITHS), t.SWEEPS))
for gi, grid in enumerate(grids):
    waves = t.GRIDS[grid][1]
    if waves:
        os.environ["LSF_GS_SKEW_W"] = waves
    else:
        os.environ.pop("LSF_GS_SKEW_W", None)
    for fi, field in enumerate(t.FIELDS):
        for ai, arith in enumerate(t.ARITHS):
            got, tr = t.run_case(lsf, grid, field, arith)
            assert np.isfinite(got).all() and np.isfinite(tr).all(), (grid, field, arith)
            np.save(os.path.join(out, os.path.basename(t.fixture_path(grid, field, arith))), got)
            rms[gi, fi, ai] = tr
            print(grid, field, arith, "rms", tr[0], "...", tr[-1], flush=True)
np.save(os.path.join(out, os.path.basename(t.RMS_PATH)), rms)
print("library", os.environ.get("LSF_LIB_PATH") or "in-tree")
