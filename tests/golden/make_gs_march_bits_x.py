#!/usr/bin/env python3
"""Records the fixtures of tests/test_gpu_gs_march_bits_x.py: field and RMS trace of every case of that test (the march along x,
LSF_GS_MARCH=x), as the library that is loaded returns them.  Run on a GPU with the library of the commit whose results are to be
kept, e.g.

    LSF_LIB_PATH=/path/to/that/liblsf_hip.so python3 tests/golden/make_gs_march_bits_x.py [OUTDIR]

(OUTDIR defaults to tests/golden).  The committed files come from the commit before the second instruction diet of the three-lane tile.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_gpu_gs_march_bits_x as t  # noqa: E402

import levelsetfortran_amd as lsf  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else HERE
os.makedirs(out, exist_ok=True)
t.set_switches(os.environ.__setitem__, lambda k: os.environ.pop(k, None))
rms = np.zeros((len(t.FIELDS), len(t.ARITHS), t.SWEEPS))
for fi, field in enumerate(t.FIELDS):
    for ai, arith in enumerate(t.ARITHS):
        got, tr = t.run_case(lsf, t.GRID, field, arith)
        assert np.isfinite(got).all() and np.isfinite(tr).all(), (field, arith)
        np.save(os.path.join(out, os.path.basename(t.fixture_path(field, arith))), got)
        rms[fi, ai] = tr
        print(field, arith, "rms", tr[0], "...", tr[-1], flush=True)
np.save(os.path.join(out, os.path.basename(t.RMS_PATH)), rms)
print("library", os.environ.get("LSF_LIB_PATH") or "in-tree")
