"""Time lsf_label_band beside lsf_curvature_band on the same sphere and mask: ms per call and passes run at 256^3 and 512^3, and on
the two-sphere field with every interior point listed at 256^3 (profiles/label_band_time.txt).

    python3 profiles/micro/label_band_time.py [--repeats 5] [--out FILE]

Cases: "band" is that of profiles/micro/curvature_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05)
on N^3 points over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx (phiSB of lsf_narrowband), device seam.  Timed: lsf_label_band with side =
both and the default table of 1024 rows, and the same call without a table (comp_cap = 0: the labels and ncomp alone); beside them
lsf_curvature_band (kappa only, clamp 1) on the same mask -- a call that builds the same list and makes one launch over it.
"full" is min of the distances to two spheres (radius 0.4 at (-0.6, 0, -0.2) and 0.45 at (0.6, 0.1, -0.1)) with a mask of ones: every
interior point in the list.  Each case is a child process of its own under its own time limit; the next one is not started if one
fails.  Per figure: host clock around one call that ends in a synchronise, after one warm-up call; median and spread over `repeats`
calls.  A record, not a gate.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 240  # seconds per case
CASES = ("band:256", "band:512", "full:256")

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="kind:N (internal: one child process per case)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for c in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", c, "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {c} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": "lsf_label_band (side = both) beside lsf_curvature_band (kappa only) on the same mask, device seam: ms per call (host "
                   f"clock around a call; median of {args.repeats} calls after a warm-up) and passes run",
           "command": "python3 profiles/micro/label_band_time.py", "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

kind, N = args.case.split(":")
N = int(N)
n = N - 1
dx = 3.0 / n
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
dist = lambda c, r: torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r
if kind == "band":
    phi = dist((-0.15, -0.1, 0.05), 0.5).reshape(-1).contiguous()
    mask = (phi.abs() < 8.1 * dx).to(torch.int32)
else:
    phi = torch.minimum(dist((-0.6, 0.0, -0.2), 0.4), dist((0.6, 0.1, -0.1), 0.45)).reshape(-1).contiguous()
    mask = torch.ones_like(phi, dtype=torch.int32)
label = torch.full_like(mask, -7)
kappa = torch.full_like(phi, float("nan"))


def timed(fn):
    ms = []
    for it in range(args.repeats + 1):  # the first call is the warm-up: workspace, code objects
        torch.cuda.synchronize()
        t = time.perf_counter()
        rep = fn()
        torch.cuda.synchronize()
        if it:
            ms.append((time.perf_counter() - t) * 1e3)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep


row = {"case": kind, "N": N, "device": torch.cuda.get_device_name(0)}
med, spread, rep = timed(lambda: L.labelBand(phi, mask, n, n, n, label, side="both"))
assert rep.certified
row.update(label_ms=med, label_spread=spread, passes=rep.passes, ncomp=rep.ncomp, list_cells=rep.info[0], list_fraction=rep.info[0] / N ** 3,
           inside_components=rep.info[2], outside_components=rep.info[3], components=rep.components[:4].tolist())
med, spread, rep = timed(lambda: L.labelBand(phi, mask, n, n, n, label, side="both", comp_cap=0))
assert rep.certified and rep.ncomp == row["ncomp"]
row.update(label_no_table_ms=med, label_no_table_spread=spread, passes_no_table=rep.passes)


def curvature():
    try:
        return L.curvatureBand(phi, mask, n, n, n, dx, kappa, clamp=1.0).cells
    except L.LsfNaNError:  # (a kink of the field: the call has done all its work all the same)
        return row["list_cells"]


med, spread, cells = timed(curvature)
assert cells == row["list_cells"]
row.update(curvature_kappa_ms=med, curvature_kappa_spread=spread)
print(f"# {kind} {N}^3: label {row['label_ms']:.3f} ms ({row['label_no_table_ms']:.3f} ms without the table), {row['passes']} passes, "
      f"{row['ncomp']} components on {row['list_cells']} cells ({row['list_fraction']:.1%} of the grid); curvature "
      f"{row['curvature_kappa_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
