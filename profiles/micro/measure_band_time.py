"""Time lsf_measure_band beside lsf_curvature_band on the same mask and lsf_extract_surface on the same field: ms per call at 256^3
and 512^3 (profiles/measure_band_time.txt).

    python3 profiles/micro/measure_band_time.py [--repeats 5] [--out FILE]

Case: that of profiles/micro/curvature_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3
points over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx (phiSB of lsf_narrowband), device seam.  Timed: lsf_measure_band with the totals
only and with q (the gauss just computed, NaN off the list) and cell_area; lsf_curvature_band with all three outputs on the same mask;
extractSurface on the same field (lsf_extract_surface and lsf_extract_get_device: what a caller pays today before the host sums).
Each N is a child process of its own under its own time limit; the next one is not started if one fails.  Per figure: host clock
around one call that ends in a synchronise, after one warm-up call; median and spread over `repeats` calls.
A record, not a gate.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 240  # seconds per case
SIZES = (256, 512)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="N (internal: one child process per size)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for n in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(n), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {n} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": "lsf_measure_band (mask |phi| < 8.1 dx) beside lsf_curvature_band on the same mask and extractSurface on the same field, device "
                   f"seam: ms per call (host clock around a call; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/measure_band_time.py", "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

N = int(args.case)
n = N - 1
dx = 3.0 / n
LO = (-1.5, -1.5, -1.5)
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
phi = (torch.sqrt((X + 0.15) ** 2 + (Y + 0.1) ** 2 + (Z - 0.05) ** 2) - 0.5).reshape(-1).contiguous()
mask = (phi.abs() < 8.1 * dx).to(torch.int32)
kappa, gauss, gmag, cell = (torch.full_like(phi, float("nan")) for _ in range(4))


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


row = {"N": N, "device": torch.cuda.get_device_name(0)}
med, spread, rep = timed(lambda: L.curvatureBand(phi, mask, n, n, n, dx, kappa, gauss=gauss, gmag=gmag, clamp=1.0))
row.update(curvature_all_three_ms=med, curvature_all_three_spread=spread, list_cells=rep.cells, list_fraction=rep.cells / N ** 3)
med, spread, rep = timed(lambda: L.measureBand(phi, mask, n, n, n, dx, LO))
row.update(measure_ms=med, measure_spread=spread, crossed=rep.crossed, triangles=rep.triangles, open=rep.open, area=rep.area, volume=rep.volume,
           area_error=rep.area / (4 * math.pi * 0.25) - 1, volume_error=rep.volume / (4 / 3 * math.pi * 0.125) - 1)
assert rep.cells == row["list_cells"] and rep.open == 0
med, spread, rep = timed(lambda: L.measureBand(phi, mask, n, n, n, dx, LO, q=gauss, cell_area=cell))
row.update(measure_q_cell_ms=med, measure_q_cell_spread=spread, gauss_bonnet=rep.q_integral / (4 * math.pi))
med, spread, rep = timed(lambda: L.extractSurface(phi, n, n, n, dx, LO))
row.update(extract_ms=med, extract_spread=spread, extract_triangles=rep[2].triangles, extract_cells=rep[2].cells_crossed)
assert row["extract_triangles"] == row["triangles"] and row["extract_cells"] == row["crossed"]
print(f"# {N}^3: measure {row['measure_ms']:.3f} ms (totals), {row['measure_q_cell_ms']:.3f} ms (with q and cell_area) on {row['list_cells']} cells "
      f"({row['list_fraction']:.1%} of the grid, {row['crossed']} crossed); curvature {row['curvature_all_three_ms']:.3f} ms; "
      f"extractSurface {row['extract_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
