"""Time lsf_cut_cells_band beside lsf_measure_band and lsf_curvature_band on the same list: ms per call at 256^3 and 512^3
(profiles/cut_cells_time.txt).

    python3 profiles/micro/cut_cells_time.py [--repeats 5] [--out FILE]

Case: that of profiles/micro/measure_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3
points over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx (phiSB of lsf_narrowband), device seam.  Timed: lsf_cut_cells_band with all seven
outputs and with volume only; lsf_measure_band (totals only) and lsf_curvature_band (all three outputs) on the same mask.
Each N is a child process of its own under its own time limit; the next one is not started if one fails.  Per figure: host clock
around one call that ends in a synchronise, after one warm-up call; median and spread over `repeats` calls.
A record, not a gate.  Prints one JSON line.
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
    out = {"what": "lsf_cut_cells_band (mask |phi| < 8.1 dx) beside lsf_measure_band and lsf_curvature_band on the same mask, device seam: ms per "
                   f"call (host clock around a call; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/cut_cells_time.py", "rows": rows}
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
kappa, gauss, gmag, vof, a0, a1, a2, b0, b1, b2 = (torch.full_like(phi, float("nan")) for _ in range(10))


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
row.update(measure_ms=med, measure_spread=spread, crossed=rep.crossed, measure_volume=rep.volume)
med, spread, rep = timed(lambda: L.cutCellsBand(phi, mask, n, n, n, dx, vof=vof, aperture=(a0, a1, a2), area_vector=(b0, b1, b2)))
row.update(cut_all_ms=med, cut_all_spread=spread, cut=rep.cut, full=rep.full, open=rep.open, clamped=rep.clamped, vof_min=rep.vof_min,
           volume=rep.volume)
assert rep.cells == row["list_cells"] and rep.cut == row["crossed"]
med, spread, rep = timed(lambda: L.cutCellsBand(phi, mask, n, n, n, dx))
row.update(cut_volume_only_ms=med, cut_volume_only_spread=spread)
assert rep.volume == row["volume"]
print(f"# {N}^3: cut cells {row['cut_all_ms']:.3f} ms (all outputs), {row['cut_volume_only_ms']:.3f} ms (volume only) on {row['list_cells']} cells "
      f"({row['list_fraction']:.1%} of the grid, {row['cut']} cut); measure {row['measure_ms']:.3f} ms; curvature "
      f"{row['curvature_all_three_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
