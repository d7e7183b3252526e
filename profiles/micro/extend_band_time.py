"""Time extendFieldBand beside extendField on the same field (profiles/extend_band_time.txt): the extension on a cell list, whose
cost follows the list, against the full-grid call, whose cost follows the grid.

    python3 profiles/micro/extend_band_time.py [--repeats 5] [--out FILE]

Field: the two-sphere distance of profiles/micro/extend_field_time.py (radii 0.5 and 0.35, the second one leaving through a wall) on
N^3 points of [-1.5, 1.5]^3, made on the device; frozen band 3.5 cells; mask |phi| < 8.1 dx; q = 1 + 0.5 x - 0.3 y + 0.2 z^2.
N = 256 and 512, device seam, each case a child process of its own under its own time limit; a case is not started if the one
before failed.  Host clock around calls that end in a synchronise, median of `repeats` calls after one warm-up.  extendFieldBand is
timed twice: to convergence, and with max_passes = 1 -- list build, plan, init, one pass and the count -- so that the difference
divided by the passes beyond the first is the cost of a pass and the rest is the fixed part of a call.  A record, not a gate: there
is no threshold.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMITS = {256: 180, 512: 420}  # seconds per case
BAND, WIDTH = 3.5, 8.1

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--case", type=int, choices=sorted(LIMITS), default=None)
args = ap.parse_args()

if args.case is None:
    rows = {}
    for N in sorted(LIMITS):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(N), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMITS[N])
        if r.returncode != 0:
            sys.exit(f"case {N} ended with status {r.returncode}: nothing more is started")
        rows[str(N)] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"what": "two-sphere distance on N^3 points, frozen band 3.5 cells, mask |phi| < 8.1 dx, device seam: extendFieldBand and "
                   f"extendField on the same field; host clock, ms per call (median of {args.repeats})",
           "command": "python3 profiles/micro/extend_band_time.py", **rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

N = args.case
n = N - 1
dx = 3.0 / n
ax = -1.5 + torch.arange(N, dtype=torch.float64, device="cuda") * dx
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # (nz+1, ny+1, nx+1): i is the unit-stride axis


def sphere(cx, cy, cz, r):
    return torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) - r


phi = torch.minimum(sphere(-0.3, 0.2, 0.1, 0.5), sphere(1.3, 0.6, -0.2, 0.35)).contiguous()
q0 = (1.0 + 0.5 * X - 0.3 * Y + 0.2 * Z * Z).expand_as(phi).contiguous()
mask = (phi.abs() < WIDTH * dx).to(torch.int32).contiguous()
del X, Y, Z


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def run(fn, fresh):
    work = fresh.clone()
    fn(work)  # warm-up: workspace, code objects
    ms = []
    for _ in range(args.repeats):
        work.copy_(fresh)
        t, rep = timed(lambda: fn(work))
        ms.append(t)
    return ms, rep


t_band, (_, rep_b) = run(lambda a: L.extendFieldBand(a, phi, mask, dx, band=BAND), q0)
t_one, (_, rep_1) = run(lambda a: L.extendFieldBand(a, phi, mask, dx, band=BAND, max_passes=1), q0)
t_full, rep_f = run(lambda a: L.extendField(a, phi, n, n, n, dx, band=BAND), q0)
assert rep_b.converged and rep_1.passes == 1 and rep_1.cells == rep_b.cells
band_ms, one_ms, full_ms = statistics.median(t_band), statistics.median(t_one), statistics.median(t_full)
per_pass = (band_ms - one_ms) / max(rep_b.passes - 1, 1)
row = {"band_ms": band_ms, "band_ms_samples": t_band, "band_passes": rep_b.passes, "band_trace": rep_b.trace, "band_cells": rep_b.cells,
       "band_frozen": rep_b.frozen, "band_unreached": rep_b.unreached, "band_one_pass_ms": one_ms, "band_one_pass_ms_samples": t_one,
       "band_ms_per_pass": per_pass, "band_fixed_ms": one_ms - per_pass, "band_fixed_share": (one_ms - per_pass) / band_ms,
       "band_ms_per_pass_overall": band_ms / rep_b.passes,
       "full_ms": full_ms, "full_ms_samples": t_full, "full_rounds": rep_f.rounds, "full_ms_per_round": full_ms / rep_f.rounds,
       "full_frozen_points": rep_f.frozen_points, "full_converged": rep_f.converged, "full_over_band": full_ms / band_ms,
       "list_share_of_grid": rep_b.cells / float(N) ** 3, "device": torch.cuda.get_device_name(0), "grid": [N, N, N]}
print(f"# {N}^3: extendFieldBand {band_ms:.3f} ms / {rep_b.passes} passes on {rep_b.cells} cells ({per_pass:.4f} ms per pass, "
      f"{one_ms - per_pass:.3f} ms fixed); extendField {full_ms:.2f} ms / {rep_f.rounds} rounds", file=sys.stderr, flush=True)
print(json.dumps(row))
