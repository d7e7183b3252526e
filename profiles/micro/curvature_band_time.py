"""Time lsf_curvature_band beside one Euler step of lsf_advect_field_band on the same sphere and mask: ms per call at 256^3 and 512^3
(profiles/curvature_band_time.txt).

    python3 profiles/micro/curvature_band_time.py [--repeats 5] [--out FILE]

Case: that of profiles/micro/advect_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3 points
over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx (phiSB of lsf_narrowband), device seam.  Timed: lsf_curvature_band with kappa only and
with all three outputs, clamp = 1, and beside them ONE Euler step of lsf_advect_field_band (STRICT) on the same mask with the kappa
just computed as its speed, dt = 0.25 dx^2 -- a call that builds the same list and makes one launch over it, plus a copy of the field.
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
    out = {"what": "lsf_curvature_band (mask |phi| < 8.1 dx, clamp 1) beside one Euler step of lsf_advect_field_band on the same mask, device "
                   f"seam: ms per call (host clock around a call; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/curvature_band_time.py", "rows": rows}
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
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
phi0 = (torch.sqrt((X + 0.15) ** 2 + (Y + 0.1) ** 2 + (Z - 0.05) ** 2) - 0.5).reshape(-1).contiguous()
mask = (phi0.abs() < 8.1 * dx).to(torch.int32)
phi = phi0.clone()
kappa, gauss, gmag = (torch.full_like(phi0, float("nan")) for _ in range(3))
dt = 0.25 * dx * dx  # |kappa| <= 1/dx: CFL <= 0.25


def curvature(all_three):
    return L.curvatureBand(phi0, mask, n, n, n, dx, kappa, gauss=gauss if all_three else None, gmag=gmag if all_three else None, clamp=1.0)


def euler_step():
    return L.advectFieldBand(phi, mask, n, n, n, dx, dt, 1, speed=kappa, scheme="euler", arith="strict")


def timed(fn, before=None):
    ms = []
    for it in range(args.repeats + 1):  # the first call is the warm-up: workspace, code objects
        if before:
            before()
        torch.cuda.synchronize()
        t = time.perf_counter()
        rep = fn()
        torch.cuda.synchronize()
        if it:
            ms.append((time.perf_counter() - t) * 1e3)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep


row = {"N": N, "device": torch.cuda.get_device_name(0)}
med, spread, rep = timed(lambda: curvature(False))
row.update(kappa_only_ms=med, kappa_only_spread=spread, list_cells=rep.cells, list_fraction=rep.cells / N ** 3, clamped=rep.clamped,
           degenerate=rep.degenerate, kappa_max_dx=rep.kappa_max * dx)
med, spread, rep = timed(lambda: curvature(True))
row.update(all_three_ms=med, all_three_spread=spread)
med, spread, rep = timed(euler_step, before=lambda: phi.copy_(phi0))
assert rep.steps == 1 and rep.cells == row["list_cells"]
row.update(advect_band_euler_step_ms=med, advect_band_euler_step_spread=spread, advect_cfl=rep.cfl)
print(f"# {N}^3: curvature {row['kappa_only_ms']:.3f} ms (kappa), {row['all_three_ms']:.3f} ms (all three) on {row['list_cells']} cells "
      f"({row['list_fraction']:.1%} of the grid); one Euler step of the band transport {row['advect_band_euler_step_ms']:.3f} ms",
      file=sys.stderr, flush=True)
print(json.dumps(row))
