"""Time lsf_advect_field_band against lsf_advect_field: ms per step at 256^3 and 512^3, both arithmetics, RK3
(profiles/advect_band_time.txt).

    python3 profiles/micro/advect_band_time.py [--steps 20] [--repeats 3] [--out FILE]

Case: the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3 points over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx
(phiSB of lsf_narrowband), a rigid rotation about the z axis plus a speed along the normal that changes sign across the domain (the
kernel with every term), dt at CFL 0.5 over the whole grid, device seam.  Both calls move the same field with the same inputs.  Each
(N, arithmetic) is a child process of its own under its own time limit; the next one is not started if one fails.  Per case: host
clock around a call of `steps` steps that ends in a synchronise, after one warm-up call; median and spread over `repeats` calls,
divided by the steps.  The band call's time includes what it does once per call (the list build, two copies of the field, the edge and
closing passes), so a call of ONE step is timed too: that is what a loop "advect one step, reinit, rebuild the mask" pays.
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
CASES = [(n, a) for n in (256, 512) for a in ("strict", "fast")]

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="N,arith (internal: one child process per case)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for n, a in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{n},{a}", "--steps", str(args.steps), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {n},{a} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": "lsf_advect_field_band (mask |phi| < 8.1 dx) against lsf_advect_field, device seam, RK3, velocity + speed, CFL 0.5: ms per "
                   f"step (host clock around a call of {args.steps} steps, and of 1 step; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/advect_band_time.py", "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

N, arith = args.case.split(",")
N = int(N)
n = N - 1
dx = 3.0 / n
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
phi0 = (torch.sqrt((X + 0.15) ** 2 + (Y + 0.1) ** 2 + (Z - 0.05) ** 2) - 0.5).reshape(-1).contiguous()
mask = (phi0.abs() < 8.1 * dx).to(torch.int32)
one = torch.ones((N, N, N), dtype=torch.float64, device="cuda")
u, v, w = (-Y * one).reshape(-1), (X * one).reshape(-1), (0.1 * Z * one).reshape(-1)
speed = (0.3 * torch.cos(1.5 * X + 0.7 * Y - 0.9 * Z)).reshape(-1).contiguous()
del one
smax = float((u.abs() + v.abs() + w.abs() + speed.abs()).max())
dt = 0.5 * dx / smax
phi = torch.empty_like(phi0)


def call(band, steps):
    phi.copy_(phi0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    if band:
        rep = L.advectFieldBand(phi, mask, n, n, n, dx, dt, steps, velocity=(u, v, w), speed=speed, arith=arith)
    else:
        rep = L.advectField(phi, n, n, n, dx, dt, steps, velocity=(u, v, w), speed=speed, arith=arith)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps, rep


def timed(band, steps):
    call(band, steps)  # warm-up: workspace, code objects
    ms = []
    for _ in range(args.repeats):
        t, rep = call(band, steps)
        ms.append(t)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep


row = {"N": N, "arith": arith, "scheme": "rk3", "steps": args.steps, "device": torch.cuda.get_device_name(0)}
for name, band in (("band", True), ("full", False)):
    for label, steps in (("", args.steps), ("_one_step_call", 1)):
        med, spread, rep = timed(band, steps)
        row[f"{name}{label}_ms_per_step"], row[f"{name}{label}_spread"] = med, spread
    if band:
        row.update(list_cells=rep.cells, list_fraction=rep.cells / N ** 3, edge_cells=rep.edge_cells, cfl_on_list=rep.cfl)
row["full_over_band"] = row["full_ms_per_step"] / row["band_ms_per_step"]
row["full_over_band_one_step_call"] = row["full_one_step_call_ms_per_step"] / row["band_one_step_call_ms_per_step"]
print(f"# {N}^3 {arith}: band {row['band_ms_per_step']:.3f} ms per step ({row['list_fraction']:.1%} of the grid), full grid "
      f"{row['full_ms_per_step']:.3f}; calls of one step: {row['band_one_step_call_ms_per_step']:.3f} against "
      f"{row['full_one_step_call_ms_per_step']:.3f}", file=sys.stderr, flush=True)
print(json.dumps(row))
