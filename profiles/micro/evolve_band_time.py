"""Time lsf_evolve_band against the loop of public calls it replaces: ms per step at 256^3 and 512^3, both arithmetics, RK3, 2 sweeps
(profiles/evolve_band_time.txt).

    python3 profiles/micro/evolve_band_time.py [--steps 20] [--repeats 3] [--out FILE]

Case: that of profiles/micro/advect_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3 points
over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx, a rigid rotation about the z axis plus a speed along the normal that changes sign, dt at
CFL 0.5 over the whole grid, device seam.  `evolve`: ONE lsf_evolve_band call of `steps` steps (core 3, ring 3, 2 sweeps, h = 0.5 dx,
a check after every step).  `loop`: the same steps with the calls that existed before it, per step one lsf_advect_field_band step and
one lsf_reinit_band(iter = 1, tol = 0) on the same mask -- each of which builds the list from the mask and copies the field.  Without a
rebuild both compute the same field (tests/test_gpu_evolve_band.py); the rebuild count is recorded beside the times.
`evolve_core6`: the evolve call again with core = 6, so that the margin (8.1 dx at the start) falls below core dx within the steps
and the list is rebuilt: what a rebuild adds.  Each (N, arithmetic) is a child process of its own under its own time limit; the next
one is not started if one fails.  Host clock around the work, which ends in a synchronise, after one warm-up; median and spread over
`repeats`, divided by the steps.
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
    out = {"what": "lsf_evolve_band (one call) against a loop of lsf_advect_field_band(1 step) + lsf_reinit_band(iter=1, tol=0), mask "
                   f"|phi| < 8.1 dx, device seam, RK3, 2 sweeps, velocity + speed, CFL 0.5: ms per step over {args.steps} steps (host clock; "
                   f"median of {args.repeats} after a warm-up)",
           "command": "python3 profiles/micro/evolve_band_time.py", "rows": rows}
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
mask0 = (phi0.abs() < 8.1 * dx).to(torch.int32)
one = torch.ones((N, N, N), dtype=torch.float64, device="cuda")
u, v, w = (-Y * one).reshape(-1), (X * one).reshape(-1), (0.1 * Z * one).reshape(-1)
speed = (0.3 * torch.cos(1.5 * X + 0.7 * Y - 0.9 * Z)).reshape(-1).contiguous()
del one
smax = float((u.abs() + v.abs() + w.abs() + speed.abs()).max())
dt = 0.5 * dx / smax
phi, mask = torch.empty_like(phi0), torch.empty_like(mask0)


def run(evolve, steps, core=3.0):
    phi.copy_(phi0)
    mask.copy_(mask0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    if evolve:
        rep = L.evolveBand(phi, mask, n, n, n, dx, dt, steps, velocity=(u, v, w), speed=speed, arith=arith, core=core, ring=3, reinit_sweeps=2,
                           h=0.5 * dx, check_every=1)
    else:
        for _ in range(steps):
            rep = L.advectFieldBand(phi, mask, n, n, n, dx, dt, 1, velocity=(u, v, w), speed=speed, arith=arith)
            L.reinitBand(phi, mask, n, n, n, 1, dx, 0.5 * dx, tol=0.0, arith=arith)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps, rep


def timed(evolve, steps, core=3.0):
    run(evolve, steps, core)  # warm-up: workspace, code objects
    ms = []
    for _ in range(args.repeats):
        t, rep = run(evolve, steps, core)
        ms.append(t)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep


row = {"N": N, "arith": arith, "scheme": "rk3", "sweeps": 2, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
med, spread, rep = timed(True, args.steps)
row.update(evolve_ms_per_step=med, evolve_spread=spread, steps_done=rep.steps, rebuilds=rep.rebuilds, entered=rep.entered, flips=rep.flips,
           list_cells=rep.cells, list_fraction=rep.cells / N ** 3, margin_dx=rep.margin / dx)
evolved = phi.clone()
med, spread, rep = timed(False, args.steps)
row.update(loop_ms_per_step=med, loop_spread=spread, loop_over_evolve=med / row["evolve_ms_per_step"])
row["same_field"] = bool(torch.equal(evolved, phi))  # expected without a rebuild (STRICT and FAST alike: the same kernels in the same order)
med, spread, rep = timed(True, args.steps, 6.0)
row.update(evolve_core6_ms_per_step=med, evolve_core6_spread=spread, core6_steps_done=rep.steps, core6_rebuilds=rep.rebuilds,
           core6_entered=rep.entered, core6_flips=rep.flips, core6_list_cells=rep.cells)
print(f"# {N}^3 {arith}: core 6: {med:.3f} ms per step with {rep.rebuilds} rebuild(s), {rep.entered} cells entered", file=sys.stderr, flush=True)
print(f"# {N}^3 {arith}: evolve {row['evolve_ms_per_step']:.3f} ms per step ({row['rebuilds']} rebuilds, {row['list_fraction']:.1%} of the grid), "
      f"loop of public calls {row['loop_ms_per_step']:.3f}; same field: {row['same_field']}", file=sys.stderr, flush=True)
print(json.dumps(row))
