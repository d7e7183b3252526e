"""Time lsf_evolve_band_curv beside lsf_evolve_band on the same inputs and beside the loop of public calls it replaces: ms per step at
256^3 and 512^3, STRICT, RK3, 2 sweeps (profiles/evolve_band_curv_time.txt).

    python3 profiles/micro/evolve_band_curv_time.py [--steps 20] [--repeats 3] [--out FILE]

Case: that of profiles/micro/evolve_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3 points
over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx, a rigid rotation about the z axis plus a speed along the normal `a` that changes sign, dt
at CFL 0.5 over the whole grid -- with b = 0.15 dx^2 / dt, clamp 1, core 3, ring 3, 2 sweeps, h = 0.5 dx, a check after every step,
device seam.
  curv    ONE lsf_evolve_band_curv call of `steps` steps with bcurv = b, the velocity and speed = a
  evolve  ONE lsf_evolve_band call of `steps` steps with the velocity and speed = a: the parent's stage kernel on the same inputs,
          the baseline
  loop    what `curv` replaces: per step lsf_curvature_band(clamp 1), speed = a - b*kappa in torch, lsf_evolve_band(steps = 1) with
          the velocity and that speed.  (It is not the same scheme: kappa is frozen over the three stages and upwinded; the fields
          differ.)
The steps run, the rebuilds and the flips of each are recorded beside the times.
Each N is a child process of its own under its own time limit; the next one is not started if one fails.  Host clock around the work,
which ends in a synchronise, after one warm-up; median and spread over `repeats`, divided by the steps run.
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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="N (internal: one child process per case)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for n in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(n), "--steps", str(args.steps), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {n} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": "lsf_evolve_band_curv (one call, bcurv > 0, a velocity and a speed) against lsf_evolve_band (one call, the same inputs) and a loop of "
                   "lsf_curvature_band + (speed = a - b*kappa) + lsf_evolve_band(steps=1), mask |phi| < 8.1 dx, device seam, RK3, STRICT, 2 "
                   f"sweeps, velocity + speed, CFL 0.5, b dt/dx^2 = 0.15: ms per step over {args.steps} steps (host clock; median of {args.repeats} after a warm-up)",
           "command": "python3 profiles/micro/evolve_band_curv_time.py", "rows": rows}
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
mask0 = (phi0.abs() < 8.1 * dx).to(torch.int32)
one = torch.ones((N, N, N), dtype=torch.float64, device="cuda")
vel = tuple(t.reshape(-1) for t in (-Y * one, X * one, 0.1 * Z * one))
a = (0.3 * torch.cos(1.5 * X + 0.7 * Y - 0.9 * Z)).reshape(-1).contiguous()
del one
dt = 0.5 * dx / float((vel[0].abs() + vel[1].abs() + vel[2].abs() + a.abs()).max())
b = 0.15 * dx * dx / dt
phi, mask = torch.empty_like(phi0), torch.empty_like(mask0)
kappa, speed = torch.zeros_like(phi0), torch.empty_like(phi0)
KW = dict(arith="strict", core=3.0, ring=3, reinit_sweeps=2, h=0.5 * dx, check_every=1)


def run(which, steps):
    phi.copy_(phi0)
    mask.copy_(mask0)
    kappa.zero_()
    torch.cuda.synchronize()
    t = time.perf_counter()
    if which == "curv":
        rep = L.evolveBandCurv(phi, mask, n, n, n, dx, dt, steps, curvature=b, velocity=vel, speed=a, clamp=1.0, **KW)
        done = rep.steps
    elif which == "evolve":
        rep = L.evolveBand(phi, mask, n, n, n, dx, dt, steps, velocity=vel, speed=a, **KW)
        done = rep.steps
    else:
        done = 0
        for _ in range(steps):
            L.curvatureBand(phi, mask, n, n, n, dx, kappa, clamp=1.0)
            torch.sub(a, kappa, alpha=b, out=speed)
            rep = L.evolveBand(phi, mask, n, n, n, dx, dt, 1, velocity=vel, speed=speed, **KW)
            done += rep.steps
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / max(done, 1), rep, done


def timed(which, steps):
    run(which, steps)  # warm-up: workspace, code objects
    ms = []
    for _ in range(args.repeats):
        t, rep, done = run(which, steps)
        ms.append(t)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep, done


row = {"N": N, "arith": "strict", "scheme": "rk3", "sweeps": 2, "steps": args.steps, "device": torch.cuda.get_device_name(0), "bcurv": b, "dt": dt}
med, spread, rep, done = timed("curv", args.steps)
row.update(curv_ms_per_step=med, curv_spread=spread, steps_done=done, rebuilds=rep.rebuilds, flips=rep.flips, list_cells=rep.cells,
           list_fraction=rep.cells / N ** 3, cfl=rep.cfl, diffusion=rep.diffusion, margin_dx=rep.margin / dx)
med, spread, rep, done = timed("evolve", args.steps)
row.update(evolve_ms_per_step=med, evolve_spread=spread, evolve_steps_done=done, evolve_rebuilds=rep.rebuilds, evolve_flips=rep.flips, curv_over_evolve=row["curv_ms_per_step"] / med)
med, spread, rep, done = timed("loop", args.steps)
row.update(loop_ms_per_step=med, loop_spread=spread, loop_steps_done=done, loop_over_curv=med / row["curv_ms_per_step"])
print(f"# {N}^3 strict: curv {row['curv_ms_per_step']:.3f} ms per step ({row['rebuilds']} rebuilds, {row['list_fraction']:.1%} of the grid), "
      f"evolve {row['evolve_ms_per_step']:.3f}, loop of public calls {row['loop_ms_per_step']:.3f}", file=sys.stderr, flush=True)
print(json.dumps(row))
