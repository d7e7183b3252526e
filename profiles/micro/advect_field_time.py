"""Time lsf_advect_field: ms per step at 256^3 and 512^3, both arithmetics, both schemes (profiles/advect_field_time.txt).

    python3 profiles/micro/advect_field_time.py [--steps 20] [--repeats 3] [--out FILE]

Case: the two-sphere field of levelsetfortran_amd.fields on N^3 points over [-1.5, 1.5]^3, a rigid rotation about the z axis plus a
speed along the normal that changes sign across the domain (all three velocity components and the speed present: the kernel with
every term), dt at CFL 0.5, device seam.  Each (N, arithmetic, scheme) is a child process of its own under its own time limit; the
next one is not started if one fails.  Per case: host clock around a call of `steps` steps that ends in a synchronise, after one
warm-up call; median and spread over `repeats` calls, divided by the steps; the bytes a step moves at the least (RK3: three stages
of 5 field reads of the stage input's planes counted once + 4 inputs + old phi + store) against that time.
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
CASES = [(n, a, s) for n in (256, 512) for a in ("strict", "fast") for s in ("rk3", "euler")]

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="N,arith,scheme (internal: one child process per case)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for n, a, s in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{n},{a},{s}", "--steps", str(args.steps), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {n},{a},{s} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": "lsf_advect_field, device seam, velocity + speed, CFL 0.5: ms per step (host clock around a call of "
                   f"{args.steps} steps, median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/advect_field_time.py", "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402
from levelsetfortran_amd import fields  # noqa: E402

N, arith, scheme = args.case.split(",")
N = int(N)
n = N - 1
phi0, dx = fields.two_sphere_phi0_device((N, N, N), "cuda")
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
one = torch.ones((N, N, N), dtype=torch.float64, device="cuda")
u, v, w = (-Y * one).reshape(-1), (X * one).reshape(-1), (0.1 * Z * one).reshape(-1)
speed = (0.3 * torch.cos(1.5 * X + 0.7 * Y - 0.9 * Z)).reshape(-1).contiguous()
del one
smax = float((u.abs() + v.abs() + w.abs() + speed.abs()).max())
dt = 0.5 * dx / smax
phi = torch.empty_like(phi0)


def call():
    phi.copy_(phi0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rep = L.advectField(phi, n, n, n, dx, dt, args.steps, velocity=(u, v, w), speed=speed, scheme=scheme, arith=arith)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / args.steps, rep


call()  # warm-up: workspace, code objects
ms = []
for _ in range(args.repeats):
    t, rep = call()
    ms.append(t)
stages = 3 if scheme == "rk3" else 1
fields_moved = stages * (1 + 4 + 1) + (2 if scheme == "rk3" else 0)  # per stage: input, u, v, w, speed, store; RK3: old phi twice
med = statistics.median(ms)
row = {"N": N, "arith": arith, "scheme": scheme, "ms_per_step": med, "samples": ms, "spread": (max(ms) - min(ms)) / med, "cfl": rep.cfl,
       "last_change": rep.change[-1], "min_gb_per_s": fields_moved * 8.0 * N ** 3 / (med * 1e-3) / 1e9, "device": torch.cuda.get_device_name(0)}
print(f"# {N}^3 {arith} {scheme}: {med:.3f} ms per step (spread {row['spread']:.1%}), cfl {rep.cfl:.3f}", file=sys.stderr, flush=True)
print(json.dumps(row))
