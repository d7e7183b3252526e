"""Time lsf_extract_surface: ms per call at 256^3 and 512^3 (profiles/extract_surface_time.txt).

    python3 profiles/micro/extract_surface_time.py [--repeats 5] [--out FILE]

Case: the two-sphere field of levelsetfortran_amd.fields on N^3 points over [-1.5, 1.5]^3, device seam: one call of extractSurface
(extraction + get, the mesh left in device tensors).  Each N is a child process of its own under its own time limit; the next one is
not started if one fails.  Per case: host clock around a call that ends in a synchronise, after one warm-up call; median and spread
over `repeats` calls; the bytes a call moves at the least (the field once for the count, 2 + 2 + 2 bytes per point written and read
by the sums and the scatter, 8 written, and mask, corner byte and offsets read once more by the emit) against that time.
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
CASES = [256, 512]

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="N (internal: one child process per case)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for n in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(n), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {n} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": f"lsf_extract_surface + lsf_extract_get_device, two spheres: ms per call (host clock, median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/extract_surface_time.py", "rows": rows}
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

N = int(args.case)
n = N - 1
phi, dx = fields.two_sphere_phi0_device((N, N, N), "cuda")
lo = (-1.5, -1.5, -1.5)


def call():
    torch.cuda.synchronize()
    t = time.perf_counter()
    X, E, info = L.extractSurface(phi, n, n, n, dx, lo)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, info


call()  # warm-up: workspace, code objects
ms = []
for _ in range(args.repeats):
    t, info = call()
    ms.append(t)
med = statistics.median(ms)
bytes_moved = (8 + 2 + 2 + 2 + 8 + 10) * N ** 3 + 24 * info.nodes + 12 * info.triangles
row = {"N": N, "ms_per_call": med, "samples": ms, "spread": (max(ms) - min(ms)) / med, "nodes": info.nodes, "triangles": info.triangles,
       "cells_crossed": info.cells_crossed, "min_gb_per_s": bytes_moved / (med * 1e-3) / 1e9, "device": torch.cuda.get_device_name(0)}
print(f"# {N}^3: {med:.3f} ms per call (spread {row['spread']:.1%}), {info.nodes} nodes, {info.triangles} triangles", file=sys.stderr, flush=True)
print(json.dumps(row))
