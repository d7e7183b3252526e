"""Time lsf_mesh_distance_device against lsf_phi0_device and count the sweeps lsf_reinit needs from each start
(profiles/mesh_distance_time.txt).

    python3 profiles/micro/mesh_distance_time.py [--repeats 5] [--iter 20000] [--out FILE]

Case: cube40 (18 276 triangles) at 256^3, dx = 2 / 233.5 and 10 pad cells as in tests/golden/make_golden_c2.py (BASELINE
configuration 2), device seam.  Per start -- phi0Init as it stands, meshDistance with width 3.5 and with width 8 -- the time of the
initialisation call (host clock around a call that ends in a synchronise: host-side mesh preparation and table upload included;
median and spread of `repeats` calls after one warm-up), then ONE lsf_reinit from that field (exact ordering, STRICT arithmetic,
the reference's h, tol 1e-5): sweeps to the stop and the time of the call.  A record, not a gate.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import levelsetfortran_amd as L  # noqa: E402
import stl_io  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--iter", type=int, default=20000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

DX = 2.0 / 233.5
s = np.load(os.path.join(ROOT, "tests", "golden", "surfaces.npz"))
X, E = s["cube40_surfX"].astype(np.float64), s["cube40_surfElem"]
n, xLo, mn, mx = stl_io.grid_from_surface(X, dx=DX, dd=10)
assert tuple(n) == (255, 255, 255), n
ext = mx - mn
h = 0.1 * (DX / np.sqrt(ext @ ext))  # set3d.f90:301-305
npts = (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
phi = torch.empty(npts, dtype=torch.float64, device="cuda")

starts = [("phi0Init", lambda: L.phi0Init(phi, n[0], n[1], n[2], DX, xLo, mn, mx, X, E)),
          ("meshDistance width 3.5", lambda: L.meshDistance(phi, n[0], n[1], n[2], DX, xLo, X, E, width=3.5)),
          ("meshDistance width 8", lambda: L.meshDistance(phi, n[0], n[1], n[2], DX, xLo, X, E, width=8.0))]
rows = []
for name, init in starts:
    info = init()  # warm-up: workspace, code objects
    ts = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        init()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    rep = L.reinit(phi, None, None, n[0], n[1], n[2], args.iter, DX, h, order="gs", arith="strict")
    torch.cuda.synchronize()
    row = {"start": name, "init_ms": statistics.median(ts), "init_ms_samples": ts, "init_spread": (max(ts) - min(ts)) / statistics.median(ts),
           "tube_points": info.tube_points if info is not None else None, "reinit_sweeps": rep.count, "reinit_converged": rep.converged,
           "reinit_ms": (time.perf_counter() - t) * 1e3}
    rows.append(row)
    print(f"# {name}: init {row['init_ms']:.3f} ms (spread {100 * row['init_spread']:.0f} %), reinit {rep.count} sweeps in {row['reinit_ms']:.0f} ms"
          f"{'' if rep.converged else ' (NOT converged)'}", file=sys.stderr, flush=True)

out = {"what": "cube40 at 256^3 (dx = 2/233.5, 10 pad cells), device seam: initialisation call, then lsf_reinit (GS, STRICT, reference h, tol 1e-5) "
               f"from that field; init time = median of {args.repeats} calls, host clock",
       "command": "python3 profiles/micro/mesh_distance_time.py", "device": torch.cuda.get_device_name(0), "grid": [v + 1 for v in n],
       "triangles": int(len(E)), "dx": DX, "h": float(h), "rows": rows}
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
