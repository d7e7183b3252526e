"""Time meshDistance(width 8.5) + distanceFill against the route to a whole-grid distance that existed before: lsf_reinit from the
same clamped field (profiles/distance_fill_time.txt).

    python3 profiles/micro/distance_fill_time.py [--repeats 3] [--iter 20000] [--out FILE]

Case: cube40 (18 276 triangles) at 256^3, dx = 2 / 233.5 and 10 pad cells as in tests/golden/make_golden_c2.py (BASELINE
configuration 2), device seam.  Two steps, each a child process of its own under its own time limit; the second is not started if
the first fails:
  fill     meshDistance(width 8.5), then distanceFill(band 8.5) on a copy of that field: host clock around calls that end in a
           synchronise, median and spread of `repeats` calls after one warm-up; rounds, trace, frozen points; the largest error
           against the closed-form box distance, in dx.
  reinit   ONE lsf_reinit (exact ordering, STRICT arithmetic, the reference's h, tol 1e-5) from the clamped field: sweeps to the
           stop and the time of the call.
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
LIMITS = {"fill": 240, "reinit": 420}  # seconds per step

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--iter", type=int, default=20000)
ap.add_argument("--out", default=None)
ap.add_argument("--step", choices=sorted(LIMITS), default=None)
args = ap.parse_args()

if args.step is None:
    rows = {}
    for step in ("fill", "reinit"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--repeats", str(args.repeats), "--iter", str(args.iter)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMITS[step])
        if r.returncode != 0:
            sys.exit(f"step {step} ended with status {r.returncode}: nothing more is started")
        rows[step] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"what": "cube40 at 256^3 (dx = 2/233.5, 10 pad cells), device seam: meshDistance(width 8.5) + distanceFill(band 8.5) against "
                   "lsf_reinit (GS, STRICT, reference h, tol 1e-5) from the same clamped field; host clock, times in ms, "
                   f"median of {args.repeats} calls for the fill",
           "command": "python3 profiles/micro/distance_fill_time.py", **rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import levelsetfortran_amd as L  # noqa: E402
import stl_io  # noqa: E402

WIDTH = 8.5
DX = 2.0 / 233.5
s = np.load(os.path.join(ROOT, "tests", "golden", "surfaces.npz"))
X, E = s["cube40_surfX"].astype(np.float64), s["cube40_surfElem"]
n, xLo, mn, mx = stl_io.grid_from_surface(X, dx=DX, dd=10)
assert tuple(n) == (255, 255, 255), n
npts = (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
clamped = torch.empty(npts, dtype=torch.float64, device="cuda")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def mesh():
    return L.meshDistance(clamped, n[0], n[1], n[2], DX, xLo, X, E, width=WIDTH)


if args.step == "fill":
    phi = torch.empty_like(clamped)
    mesh()
    phi.copy_(clamped)
    L.distanceFill(phi, n[0], n[1], n[2], DX, band=WIDTH)  # warm-up: workspace, code objects
    t_mesh, t_fill = [], []
    for _ in range(args.repeats):
        t_mesh.append(timed(mesh)[0])
        phi.copy_(clamped)
        ms, rep = timed(lambda: L.distanceFill(phi, n[0], n[1], n[2], DX, band=WIDTH))
        t_fill.append(ms)
    # the closed-form distance of the fixture's box, plane by plane on the device
    ax = [torch.tensor(xLo[a] + np.arange(n[a] + 1) * DX, device="cuda") for a in range(3)]
    q = [torch.maximum(float(mn[a]) - ax[a], ax[a] - float(mx[a])) for a in range(3)]
    qx, qy, qz = q[0][None, None, :], q[1][None, :, None], q[2][:, None, None]
    outside = torch.sqrt(qx.clamp(min=0) ** 2 + qy.clamp(min=0) ** 2 + qz.clamp(min=0) ** 2)
    inside = torch.maximum(torch.maximum(qx, qy), qz)
    ref = torch.where((qx <= 0) & (qy <= 0) & (qz <= 0), inside, outside).reshape(-1)
    row = {"mesh_ms": statistics.median(t_mesh), "mesh_ms_samples": t_mesh, "fill_ms": statistics.median(t_fill), "fill_ms_samples": t_fill,
           "fill_spread": (max(t_fill) - min(t_fill)) / statistics.median(t_fill), "rounds": rep.rounds, "changed": rep.changed,
           "frozen_points": rep.frozen_points, "converged": rep.converged, "max_error_dx": float((phi - ref).abs().max() / DX),
           "launches_per_round": 8 * (-(-(n[0] + 1) // 32) + -(-(n[1] + 1) // 8) + -(-(n[2] + 1) // 8) - 2),
           "device": torch.cuda.get_device_name(0), "grid": [v + 1 for v in n]}
    print(f"# meshDistance {row['mesh_ms']:.2f} ms + distanceFill {row['fill_ms']:.2f} ms ({rep.rounds} rounds, trace {rep.changed}), "
          f"max error {row['max_error_dx']:.2f} dx", file=sys.stderr, flush=True)
else:
    ext = mx - mn
    h = 0.1 * (DX / np.sqrt(ext @ ext))  # set3d.f90:301-305
    mesh()
    ms, rep = timed(lambda: L.reinit(clamped, None, None, n[0], n[1], n[2], args.iter, DX, h, order="gs", arith="strict"))
    row = {"reinit_sweeps": rep.count, "reinit_converged": rep.converged, "reinit_ms": ms, "h": float(h)}
    print(f"# lsf_reinit from the clamped field: {rep.count} sweeps in {ms:.0f} ms{'' if rep.converged else ' (NOT converged)'}",
          file=sys.stderr, flush=True)
print(json.dumps(row))
