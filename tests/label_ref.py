"""The serial statement of lsf_label_band (include/lsf.h): a flood fill in ascending point-index order over the list, with the table
and the info of the contract.  numpy and plain Python, no device, no library.

    LIST       interior points (1..n-1 on each axis) with mask == 1
    CLASS      d = phi - iso once per cell; INSIDE d < 0, OUTSIDE everything else that is finite (d == 0 and -0.0 included)
    COMPONENT  labelled list cells linked through face neighbours (+-1 on one axis) of the same class, transitively
    label      the smallest point index i + (nx+1)*(j + (ny+1)*k) of the component; -1 at a list cell of a class `side` leaves out;
               untouched everywhere else

Fields are Fortran-ordered (nx+1, ny+1, nz+1) arrays, so the point index is the index into ravel(order="F").

`defect` plants one of four mistakes, for tests/test_label_band_cpu.py to show that a check notices each:
    "diagonal"  the 12 edge-diagonal neighbours link as well
    "zero"      d == 0 is taken as INSIDE
    "offlist"   two list cells link through one off-list cell between them on an axis
    "wall"      a wall point with mask == 1 is admitted to the list
"""
from collections import deque
from typing import NamedTuple

import numpy as np

SIDES = ("inside", "outside", "both")
COMP_LEN, INFO_LEN = 10, 8
FACES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGONALS = [(a, b, 0) for a in (1, -1) for b in (1, -1)] + [(a, 0, b) for a in (1, -1) for b in (1, -1)] + \
            [(0, a, b) for a in (1, -1) for b in (1, -1)]


class LabelResult(NamedTuple):
    label: np.ndarray  # int32, the caller's array with the list cells written
    ncomp: int
    comp: np.ndarray   # int64 (ncomp, 10), EVERY component, ascending root index: the call returns the first min(ncomp, comp_cap) rows
    info: tuple        # [0] list cells [1] labelled [2] INSIDE components [3] OUTSIDE components [4] 0 (passes: the call's own)
    #                    [5] 0 (certified) [6] list cells at -1 [7] 0


def list_of(mask, walls=False):
    """the LIST as a boolean field"""
    lst = np.asarray(mask) == 1
    if not walls:
        lst = lst.copy()
        lst[0, :, :] = lst[-1, :, :] = lst[:, 0, :] = lst[:, -1, :] = lst[:, :, 0] = lst[:, :, -1] = False
    return lst


def label_band(phi, mask, label, iso=0.0, side="inside", defect=None):
    """returns LabelResult; `label` (int32, phi's shape) is copied, never written.  Raises ValueError with the count when a list cell
    holds a non-finite phi - iso."""
    assert side in SIDES and defect in (None, "diagonal", "zero", "offlist", "wall")
    phi, mask = np.asarray(phi), np.asarray(mask)
    shape = phi.shape
    assert mask.shape == shape and label.shape == shape and label.dtype == np.int32
    lst = list_of(mask, walls=defect == "wall")
    with np.errstate(invalid="ignore"):
        d = phi - iso
    bad = int(np.count_nonzero(lst & ~np.isfinite(d)))
    if bad:
        raise ValueError(f"{bad} list cell(s) hold a non-finite phi - iso")
    with np.errstate(invalid="ignore"):
        inside = (d <= 0) if defect == "zero" else (d < 0)
    labelled = lst & {"inside": inside, "outside": ~inside, "both": np.ones(shape, bool)}[side]
    out = np.array(label, order="F", copy=True)
    out[lst] = -1
    n0, n1, n2 = shape
    steps = FACES + (DIAGONALS if defect == "diagonal" else [])
    seen = np.zeros(shape, bool)
    rows = []
    flat = lambda i, j, k: i + n0 * (j + n1 * k)
    # ascending point index: k slowest, i fastest
    for k, j, i in zip(*np.nonzero(labelled.transpose(2, 1, 0))):
        i, j, k = int(i), int(j), int(k)
        if seen[i, j, k]:
            continue
        root, cls = flat(i, j, k), bool(inside[i, j, k])
        seen[i, j, k] = True
        todo = deque([(i, j, k)])
        cells = edge = 0
        lo, hi = [i, j, k], [i, j, k]
        while todo:
            a, b, c = todo.popleft()
            out[a, b, c] = root
            cells += 1
            lo, hi = [min(lo[0], a), min(lo[1], b), min(lo[2], c)], [max(hi[0], a), max(hi[1], b), max(hi[2], c)]
            open_face = False
            for da, db, dc in FACES:
                x, y, z = a + da, b + db, c + dc
                if not (0 <= x < n0 and 0 <= y < n1 and 0 <= z < n2) or not lst[x, y, z]:
                    open_face = True
            edge += open_face
            reach = [(a + da, b + db, c + dc) for da, db, dc in steps]
            if defect == "offlist":
                reach += [(a + 2 * da, b + 2 * db, c + 2 * dc) for da, db, dc in FACES
                          if 0 <= a + da < n0 and 0 <= b + db < n1 and 0 <= c + dc < n2 and not lst[a + da, b + db, c + dc]]
            for x, y, z in reach:
                if 0 <= x < n0 and 0 <= y < n1 and 0 <= z < n2 and labelled[x, y, z] and not seen[x, y, z] and bool(inside[x, y, z]) == cls:
                    seen[x, y, z] = True
                    todo.append((x, y, z))
        rows.append([root, cells, -1 if cls else 1, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], edge])
    comp = np.array(rows, np.int64).reshape(len(rows), COMP_LEN)
    assert np.all(np.diff(comp[:, 0]) > 0)  # found in ascending order of root
    nlist, nlab = int(lst.sum()), int(labelled.sum())
    info = (nlist, nlab, int(np.count_nonzero(comp[:, 2] == -1)), int(np.count_nonzero(comp[:, 2] == 1)), 0, 0, nlist - nlab, 0)
    return LabelResult(out, len(rows), comp, info)
