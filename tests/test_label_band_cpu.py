"""tests/label_ref.py, the serial statement of lsf_label_band (include/lsf.h), on the CPU: known counts on the constructed fields of
tests/label_cases.py, agreement with scipy.ndimage.label where the mask is all ones, and four planted defects that each fail a check.
No device, no library."""
import numpy as np
import pytest

import label_cases as C
import label_ref as L


def _run(case, side, defect=None):
    phi, mask, npts, iso = C.geometry(case)
    return L.label_band(phi, mask, C.prefill(npts), iso, side, defect=defect)


def _classes(case, side):
    r = _run(case, side)
    return r.info[2], r.info[3]


def test_known_counts():
    assert _run("onecell", "both").comp.tolist() == [[4 + 10 * (4 + 10 * 4), 1, -1, 4, 4, 4, 4, 4, 4, 1]]
    assert _run("onecell", "outside").ncomp == 0 and _run("onecell", "outside").info == (1, 0, 0, 0, 0, 0, 1, 0)
    r = _run("small", "both")
    assert r.info[:4] == (246, 246, 1, 1) and sorted(r.comp[:, 1]) == [24, 222]  # the inner shell and the outer shell
    assert _classes("two", "both") == (2, 1) and _classes("two", "inside") == (2, 0) and _classes("two", "outside") == (0, 1)
    two = _run("two", "inside")
    assert (two.comp[:, 9] == 0).all()  # both balls are closed inside the list
    assert _classes("hollow", "both") == (1, 2)
    h = _run("hollow", "outside")
    assert h.comp[:, 9].tolist()[1] == 0 and h.comp[0, 9] > 0  # the cavity is closed, the exterior reaches the walls
    assert (_run("hollow_band", "both").comp[:, 9] > 0).all() and _classes("hollow_band", "both") == (1, 2)
    for v in ("snake_end", "snake_mid"):
        r = _run(v, "inside")
        assert r.ncomp == 1 and r.comp[0, :2].tolist() == [1 + 17 * (1 + 17 * 1), C.SNAKE_CELLS]
    r = _run("checker", "both")
    assert r.ncomp == 10 * 9 * 8 == r.info[1] and (r.comp[:, 1] == 1).all() and r.info[2] == r.info[3] == 360
    assert _run("values", "both").info[0] == 184
    # iso: 0.25 planted inside is an OUTSIDE cell of its own, one ulp above too, one ulp below stays INSIDE; outside likewise
    assert _classes("iso", "both") == (2, 3) and _classes("negzero", "both") == (1, 3)


def test_the_snake_is_one_path():
    for v in ("end", "mid"):
        path = C.snake_path(v)
        cells = set(path)
        assert len(path) == len(cells) == C.SNAKE_CELLS
        assert all(sum(abs(a - b) for a, b in zip(p, q)) == 1 for p, q in zip(path, path[1:]))  # consecutive cells are face neighbours
        deg = [sum((p[0] + d[0], p[1] + d[1], p[2] + d[2]) in cells for d in L.FACES) for p in path]
        assert deg[0] == deg[-1] == 1 and set(deg[1:-1]) == {2}  # ... and nothing else touches: the diameter is the cell count
        assert min(path, key=lambda p: p[0] + 17 * (p[1] + 17 * p[2])) == (1, 1, 1)
    assert C.snake_path("end").index((1, 1, 1)) == 0 and C.snake_path("mid").index((1, 1, 1)) == 126
    # it crosses every brick boundary (8 x 8 x 4 points) and, in the brick-sorted list of 1575 cells, several chunks of 256
    bricks = {(p[0] // 8, p[1] // 8, p[2] // 4) for p in C.snake_path("end")}
    assert len(bricks) == 2 * 2 * 2  # every brick that holds an interior point


def test_label_is_written_at_list_cells_only():
    for case in C.CASES:
        phi, mask, npts, iso = C.geometry(case)
        lst = L.list_of(mask)
        for side in L.SIDES:
            r = _run(case, side)
            assert np.array_equal(r.label[~lst], C.prefill(npts)[~lst])
            lab = r.label[lst]
            assert ((lab == -1) | (lab >= 0)).all() and np.count_nonzero(lab == -1) == r.info[6]
            assert r.ncomp == len(np.unique(lab[lab >= 0])) == r.info[2] + r.info[3]
            flat = r.label.ravel(order="F")
            roots = r.comp[:, 0]
            assert (flat[roots] == roots).all() and r.comp[:, 1].sum() == r.info[1]
            idx = np.flatnonzero(flat >= 0) if case in C.ALL_ONES else None
            if idx is not None:
                idx = idx[lst.ravel(order="F")[idx]]
                assert (flat[idx] <= idx).all()  # the label is the smallest index of the component


@pytest.mark.parametrize("case", C.ALL_ONES)
def test_agrees_with_scipy_on_all_ones_masks(case):
    ndi = pytest.importorskip("scipy.ndimage")
    phi, mask, npts, iso = C.geometry(case)
    lst = L.list_of(mask)
    six = ndi.generate_binary_structure(3, 1)
    for side, sel in (("inside", phi - iso < 0), ("outside", ~(phi - iso < 0))):
        r = _run(case, side)
        lab, n = ndi.label(sel & lst, structure=six)
        assert n == r.ncomp
        # the same partition: every scipy component carries exactly one of our labels, its own smallest index
        flat, ours = lab.ravel(order="F"), r.label.ravel(order="F")
        for t in range(1, n + 1):
            idx = np.flatnonzero(flat == t)
            assert (ours[idx] == idx.min()).all()
        cells = np.bincount(flat, minlength=n + 1)[1:]
        assert sorted(cells) == sorted(r.comp[:, 1])


def test_the_table_describes_the_labels():
    for case in ("two", "hollow_band", "values"):
        phi, mask, npts, iso = C.geometry(case)
        lst = L.list_of(mask)
        r = _run(case, "both")
        for row in r.comp:
            sel = (r.label == row[0]) & lst
            i, j, k = np.nonzero(sel)
            assert row[1] == sel.sum() and row[3:9].tolist() == [i.min(), i.max(), j.min(), j.max(), k.min(), k.max()]
            assert row[2] == (-1 if phi.ravel(order="F")[row[0]] - iso < 0 else 1)
            open_ = np.zeros(npts, bool)
            for a in range(3):
                for s in (1, -1):
                    open_ |= ~np.roll(lst, s, axis=a)  # (list cells are interior: the roll never wraps onto one)
            assert row[9] == (sel & open_).sum()


def test_a_nan_is_refused_on_the_list_and_accepted_off_it():
    phi, mask, npts, iso = C.geometry("small")
    lst = L.list_of(mask)
    bad = phi.copy(order="F")
    bad[tuple(np.argwhere(~lst)[5])] = np.nan
    assert np.array_equal(L.label_band(bad, mask, C.prefill(npts)).label, _run("small", "inside").label)
    for v in (np.nan, np.inf):
        bad[tuple(np.argwhere(lst)[7])] = v
        bad[tuple(np.argwhere(lst)[70])] = v
        with pytest.raises(ValueError, match="2 list cell"):
            L.label_band(bad, mask, C.prefill(npts))


# ---------------------------------------------------------------------------------- the planted defects: each fails a check
def test_defect_diagonal_neighbours():
    assert _run("checker", "both", defect="diagonal").ncomp == 2 != _run("checker", "both").ncomp  # the parity classes fuse


def test_defect_zero_taken_as_inside():
    assert _classes("iso", "both") == (2, 3)
    r = _run("iso", "both", defect="zero")
    assert (r.info[2], r.info[3]) != (2, 3)
    assert _run("negzero", "both", defect="zero").info[3] < _run("negzero", "both").info[3]


def test_defect_link_through_an_off_list_cell():
    phi, mask, npts, iso = C.geometry("two")
    cut = np.array(mask, order="F", copy=True)
    cut[20, :, :] = 0  # a plane off the list splits the exterior in two
    good = L.label_band(phi, cut, C.prefill(npts), iso, "outside")
    assert good.ncomp == 2 and (good.comp[:, 9] > 0).all()
    assert L.label_band(phi, cut, C.prefill(npts), iso, "outside", defect="offlist").ncomp == 1


def test_defect_wall_point_admitted():
    phi, mask, npts, iso = C.geometry("values")  # 1s on all six walls
    good, bad = _run("values", "both"), _run("values", "both", defect="wall")
    assert good.info[0] == 184 < bad.info[0]
    assert not np.array_equal(good.label, bad.label)
    walls = ~L.list_of(np.ones(npts, np.int32))
    assert np.array_equal(good.label[walls], C.prefill(npts)[walls]) and not np.array_equal(bad.label[walls], C.prefill(npts)[walls])


# ---------------------------------------------------------------------------------- the merge case, chosen here for the GPU test
def test_the_chain_case_merges():
    import evolve_band_ref as V

    phi, mask, speed, dx, dt, steps = C.two_sphere_chain()
    before = L.label_band(phi, mask, C.prefill(phi.shape), 0.0, "inside")
    assert before.ncomp == 2 and (before.comp[:, 9] == 0).all()
    gap = (0.62 - 0.45) * 2 / dx
    assert 3 < gap < 4 and steps * dt > 0.5 * gap * dx + dx  # a few cells, and closed with a cell to spare
    e = V.evolve_band(phi, mask, None, speed, dx, dt, steps)
    assert e.steps == steps and not e.nan and e.flips == 0
    after = L.label_band(e.field, e.mask, C.prefill(phi.shape), 0.0, "inside")
    assert after.ncomp == 1 and after.comp[0, 9] == 0 and after.comp[0, 1] > before.comp[:, 1].sum()
