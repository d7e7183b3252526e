"""CPU checks behind tests/test_gpu_advect_nodes.py: the oracle's narrowBand / order-8 gradients / node advection against the
reference's own run on a non-cubic grid (golden/synth_post_37x29x23.npz), the numpy statement (advect_nodes_ref.py) against the oracle
on every input set of the GPU tests, and each switchable defect of that statement against the input set named to expose it.  Every
comparison is `==` on the bit patterns."""
import functools

import numpy as np
import pytest

import advect_nodes_inputs as inp
import advect_nodes_ref as ref
from advect_nodes_inputs import same_bits


@functools.lru_cache(maxsize=None)
def _oracle_nodes(name):
    import oracle_lib

    c = inp.case(name)
    return oracle_lib.advect(c.phi, c.sb, *c.n, c.dx, c.xLo, c.nodes, iters=c.iters)


def test_oracle_equals_the_reference_on_a_non_cubic_grid(oracle):
    g = inp.post_fixture()
    nx, ny, nz = int(g["nx"]), int(g["ny"]), int(g["nz"])
    assert (nx + 1, ny + 1, nz + 1) == inp.POST_NPTS and len({nx, ny, nz}) == 3 and len(set(g["xLo"])) == 3
    phi, nodes = inp.post_input()  # the committed input is what the shared constructor builds
    assert same_bits(phi, g["phi"]) and same_bits(nodes, g["nodes_in"])
    nb, sb = oracle.narrowband(nx, ny, nz, float(g["dx"]), phi)
    assert np.array_equal(nb, g["NB"]) and np.array_equal(sb, g["SB"])
    assert same_bits(oracle.firstderiv8(phi, sb, nx, ny, nz, float(g["dx"])), g["gradPhi"])
    assert same_bits(g["nodes_0"], g["nodes_in"])
    for k in inp.POST_PASSES:
        assert same_bits(_oracle_nodes(f"synth-post-{k}"), g[f"nodes_{k}"]), k
    # the passes differ from one another, so a pass too many or too few is seen
    assert not same_bits(g["nodes_0"], g["nodes_1"]) and not same_bits(g["nodes_1"], g["nodes_2"])
    assert not same_bits(g["nodes_2"], g["nodes_1000"]) and int(g["passes_to_settle"]) > 2


@pytest.mark.parametrize("q", range(len(inp.NB_DXS)))
def test_narrowband_thresholds_equal_the_reference(oracle, q):
    """values exactly on 4.1*dx and 8.1*dx, their neighbours in double, +-0.0, NaN, +-inf"""
    g, dx = inp.post_fixture(), inp.NB_DXS[q]
    f = inp.threshold_field(dx)
    nb, sb = oracle.narrowband(*(v - 1 for v in f.shape), dx, f)
    assert np.array_equal(nb, g[f"thr{q}_NB"]) and np.array_equal(sb, g[f"thr{q}_SB"])
    rnb, rsb = ref.narrowband(f, dx)
    assert np.array_equal(nb, rnb) and np.array_equal(sb, rsb)
    flat, fnb, fsb = f.ravel(order="F"), nb.ravel(order="F"), sb.ravel(order="F")
    # +-t is outside, the double below it inside, for both bands; NaN and inf are outside, both zeros inside
    assert list(fnb[:6]) == [0, 0, 1, 1, 0, 0] and list(fsb[:6]) == [1] * 6
    assert list(fnb[6:12]) == [0] * 6 and list(fsb[6:12]) == [0, 0, 1, 1, 0, 0]
    assert list(fnb[12:17]) == [1, 1, 0, 0, 0] and list(fsb[12:17]) == [1, 1, 0, 0, 0] and np.isnan(flat[14])
    assert 0 < fnb[17:].sum() < fsb[17:].sum() < flat.size - 17


@pytest.mark.parametrize("name", inp.ADVECT_CASES)
def test_numpy_statement_equals_the_oracle(oracle, name):
    c = inp.case(name)
    assert inp.admissible(c.nodes, c.n, c.dx, c.xLo)
    want = _oracle_nodes(name)
    assert same_bits(ref.firstderiv8(c.phi, c.sb, *c.n, c.dx), oracle.firstderiv8(c.phi, c.sb, *c.n, c.dx))
    assert same_bits(ref.advect_nodes(c.phi, c.sb, *c.n, c.dx, c.xLo, c.nodes, iters=c.iters), want)
    inp.expectations(name, c, want)


@pytest.mark.parametrize("defect", sorted(ref.DEFECTS))
def test_each_defect_is_exposed_by_its_input_set(oracle, defect):
    """the inputs discriminate: the statement with ONE deliberate error differs from the oracle on the set named for it"""
    name = ref.DEFECTS[defect]
    assert name in inp.ADVECT_CASES
    c = inp.case(name)
    bad = ref.advect_nodes(c.phi, c.sb, *c.n, c.dx, c.xLo, c.nodes, iters=c.iters, defect=defect)
    assert not same_bits(bad, _oracle_nodes(name))
