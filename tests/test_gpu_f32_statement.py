"""fp32 Jacobi reinit against its float32 statement: accuracy, every kernel instance, hard fields.

The fp32 path (lsf_f32.hpp: k_reinit_jacobi_f32_sh<1|2|4|8>, k_reinit_jacobi_f32<false|true>; jacobi_plan_f32; the float
instantiation of jacobi_loop) has no fp64 twin to be identical to.  Its yardstick is tests/reinit_f32_ref.py, one numpy
statement of the oracle's Jacobi sweep that takes a dtype: with float64 it IS the C oracle bit for bit
(tests/test_reinit_f32_cpu.py), with float32 it is what plain single precision makes of the same operations.

Rule (a): on the same fp32-rounded input, max and RMS of (kernel - fp64 oracle) over the whole array, wall points
included, are at most 3 x the float32 statement's own max and RMS distance from the fp64 oracle, the statement's distance
being computed here and never stored; and the signs agree wherever |oracle| > 3 x the statement's max error.  The factor 3
covers what the kernel does beyond the statement (approximate v_rcp_f32 / v_rsq_f32, FMA-contracted lean algebra, the
interface form), each a rounding of the size the statement already has.

Measured distances from the fp64 oracle in units of eps32 * max|phi|, whole array, (37,30,41) points (cube: 62^3): the
statement on the CPU, the kernel (k_reinit_jacobi_f32_sh<1>) on an MI355X.

  field         sweeps   statement max / rms    kernel max / rms
  two              1        1.123 / 0.172         1.123 / 0.172
  two              9        2.567 / 0.492         2.567 / 0.492
  cube             1        0.966 / 0.101         0.966 / 0.101
  cube             9        1.282 / 0.375         1.282 / 0.373
  box              1        0.689 / 0.066         0.689 / 0.066
  box              9        1.004 / 0.165         1.004 / 0.164
  noisy            1        0.965 / 0.153         0.965 / 0.153
  noisy            9        2.383 / 0.488         2.383 / 0.489
  random           1        0.567 / 0.109         0.545 / 0.109
  random           9        1.531 / 0.261         1.468 / 0.264
  box * 1e-8       1        0.395 / 0.068         0.395 / 0.068
  box * 1e-8       9        1.368 / 0.192         1.368 / 0.192
  box * 1e8        1        0.600 / 0.079         0.600 / 0.079
  box * 1e8        9        1.334 / 0.187         1.334 / 0.188
  box * 1e-13      1        0.240 / 0.028        26.570 / 2.268     (not asserted: the floor has taken over)
  box * 1e-13      9        1.194 / 0.161       670.667 / 59.365    (not asserted)
  box * 1e15       1        0.632 / 0.079         0.632 / 0.079     (not asserted)
  box * 1e15       9        1.159 / 0.179         1.159 / 0.183     (not asserted)

Largest kernel : statement ratio over every asserted case, the per-cell and thin-x kernels at the shapes of (c) and (d)
included: 1.00 (max), 1.01 (RMS).  Both distances are dominated by the one rounding of phi + h * k1 that kernel and
statement share (h * k1 is ~1e-3 of phi, so a relative error of 1e-6 in the gradient is 1e-9 of phi); what the rule
leaves room for is an error of a few 1e-5 in the one-sided differences, not of a few eps32 -- a wrong weight, neighbour or
half of a pair moves the differences by far more on the kinked fields (see the mutants in the commit that added this file).

Fields: tests/reinit_f32_fields.py.  Value range (derived from lsf_f32.hpp, see include/lsf.h): the unscaled q_k are
squares of second differences and overflow near |dphi| ~ 1e18; below |dphi| ~ 2e-12 the 1e-30 floor replaces the
reference's relative epsilon.  Scales 1e-8 and 1e8 get rule (a); 1e-13 and 1e15 finiteness of field and trace only.
"""
import numpy as np
import pytest
import torch

import reinit_f32_fields as F32F
import reinit_f32_ref as stmt

pytestmark = pytest.mark.gpu

EPS32 = stmt.EPS32
MARGIN = 3.0


@pytest.fixture(autouse=True)
def _auto_plan(monkeypatch):
    """jacobi_plan_f32 reads LSF_JAC_SH on every call: every test starts from the automatic choice"""
    monkeypatch.delenv("LSF_JAC_SH", raising=False)


def _dev(a32):
    return torch.from_numpy(np.array(a32.ravel(order="F"))).to("cuda:0")  # a copy: the shared inputs are read-only


def _back(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _kernel_name():
    from levelsetfortran_amd import _lib

    return (_lib.load().lsf_profile_kernel() or b"").decode()


def _run(c, sweeps=None, phiS=None, start=None):
    """`sweeps` Jacobi sweeps of case c's input (or of `start`) on the device seam; returns (float32 array, report)."""
    import levelsetfortran_amd as lsf

    d = _dev(c.in32 if start is None else start)
    rep = lsf.reinit(d, None, None, c.nx, c.ny, c.nz, (sweeps or c.sweeps) - 1, c.dx, c.h, tol=0.0, order="jacobi", arith="fast",
                     phiS=phiS)
    got = _back(d, c.in32.shape)
    assert got.dtype == np.float32 and rep.count == (sweeps or c.sweeps)
    return got, rep


def _rule_a(got, c, what=""):
    """rule (a) of the module docstring; prints the figures before it asserts.  Returns the two kernel : statement ratios."""
    k_max, k_rms = stmt.distance(got, c.ref)
    r_max, r_rms = k_max / c.stmt_max, k_rms / c.stmt_rms
    print(f"f32-distance {c.name:>12s} {str(c.in32.shape):>14s} sweeps={c.sweeps} {what:>26s}: statement max {c.stmt_max:6.3f} rms {c.stmt_rms:6.3f}"
          f" | kernel max {k_max:6.3f} rms {k_rms:6.3f} | ratio max {r_max:5.2f} rms {r_rms:5.2f}")
    assert np.isfinite(got).all()
    assert k_max <= MARGIN * c.stmt_max, (c.name, c.sweeps, k_max, c.stmt_max)
    assert k_rms <= MARGIN * c.stmt_rms, (c.name, c.sweeps, k_rms, c.stmt_rms)
    far = np.abs(c.ref) > MARGIN * c.stmt_max * EPS32 * np.abs(c.ref).max()
    assert far.mean() > 0.9 and np.array_equal(np.signbit(got[far]), np.signbit(c.ref[far]))
    return r_max, r_rms


# ------------------------------------------------------------------------------------------------ (a) accuracy
@pytest.mark.parametrize("sweeps", [1, 9])
@pytest.mark.parametrize("name", F32F.ACCURACY_FIELDS)
def test_kernel_within_three_times_the_statements_distance(oracle, name, sweeps):
    c = F32F.case(name, sweeps)
    got, rep = _run(c)
    _rule_a(got, c, _kernel_name())
    assert np.allclose(rep.rms, c.ref_trace, rtol=2e-3, atol=0)


@pytest.mark.parametrize("name", F32F.FINITE_FIELDS)
def test_scales_beyond_the_stated_range_stay_finite(oracle, name):
    """|dphi| ~ 8e-15 (the floor has taken over from the relative epsilon) and ~ 8e13 (four decades below the overflow of the
    unscaled q_k): finite field and trace; the distance is printed for the table, not asserted."""
    for sweeps in (1, 9):
        c = F32F.case(name, sweeps)
        got, rep = _run(c)
        k_max, k_rms = stmt.distance(got, c.ref)
        print(f"f32-distance {c.name:>12s} {str(c.in32.shape):>14s} sweeps={sweeps} {'(finiteness only)':>26s}: statement max {c.stmt_max:6.3f} rms"
              f" {c.stmt_rms:6.3f} | kernel max {k_max:6.3f} rms {k_rms:6.3f}")
        assert np.isfinite(got).all() and np.isfinite(rep.rms).all() and all(r > 0 for r in rep.rms)


# ------------------------------------------------------------------------------------------------ (b) RMS trace
@pytest.mark.parametrize("name,npts", [(n, F32F.NPTS) for n in F32F.ACCURACY_FIELDS]
                         + [("two", (24, 3, 24)), ("box", (66, 21, 37)), ("two", (132, 18, 35)), ("box", (302, 9, 12)),
                            ("box", (10, 70, 12)), ("two", (5, 5, 5))])
def test_reported_rms_is_the_change_of_the_kernels_own_output(oracle, name, npts):
    """sqrt(sum (out - in)^2 / (nx ny nz)) over the whole array, recomputed in float64.  A lane accumulates at most
    2 x 32 squares (a pair, F32_KC planes) in fp32 before the double reduction: 64 eps32, relative.  Shapes with an odd
    number of rows, one row only (no second cell of a pair anywhere) and a single pair per block included: a square counted
    for a cell that does not exist, or left out, shows here and nowhere else."""
    c = F32F.case(name, 1, npts)
    got, rep = _run(c)
    d = got.astype(np.float64) - c.in32.astype(np.float64)
    want = float(np.sqrt((d * d).sum() / (c.nx * c.ny * c.nz)))
    print(f"f32-trace {name} {c.in32.shape}: reported {rep.rms[0]!r} recomputed {want!r} rel {abs(rep.rms[0] - want) / want:.2e}")
    assert abs(rep.rms[0] - want) <= 64 * EPS32 * want


# ------------------------------------------------------------------------------------------------ (c) every instance, same bits
SHAPES = [((65, 9, 9), 1), ((66, 21, 37), None), ((129, 11, 9), 2), ((132, 18, 35), None), ((257, 9, 12), 4), ((302, 9, 12), None),
          ((513, 9, 9), 8), ((35, 70, 40), None), ((24, 3, 24), None), ((5, 5, 5), None),
          # the exact-block rows above are too thin in y or z for a WENO cell (9 points: the :506 test fails everywhere), so the
          # interfaces handed from lane to lane and from wavefront to wavefront are never consumed there.  The same rows, and
          # one cell into a second eight-wavefront block, with six WENO rows (j = 4, 5; k = 4, 5, 6): every wavefront of every
          # width hands interfaces over that cells use (one row is not enough: the Godunov switch takes D- in about half the cells)
          ((65, 11, 12), 1), ((129, 11, 12), 2), ((257, 11, 12), 4), ((513, 11, 12), 8), ((514, 11, 12), None)]


@pytest.mark.parametrize("npts,auto_wx", SHAPES)
def test_every_kernel_instance_returns_the_same_bits(oracle, monkeypatch, npts, auto_wx):
    """Rows of exactly one block of each width (63, 127, 255, 511 cells), one cell more, a helper lane in the middle of a
    row, a partial second block, many pair rows, a single row, no WENO cell: the per-cell kernel (LSF_JAC_SH=0), the
    automatic choice and the forced widths 1, 2, 4, 8 return one field; the per-cell result obeys rule (a).
    `random` beside the two fields the shapes were chosen for: on `two` the WENO correction of an interface is so small that a
    wrong one moves the result by one ulp at one shape only, and on `box` it is exactly zero away from the kinks -- with
    skipped hand-overs between wavefronts both still passed every exact-block shape.  On `random` every interface matters."""
    for name in ("two", "box", "random"):
        c = F32F.case(name, 4, npts)
        monkeypatch.setenv("LSF_JAC_SH", "0")
        base, r0 = _run(c)
        assert _kernel_name() == "k_reinit_jacobi_f32<false>"
        _rule_a(base, c, "k_reinit_jacobi_f32<false>")
        for env in (None, "1", "2", "4", "8"):
            if env is None:
                monkeypatch.delenv("LSF_JAC_SH")
            else:
                monkeypatch.setenv("LSF_JAC_SH", env)
            got, r1 = _run(c)
            kn = _kernel_name()
            if env is not None or auto_wx is not None:
                assert kn == f"k_reinit_jacobi_f32_sh<{env or auto_wx}>", (kn, env)
            else:
                assert kn.startswith("k_reinit_jacobi_f32_sh<"), kn
            assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (name, npts, kn, float(np.abs(got - base).max()))
            assert np.allclose(r1.rms, r0.rms, rtol=1e-6, atol=0), (name, npts, kn)  # same squares, another order


# ------------------------------------------------------------------------------------------------ (d) THINX, single domain
@pytest.mark.parametrize("sweeps", [1, 9])
@pytest.mark.parametrize("npts", [(10, 70, 12), (7, 67, 9)])
def test_thin_x_kernel_in_a_single_domain(oracle, npts, sweeps):
    """At most 8 cells in x and at least 64 in y: k_reinit_jacobi_f32<true>, which a single domain runs with xwall = 1
    (the decomposed runs of test_gpu_f32.py use it with xwall = 0 only): lanes beside the low and the high x wall share a
    wavefront.  (10,70,12) has one WENO column (i = 4), (7,67,9) none."""
    for name in ("two", "box"):
        c = F32F.case(name, sweeps, npts)
        got, _ = _run(c)
        assert _kernel_name() == "k_reinit_jacobi_f32<true>"
        _rule_a(got, c, "k_reinit_jacobi_f32<true>")


# ------------------------------------------------------------------------------------------------ (e) resume through phiS
@pytest.mark.parametrize("name,npts", [("two", (132, 18, 35)), ("box", F32F.NPTS), ("two", (10, 70, 12))])
def test_resume_through_phiS(oracle, name, npts):
    c = F32F.case(name, 6, npts)
    whole, rw = _run(c)
    first, r1 = _run(c, sweeps=3)
    resumed, r2 = _run(c, sweeps=3, phiS=_dev(c.in32), start=first)
    assert np.array_equal(resumed.view(np.uint32), whole.view(np.uint32))
    assert r1.rms + r2.rms == rw.rms
    explicit, r3 = _run(c, sweeps=3, phiS=_dev(c.in32))
    assert np.array_equal(explicit.view(np.uint32), first.view(np.uint32)) and r3.rms == r1.rms
    # phiS is read, not ignored: another sign field gives another result
    other, _ = _run(c, sweeps=3, phiS=_dev(np.asfortranarray(-c.in32)))
    assert not np.array_equal(other, first)


# ------------------------------------------------------------------------------------------------ (f) NaN verdict
@pytest.mark.parametrize("env", [None, "0"])
def test_nan_verdict_and_the_call_after_it(oracle, monkeypatch, env):
    import levelsetfortran_amd as lsf

    if env is not None:
        monkeypatch.setenv("LSF_JAC_SH", env)
    c = F32F.case("two", 4, (40, 33, 27))
    clean, rep = _run(c)
    bad = c.in32.copy(order="F")
    bad[20, 16, 13] = np.nan
    d = _dev(bad)
    with pytest.raises(lsf.LsfNaNError):
        lsf.reinit(d, None, None, c.nx, c.ny, c.nz, 3, c.dx, c.h, tol=0.0, order="jacobi", arith="fast")
    ref64 = torch.from_numpy(np.ascontiguousarray(bad.astype(np.float64).ravel(order="F"))).to("cuda:0")
    with pytest.raises(lsf.LsfNaNError):  # as the fp64 path does
        lsf.reinit(ref64, None, None, c.nx, c.ny, c.nz, 3, c.dx, c.h, tol=0.0, order="jacobi", arith="fast")
    again, rep2 = _run(c)
    assert np.array_equal(again.view(np.uint32), clean.view(np.uint32)) and rep2.rms == rep.rms


# ------------------------------------------------------------------------------------------------ (g) host seam
def test_host_seam_equals_device_seam_on_a_long_row(oracle):
    import levelsetfortran_amd as lsf

    c = F32F.case("box", 4, (132, 18, 35))
    dev, rd = _run(c)
    host = c.in32.copy(order="F")
    rh = lsf.reinit(host, None, None, c.nx, c.ny, c.nz, 3, c.dx, c.h, tol=0.0, order="jacobi", arith="fast")
    assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), dev.view(np.uint32))
    assert rh.rms == rd.rms and rh.count == 4
