"""The statement of tests/reinit_f32_ref.py, validated without a GPU.

  * dtype=float64: equal to the C oracle's Jacobi sweep bit for bit, field and RMS trace -- so the statement IS the
    oracle's operation, and its float32 run is that operation in single precision, not a second opinion;
  * dtype=float32: its distance from the fp64 oracle (same fp32-rounded input) after one sweep is at most 4 in units of
    eps32 * max|phi| on every field.  The GPU tests allow the kernels 3 x the statement's distance
    (tests/test_gpu_f32_statement.py); this cap keeps that margin from being vacuous.  The measured figures (printed
    here, table in tests/test_gpu_f32_statement.py and DESIGN.md section 4.8) are at most 1.5.
"""
import numpy as np
import pytest

import reinit_f32_fields as F32F
import reinit_f32_ref as stmt
from levelsetfortran_amd import fields

ONE_SWEEP_CAP = 4.0


@pytest.mark.parametrize("kind", ["two", "box"])
@pytest.mark.parametrize("npts", [(5, 5, 5), (12, 9, 8), (21, 27, 13), (40, 33, 27)])
def test_float64_statement_equals_the_c_oracle_bit_for_bit(oracle, npts, kind):
    phi0, dx = fields.two_sphere_phi0(npts) if kind == "two" else F32F.box_distance(npts)
    nx, ny, nz = (v - 1 for v in npts)
    h = fields.reinit_step(dx)
    for sweeps in (1, 5):
        ref = phi0.copy(order="F")
        rc, n, tr = oracle.reinit(ref, nx, ny, nz, sweeps - 1, dx, h, tol=0.0, order=oracle.JACOBI)
        got, n_s, tr_s = stmt.reinit(phi0, nx, ny, nz, sweeps - 1, dx, h, tol=0.0, dtype=np.float64)
        assert rc == 0 and n == n_s == sweeps
        assert got.dtype == np.float64 and np.array_equal(got, ref), float(np.abs(got - ref).max())
        assert np.array_equal(tr_s, tr)
    # the stop test of the loop (subs.f90:915): the first sweep below tol is the last one
    tol = float(tr[2]) * 1.0001
    ref = phi0.copy(order="F")
    _, n, tr2 = oracle.reinit(ref, nx, ny, nz, 4, dx, h, tol=tol, order=oracle.JACOBI)
    got, n_s, tr_s = stmt.reinit(phi0, nx, ny, nz, 4, dx, h, tol=tol, dtype=np.float64)
    assert n == n_s and np.array_equal(got, ref) and np.array_equal(tr_s, tr2)


def test_float32_statement_keeps_every_intermediate_in_float32():
    """No silent promotion: the pieces return float32 for float32 operands (dx, h and every constant included)."""
    in32, dx, h = F32F.make("box", (12, 11, 10))
    T = np.float32
    q = [in32[m:m + 4, 4:7, 4:7] for m in range(7)]
    for yq in (False, True):
        assert all(v.dtype == T for v in stmt.weno_axis(q, T(dx), yq, T))
    gM = stmt.grad_mag(in32, 11, 10, 9, T(dx), T)
    assert gM.dtype == T and stmt.phisign(in32[1:-1, 1:-1, 1:-1], T(dx), gM).dtype == T
    out = stmt.sweep_jacobi(in32, in32, 11, 10, 9, T(dx), T(h), T)
    stmt.bc_closed(out, 11, 10, 9, T(dx))
    assert out.dtype == T and np.isfinite(out).all()


@pytest.mark.parametrize("name", F32F.ACCURACY_FIELDS + F32F.FINITE_FIELDS)
def test_float32_statement_distance_from_the_fp64_oracle(oracle, name):
    d = {}
    for sweeps in (1, 9):
        c = F32F.case(name, sweeps)
        assert c.stmt.dtype == np.float32 and np.isfinite(c.stmt).all() and np.isfinite(c.stmt_trace).all()
        d[sweeps] = (c.stmt_max, c.stmt_rms)
        print(f"f32-statement {name:>12s} sweeps={sweeps}: max {c.stmt_max:6.3f}  rms {c.stmt_rms:6.3f}  (eps32 * max|phi|)")
    assert d[1][0] <= ONE_SWEEP_CAP, d
    # the trace: float64 sum of float32 differences over the true cell count; the oracle's divisor is the same number here
    c = F32F.case(name, 9)
    assert np.allclose(c.stmt_trace, c.ref_trace, rtol=2e-3, atol=0)


def test_float32_rescale_changes_no_bit_where_the_squares_are_in_range():
    """The power-of-two rescale of (eps + IS_k) is the only thing the float32 statement adds to the textbook form: on
    operands whose squares neither underflow nor overflow it returns the weights of the unscaled expression, bit for bit."""
    rng = np.random.default_rng(99)
    T = np.float32
    e = [np.exp(rng.uniform(np.log(1e-9), np.log(1e9), 4096)).astype(T) for _ in range(3)]
    a = stmt._alphas(e[0], e[1], e[2], T)
    b = (T(1.) / (e[0] * e[0]), T(6.) / (e[1] * e[1]), T(3.) / (e[2] * e[2]))
    for k in (0, 2):
        assert np.array_equal(a[k] / (a[0] + a[1] + a[2]), b[k] / (b[0] + b[1] + b[2]))
    # a flat stencil (eps + IS = the floor on all three): the linear weights 0.1 and 0.3, not inf / inf
    f = np.full(3, 1e-30, dtype=T)
    a = stmt._alphas(f, f, f, T)
    assert np.allclose(a[0] / (a[0] + a[1] + a[2]), 0.1, rtol=1e-6) and np.allclose(a[2] / (a[0] + a[1] + a[2]), 0.3, rtol=1e-6)
