// lsf_host_reinit_band.hpp -- host side of lsf_reinit_band (kernels and design: lsf_reinit_band.hpp; the list: lsf_host_band.hpp).
// Included by lsf_api.hip inside its anonymous namespace.
#pragma once

int reinit_band_core(double* d_phi, const double* d_phiS, const int32_t* d_mask, int nx, int ny, int nz, int iter, double dx, double h,
                     double tol, int mode, int* sweeps_done, double* rms_trace, int trace_cap, hipStream_t st)
{
    int rc = check_dims(nx, ny, nz);
    if (rc) return rc;
    if (iter < 0) return fail(LSF_ERR_INVALID, "iter must be >= 0");
    const int order = mode & LSF_ORDER_MASK;
    if (order == LSF_ORDER_GS)
        return fail(LSF_ERR_INVALID, "lsf_reinit_band: LSF_ORDER_GS has no meaning on a list of cells (a raster order needs the grid); "
                                     "pass LSF_ORDER_JACOBI");
    if (order != LSF_ORDER_JACOBI) return fail(LSF_ERR_INVALID, "unknown ordering");
    if (!d_phi) return fail(LSF_ERR_INVALID, "phi is NULL");
    if (!d_mask) return fail(LSF_ERR_INVALID, "mask is NULL");
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    if (n > (size_t)0x7fffffff) return fail(LSF_ERR_INVALID, "lsf_reinit_band: more than 2^31 - 1 points (list entries are 32-bit point indices)");
    const bool strict = (mode & LSF_ARITH_STRICT) != 0;
    if (sweeps_done) *sweeps_done = 0;
    Ctx& c = ctx();
    const bool trace = getenv("LSF_TRACE") != nullptr;
    const double t_build0 = trace ? now_s() : 0.0;
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) return LSF_OK; // empty list: nothing to do, nothing written
    const int max_sweeps = iter + 1; // DO n=0,iter (subs.f90:735)
    if ((rc = ws(c.slot[S_RB_PHIS], (size_t)nL * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART2], 256 * sizeof(double)))) return rc;
    const int* L = bl.L;
    double* pong = (double*)bl.staging; // the second field was the staging of the list build, which is over before the field is copied into it
    double* ps = (double*)c.slot[S_RB_PHIS].p;
    double* part = (double*)c.slot[S_PART].p;
    double* part2 = (double*)c.slot[S_PART2].p;
    const dim3 b256(256), gl((unsigned)nchunks);
    hipLaunchKernelGGL(k_rb_gather, gl, b256, 0, st, L, d_phiS ? d_phiS : (const double*)d_phi, nL, ps); // subs.f90:731
    // the one pass over the grid: the second field starts as a copy of the first (points outside the list never change in either)
    HIPCHK(hipMemcpyAsync(pong, d_phi, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    StopLoop stop;
    if ((rc = stop.begin(c, max_sweeps, st))) return rc;
    if (trace) {
        HIPCHK(hipStreamSynchronize(st));
        fprintf(stderr, "[lsf] reinit on the band: %d list cells (%.2f %% of the grid), %d chunks; list built and field copied in %.3f ms\n", nL,
                100.0 * nL / (double)n, nchunks, (now_s() - t_build0) * 1e3);
    }
    double* bufs[2] = {d_phi, pong};
    for (int s = 0; s < max_sweeps; ++s) {
        const double* A = bufs[s & 1];
        double* B = bufs[(s + 1) & 1];
        with_flags(
            [&](auto S) {
                hipLaunchKernelGGL((k_reinit_band<decltype(S)::value>), gl, b256, 0, st, A, B, (const double*)ps, L, nL, nx, ny, nz, dx, h, part,
                                   (const int*)stop.ctl);
            },
            strict);
        reduce_finish(part, nchunks, part2, (double)nL, tol, stop);
        if (stop.poll(s, max_sweeps)) break;
    }
    if ((rc = stop.finish())) return rc;
    // an odd number of sweeps: the result sits in the second field; its list cells are all that differs
    if (stop.count() & 1) hipLaunchKernelGGL(k_rb_scatter, gl, b256, 0, st, L, (const double*)pong, nL, d_phi);
    HIPCHK(hipGetLastError());
    return stop.verdict(rms_trace, trace_cap, sweeps_done, "RMS became NaN (the reference STOPs here, subs.f90:926)");
}
