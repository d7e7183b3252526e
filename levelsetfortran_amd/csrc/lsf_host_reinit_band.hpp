// lsf_host_reinit_band.hpp -- host side of lsf_reinit_band (kernels and design: lsf_reinit_band.hpp).  Included by lsf_api.hip inside
// its anonymous namespace.
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
    const long nblk = (long)((n + MB_SCAN - 1) / MB_SCAN);
    // the second field doubles as the staging of the list build (n ints of it), which is over before the field is copied into it
    if ((rc = ws(c.slot[S_PONG], n * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_MB_CNT], (size_t)(2 * nblk + 8) * sizeof(int)))) return rc;
    if ((rc = ws(c.slot[S_CTL], 64))) return rc;
    double* pong = (double*)c.slot[S_PONG].p;
    int* staging = (int*)pong;
    int* counts = (int*)c.slot[S_MB_CNT].p;
    int* offsets = counts + ((nblk + 3) & ~3L); // 16-byte aligned like counts (k_mb_offsets moves vectors)
    const bool trace = getenv("LSF_TRACE") != nullptr;
    const double t_build0 = trace ? now_s() : 0.0;
    hipLaunchKernelGGL(k_mb_collect<true>, dim3((unsigned)nblk), dim3(256), 0, st, (const double*)nullptr, d_mask, nx, ny, nz, dx, staging, counts);
    hipLaunchKernelGGL(k_mb_offsets, dim3(1), dim3(1024), 0, st, (const int*)counts, nblk, offsets);
    int nL = 0;
    HIPCHK(hipMemcpyAsync(&nL, offsets + nblk, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nL <= 0) return LSF_OK; // empty list: nothing to do, nothing written
    const int max_sweeps = iter + 1; // DO n=0,iter (subs.f90:735)
    const int nchunks = (nL + MB_CH - 1) / MB_CH;
    if ((rc = ws(c.slot[S_MB_L], (size_t)nL * sizeof(int)))) return rc;
    if ((rc = ws(c.slot[S_MB_KEY], (size_t)nL * 3 * sizeof(int)))) return rc;
    if ((rc = ws(c.slot[S_RB_PHIS], (size_t)nL * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART2], 256 * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_TRACE], (size_t)max_sweeps * sizeof(double)))) return rc;
    int* L = (int*)c.slot[S_MB_L].p;
    double* ps = (double*)c.slot[S_RB_PHIS].p;
    double* part = (double*)c.slot[S_PART].p;
    double* part2 = (double*)c.slot[S_PART2].p;
    int* ctl = (int*)c.slot[S_CTL].p;
    double* d_trace = (double*)c.slot[S_TRACE].p;
    const dim3 b256(256), gl((unsigned)nchunks);
    {
        // the list in memory order and its brick keys -> sorted by key (lsf_host_minmax.hpp).  A grid whose brick keys do not fit
        // 32 bits keeps the memory order: the result does not depend on the order of the list, only the locality of a chunk does
        const int nbx = cdiv(nx + 1, 8), nby = cdiv(ny + 1, 8);
        const bool sorted = (double)nbx * nby * cdiv(nz + 1, 4) * 256.0 <= 4.0e9;
        unsigned* key_in = (unsigned*)c.slot[S_MB_KEY].p;
        unsigned* key = key_in + nL;
        int* L_in = (int*)(key + nL);
        hipLaunchKernelGGL(k_mb_gather, dim3((unsigned)((nblk + 3) / 4)), b256, 0, st, (const int*)staging, (const int*)counts, (const int*)offsets,
                           nblk, nx + 1, ny + 1, nbx, nby, sorted ? L_in : L, key_in);
        if (sorted) {
            size_t tmp_bytes = 0;
            HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_in, key, L_in, L, (size_t)nL, 0, 32, st));
            void* tmp = staging; // (free again: its segments have been gathered -- in stream order)
            if (tmp_bytes > n * sizeof(int)) { // tiny grids
                if ((rc = ws(c.slot[S_MB_TMP], tmp_bytes))) return rc;
                tmp = c.slot[S_MB_TMP].p;
            }
            HIPCHK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key, L_in, L, (size_t)nL, 0, 32, st));
        }
    }
    hipLaunchKernelGGL(k_rb_gather, gl, b256, 0, st, (const int*)L, d_phiS ? d_phiS : (const double*)d_phi, nL, ps); // subs.f90:731
    // the one pass over the grid: the second field starts as a copy of the first (points outside the list never change in either)
    HIPCHK(hipMemcpyAsync(pong, d_phi, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(ctl, 0, 64, st));
    if (trace) {
        HIPCHK(hipStreamSynchronize(st));
        fprintf(stderr, "[lsf] reinit on the band: %d list cells (%.2f %% of the grid), %d chunks; list built and field copied in %.3f ms\n", nL,
                100.0 * nL / (double)n, nchunks, (now_s() - t_build0) * 1e3);
    }
    double* bufs[2] = {d_phi, pong};
    int host_ctl[3] = {0, 0, 0};
    for (int s = 0; s < max_sweeps; ++s) {
        const double* A = bufs[s & 1];
        double* B = bufs[(s + 1) & 1];
        if (strict)
            hipLaunchKernelGGL((k_reinit_band<true>), gl, b256, 0, st, A, B, (const double*)ps, (const int*)L, nL, nx, ny, nz, dx, h, part, (const int*)ctl);
        else
            hipLaunchKernelGGL((k_reinit_band<false>), gl, b256, 0, st, A, B, (const double*)ps, (const int*)L, nL, nx, ny, nz, dx, h, part, (const int*)ctl);
        if (nchunks > 16384) {
            hipLaunchKernelGGL(k_reduce_slices, dim3(256), dim3(256), 0, st, (const double*)part, (long)nchunks, part2);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(RED_T), 0, st, (const double*)part2, 256L, (double)nL, tol, d_trace, max_sweeps, ctl);
        } else {
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(RED_T), 0, st, (const double*)part, (long)nchunks, (double)nL, tol, d_trace, max_sweeps, ctl);
        }
        if ((s + 1) % CHECK_EVERY == 0 && s + 1 < max_sweeps) {
            HIPCHK(hipMemcpyAsync(host_ctl, ctl, sizeof host_ctl, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (host_ctl[0]) break;
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host_ctl, ctl, sizeof host_ctl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int nsw = host_ctl[1];
    // an odd number of sweeps: the result sits in the second field; its list cells are all that differs
    if (nsw & 1) hipLaunchKernelGGL(k_rb_scatter, gl, b256, 0, st, (const int*)L, (const double*)pong, nL, d_phi);
    HIPCHK(hipGetLastError());
    if (rms_trace && trace_cap > 0 && nsw > 0)
        HIPCHK(hipMemcpyAsync(rms_trace, d_trace, sizeof(double) * (size_t)std::min(nsw, trace_cap), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (sweeps_done) *sweeps_done = nsw;
    if (host_ctl[2]) return fail(LSF_ERR_NAN, "RMS became NaN (the reference STOPs here, subs.f90:926)");
    return LSF_OK;
}
