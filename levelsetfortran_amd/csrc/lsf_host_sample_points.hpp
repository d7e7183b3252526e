// lsf_host_sample_points.hpp -- host side of lsf_sample_points (kernel and design: lsf_sample_points.hpp; argument checks: lsf_host_args.hpp): the one launch
// over the points and the finish of its per-block counts in block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// The finish of a launch whose blocks each left npart counts in part (here and in lsf_host_cast_rays.hpp): copies them home, synchronises
// the stream, adds them in block order (integer counts: no order in the result) into tot[0..npart) and fills info where one is given.
int block_counts_finish(const unsigned long long* part, int nblocks, int npart, unsigned long long* tot, int64_t* info, hipStream_t st)
{
    std::vector<unsigned long long> h((size_t)nblocks * npart);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int m = 0; m < npart; ++m) tot[m] = 0;
    for (int b = 0; b < nblocks; ++b)
        for (int m = 0; m < npart; ++m) tot[m] += h[(size_t)b * npart + m];
    if (info)
        for (int m = 0; m < npart; ++m) info[m] = (int64_t)tot[m];
    return LSF_OK;
}

// the arguments have passed sample_points_args_ok and every array is device memory.  info is written on LSF_OK only.  Returns after
// the stream is synchronised.
int sample_points_core(const double* d_phi, const int32_t* d_mask, const double* d_q, int nx, int ny, int nz, double dx, const double xLo[3],
                       const double* d_pts, int npts, int order, double iso, int iters, double tol, double* d_val, double* d_grad, double* d_qval,
                       double* d_foot, int32_t* d_status, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const int nblocks = (int)(((size_t)npts + SP_BLOCK - 1) / SP_BLOCK);
    if ((rc = ws(c.slot[S_PART], (size_t)nblocks * SP_NPART * sizeof(unsigned long long)))) return rc;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const double tol_dx = tol * dx;
    const dim3 grid((unsigned)nblocks), blk(SP_BLOCK);
#define LSF_SP_CALL(CU, HQ, HM, PR) \
    hipLaunchKernelGGL((k_sample_points<CU, HQ, HM, PR>), grid, blk, 0, st, G, d_q, d_pts, npts, iso, iters, tol_dx, d_val, d_grad, d_qval, d_foot, \
                       d_status, part)
    switch ((order == LSF_SAMPLE_CUBIC ? 8 : 0) | (d_q ? 4 : 0) | (d_mask ? 2 : 0) | (iters >= 1 ? 1 : 0)) {
    case 0: LSF_SP_CALL(false, false, false, false); break;
    case 1: LSF_SP_CALL(false, false, false, true); break;
    case 2: LSF_SP_CALL(false, false, true, false); break;
    case 3: LSF_SP_CALL(false, false, true, true); break;
    case 4: LSF_SP_CALL(false, true, false, false); break;
    case 5: LSF_SP_CALL(false, true, false, true); break;
    case 6: LSF_SP_CALL(false, true, true, false); break;
    case 7: LSF_SP_CALL(false, true, true, true); break;
    case 8: LSF_SP_CALL(true, false, false, false); break;
    case 9: LSF_SP_CALL(true, false, false, true); break;
    case 10: LSF_SP_CALL(true, false, true, false); break;
    case 11: LSF_SP_CALL(true, false, true, true); break;
    case 12: LSF_SP_CALL(true, true, false, false); break;
    case 13: LSF_SP_CALL(true, true, false, true); break;
    case 14: LSF_SP_CALL(true, true, true, false); break;
    default: LSF_SP_CALL(true, true, true, true); break;
    }
#undef LSF_SP_CALL
    HIPCHK(hipGetLastError());
    unsigned long long tot[SP_NPART];
    if ((rc = block_counts_finish(part, nblocks, SP_NPART, tot, info, st))) return rc;
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] samples: %d points, %d blocks, %llu ok, %llu outside, %llu off the band, %llu linear fallbacks, %llu flat, %llu not converged\n",
                npts, nblocks, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5]);
    return LSF_OK;
}
