// lsf_host_sample_points.hpp -- host side of lsf_sample_points (kernel and design: lsf_sample_points.hpp; argument checks: lsf_host_args.hpp): the one launch
// over the points and the finish of its per-block counts in block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed sample_points_args_ok and every array is device memory.  info is written on LSF_OK only.  Returns after
// the stream is synchronised.
int sample_points_core(const double* d_phi, const int32_t* d_mask, const double* d_q, int nx, int ny, int nz, double dx, const double xLo[3],
                       const double* d_pts, int npts, int order, double iso, int iters, double tol, double* d_val, double* d_grad, double* d_qval,
                       double* d_foot, int32_t* d_status, int64_t* info, hipStream_t st)
{
    int rc;
    PointPlan pp;
    if ((rc = point_plan(pp, (size_t)npts, SP_BLOCK, SP_NPART))) return rc;
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const double tol_dx = tol * dx;
    with_flags(
        [&](auto CU, auto HQ, auto HM, auto PR) {
            hipLaunchKernelGGL((k_sample_points<decltype(CU)::value, decltype(HQ)::value, decltype(HM)::value, decltype(PR)::value>), dim3((unsigned)pp.nblocks),
                               dim3(SP_BLOCK), 0, st, G, d_q, d_pts, npts, iso, iters, tol_dx, d_val, d_grad, d_qval, d_foot, d_status, pp.part);
        },
        order == LSF_SAMPLE_CUBIC, d_q != nullptr, d_mask != nullptr, iters >= 1);
    HIPCHK(hipGetLastError());
    unsigned long long tot[SP_NPART];
    if ((rc = block_counts_finish(pp.part, pp.nblocks, SP_NPART, tot, info, st))) return rc;
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] samples: %d points, %d blocks, %llu ok, %llu outside, %llu off the band, %llu linear fallbacks, %llu flat, %llu not converged\n",
                npts, pp.nblocks, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5]);
    return LSF_OK;
}
