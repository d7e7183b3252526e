// lsf_host_cast_rays.hpp -- host side of lsf_cast_rays (kernel and design: lsf_cast_rays.hpp; argument checks: lsf_host_args.hpp): the one launch over the
// rays and the finish of its per-block counts in block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed cast_rays_args_ok and every array is device memory.  info is written on LSF_OK only.  Returns after the
// stream is synchronised.
int cast_rays_core(const double* d_phi, const int32_t* d_mask, const double* d_q, int nx, int ny, int nz, double dx, const double xLo[3],
                   const double* d_org, const double* d_dir, int nrays, int order, double iso, double tmin, double tmax, double safety, double smin,
                   double smax, double skip, int refine, int max_steps, double* d_thit, double* d_hit, double* d_grad, double* d_qval,
                   int32_t* d_status, int64_t* info, hipStream_t st)
{
    int rc;
    PointPlan pp;
    if ((rc = point_plan(pp, (size_t)nrays, CR_BLOCK, CR_NPART))) return rc;
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const CrParams P{iso, tmin, tmax, safety, smin * dx, smax * dx, skip * dx, refine, max_steps}; // one rounded product each
    with_flags(
        [&](auto CU, auto HM, auto HQ) {
            hipLaunchKernelGGL((k_cast_rays<decltype(CU)::value, decltype(HM)::value, decltype(HQ)::value>), dim3((unsigned)pp.nblocks), dim3(CR_BLOCK), 0, st, G,
                               d_q, d_org, d_dir, nrays, P, d_thit, d_hit, d_grad, d_qval, d_status, pp.part);
        },
        order == LSF_SAMPLE_CUBIC, d_mask != nullptr, d_q != nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long tot[CR_NPART];
    if ((rc = block_counts_finish(pp.part, pp.nblocks, CR_NPART, tot, info, st))) return rc;
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] rays: %d rays, %d blocks, %llu hit, %llu miss, %llu no grid, %llu bad, %llu lost, %llu out of steps; %llu samples, %llu strides, %llu began inside\n",
                nrays, pp.nblocks, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7], tot[8]);
    return LSF_OK;
}
