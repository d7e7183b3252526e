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
    Ctx& c = ctx();
    const int nblocks = (int)(((size_t)nrays + CR_BLOCK - 1) / CR_BLOCK);
    if ((rc = ws(c.slot[S_PART], (size_t)nblocks * CR_NPART * sizeof(unsigned long long)))) return rc;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const CrParams P{iso, tmin, tmax, safety, smin * dx, smax * dx, skip * dx, refine, max_steps}; // one rounded product each
    const dim3 grid((unsigned)nblocks), blk(CR_BLOCK);
#define LSF_CR_CALL(CU, HM, HQ) \
    hipLaunchKernelGGL((k_cast_rays<CU, HM, HQ>), grid, blk, 0, st, G, d_q, d_org, d_dir, nrays, P, d_thit, d_hit, d_grad, d_qval, d_status, part)
    switch ((order == LSF_SAMPLE_CUBIC ? 4 : 0) | (d_mask ? 2 : 0) | (d_q ? 1 : 0)) {
    case 0: LSF_CR_CALL(false, false, false); break;
    case 1: LSF_CR_CALL(false, false, true); break;
    case 2: LSF_CR_CALL(false, true, false); break;
    case 3: LSF_CR_CALL(false, true, true); break;
    case 4: LSF_CR_CALL(true, false, false); break;
    case 5: LSF_CR_CALL(true, false, true); break;
    case 6: LSF_CR_CALL(true, true, false); break;
    default: LSF_CR_CALL(true, true, true); break;
    }
#undef LSF_CR_CALL
    HIPCHK(hipGetLastError());
    unsigned long long tot[CR_NPART];
    if ((rc = block_counts_finish(part, nblocks, CR_NPART, tot, info, st))) return rc; // (lsf_host_sample_points.hpp)
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] rays: %d rays, %d blocks, %llu hit, %llu miss, %llu no grid, %llu bad, %llu lost, %llu out of steps; %llu samples, %llu strides, %llu began inside\n",
                nrays, nblocks, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7], tot[8]);
    return LSF_OK;
}
