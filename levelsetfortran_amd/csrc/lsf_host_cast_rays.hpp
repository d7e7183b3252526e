// lsf_host_cast_rays.hpp -- host side of lsf_cast_rays (kernel and design: lsf_cast_rays.hpp): validation, the one launch over the
// rays and the finish of its per-block counts in block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// what can be decided without the device (the arrays are the caller's, host or device: only compared; xLo is a host array on both
// seams); nothing is written anywhere before this has passed
int cast_rays_args_ok(const void* phi, const void* mask, const void* q, int nx, int ny, int nz, double dx, const double* xLo, const void* org,
                      const void* dir, int nrays, int order, double iso, double tmin, double tmax, double safety, double smin, double smax, double skip,
                      int refine, int max_steps, const void* thit, const void* hit, const void* grad, const void* qval, const void* status)
{
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_cast_rays: phi is NULL");
    if (!org) return fail(LSF_ERR_INVALID, "lsf_cast_rays: org is NULL");
    if (!dir) return fail(LSF_ERR_INVALID, "lsf_cast_rays: dir is NULL");
    if (!thit) return fail(LSF_ERR_INVALID, "lsf_cast_rays: thit is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_cast_rays: xLo is NULL");
    if (nrays < 1) return fail(LSF_ERR_INVALID, "lsf_cast_rays: nrays must be >= 1");
    if (nx < 1 || ny < 1 || nz < 1) return fail(LSF_ERR_INVALID, "lsf_cast_rays: nx, ny, nz must be >= 1");
    if ((double)((size_t)nx + 1) * (double)((size_t)ny + 1) * (double)((size_t)nz + 1) > 2147483647.0)
        return fail(LSF_ERR_INVALID, "lsf_cast_rays: more than 2^31 - 1 points");
    const size_t n = ((size_t)nx + 1) * ((size_t)ny + 1) * ((size_t)nz + 1), nr = (size_t)nrays;
    if (!(dx > 0.0) || !std::isfinite(dx)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: dx must be finite and > 0");
    if (!std::isfinite(xLo[0]) || !std::isfinite(xLo[1]) || !std::isfinite(xLo[2]))
        return fail(LSF_ERR_INVALID, "lsf_cast_rays: xLo must hold three finite values");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: iso must be finite");
    if (order != LSF_SAMPLE_LINEAR && order != LSF_SAMPLE_CUBIC) return fail(LSF_ERR_INVALID, "lsf_cast_rays: unknown order");
    if (!(tmin >= 0.0) || !std::isfinite(tmin)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: tmin must be finite and >= 0");
    if (!(tmax > tmin) || !std::isfinite(tmax)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: tmax must be finite and > tmin");
    if (!(safety > 0.0 && safety <= 1.0)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: safety must lie in (0, 1]");
    if (!(smin > 0.0) || !std::isfinite(smin)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: smin must be finite and > 0");
    if (!(smax >= smin) || !std::isfinite(smax)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: smax must be finite and >= smin");
    if (!(skip > 0.0) || !std::isfinite(skip)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: skip must be finite and > 0");
    if (refine < 0) return fail(LSF_ERR_INVALID, "lsf_cast_rays: refine must be >= 0");
    if (max_steps < 1) return fail(LSF_ERR_INVALID, "lsf_cast_rays: max_steps must be >= 1");
    if (qval && !q) return fail(LSF_ERR_INVALID, "lsf_cast_rays: qval without q");
    // an output is written while the inputs and the other outputs are still being read or written: it may share a byte with none of
    // them.  The overlap test of sample_points_args_ok, each array with its own size.
    const void* a[10] = {phi, mask, q, org, dir, thit, hit, grad, qval, status};
    const size_t bytes[10] = {n * sizeof(double),       n * sizeof(int32_t),  n * sizeof(double),       3 * nr * sizeof(double), 3 * nr * sizeof(double),
                              nr * sizeof(double),      3 * nr * sizeof(double), 3 * nr * sizeof(double), nr * sizeof(double),     nr * sizeof(int32_t)};
    const char* name[10] = {"phi", "mask", "q", "org", "dir", "thit", "hit", "grad", "qval", "status"};
    for (int i = 5; i < 10; ++i) // the outputs
        for (int j = 0; j < i; ++j) {
            if (!a[i] || !a[j]) continue;
            const uintptr_t x = (uintptr_t)a[i], y = (uintptr_t)a[j];
            if (x < y ? y - x < bytes[i] : x - y < bytes[j])
                return fail(LSF_ERR_INVALID, std::string("lsf_cast_rays: ") + name[i] + " overlaps " + name[j]);
        }
    return LSF_OK;
}

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
    std::vector<unsigned long long> h((size_t)nblocks * CR_NPART);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long tot[CR_NPART] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nblocks; ++b) // block order; integer counts: no order in the result
        for (int m = 0; m < CR_NPART; ++m) tot[m] += h[(size_t)b * CR_NPART + m];
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] rays: %d rays, %d blocks, %llu hit, %llu miss, %llu no grid, %llu bad, %llu lost, %llu out of steps; %llu samples, %llu strides, %llu began inside\n",
                nrays, nblocks, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7], tot[8]);
    if (info)
        for (int m = 0; m < CR_NPART; ++m) info[m] = (int64_t)tot[m];
    return LSF_OK;
}
