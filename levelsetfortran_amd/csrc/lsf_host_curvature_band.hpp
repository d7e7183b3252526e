// lsf_host_curvature_band.hpp -- host side of lsf_curvature_band (kernel and design: lsf_curvature_band.hpp; argument checks: lsf_host_args.hpp): the list,
// the one launch over it and the finish of its partials in block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed curvature_band_args_ok.  info and kappa_max are written on LSF_OK only; on LSF_ERR_NAN the outputs hold
// what was computed.  Returns after the stream is synchronised.
int curvature_band_core(const double* d_phi, const int32_t* d_mask, double* d_kappa, double* d_gauss, double* d_gmag, int nx, int ny, int nz,
                        double dx, double clamp, int64_t* info, double* kappa_max, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_count<true>(bl, nullptr, d_mask, nx, ny, nz, dx, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing to do, nothing written
        if (info) info[0] = info[1] = info[2] = info[3] = 0;
        if (kappa_max) *kappa_max = 0.0;
        return LSF_OK;
    }
    // (a grid whose brick keys do not fit 32 bits keeps the memory order: only the locality of a chunk depends on the order)
    if ((rc = band_list_sort(bl, bl.keys_fit(), st))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * CURV_NPART * sizeof(unsigned long long)))) return rc;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const double two_dx = 2. * dx, dx2 = dx * dx, four_dx2 = 4. * (dx * dx);
    const bool clamped = clamp != 0.0;
    const double lim = clamped ? clamp / dx : 0.0, lim2 = lim * lim;
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
#define LSF_CURV_CALL(HK, HG, CL) \
    hipLaunchKernelGGL((k_curvature_band<HK, HG, CL>), grid, blk, 0, st, d_phi, (const int*)bl.L, nL, nx, ny, d_kappa, d_gauss, d_gmag, two_dx, dx2, \
                       four_dx2, lim, lim2, part)
    switch ((d_gauss ? 4 : 0) | (d_gmag ? 2 : 0) | (clamped ? 1 : 0)) {
    case 0: LSF_CURV_CALL(false, false, false); break;
    case 1: LSF_CURV_CALL(false, false, true); break;
    case 2: LSF_CURV_CALL(false, true, false); break;
    case 3: LSF_CURV_CALL(false, true, true); break;
    case 4: LSF_CURV_CALL(true, false, false); break;
    case 5: LSF_CURV_CALL(true, false, true); break;
    case 6: LSF_CURV_CALL(true, true, false); break;
    default: LSF_CURV_CALL(true, true, true); break;
    }
#undef LSF_CURV_CALL
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> h((size_t)nchunks * CURV_NPART);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long ndeg = 0, nclamp = 0, nbad = 0, amax = 0;
    for (int b = 0; b < nchunks; ++b) { // block order; integer counts and a maximum of bit patterns: no order in the result
        const unsigned long long* t = &h[(size_t)b * CURV_NPART];
        ndeg += t[0], nclamp += t[1], nbad += t[2];
        amax = t[3] > amax ? t[3] : amax;
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] curvature on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu degenerate, %llu clamped, %llu non-finite\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, ndeg, nclamp, nbad);
    if (nbad)
        return fail(LSF_ERR_NAN, "lsf_curvature_band: " + std::to_string(nbad) + " list cell(s) hold a non-finite kappa, gauss or gmag");
    if (info) info[0] = nL, info[1] = (int64_t)ndeg, info[2] = (int64_t)nclamp, info[3] = 0;
    if (kappa_max) std::memcpy(kappa_max, &amax, sizeof amax);
    return LSF_OK;
}
