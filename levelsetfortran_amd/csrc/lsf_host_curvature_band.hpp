// lsf_host_curvature_band.hpp -- host side of lsf_curvature_band (kernel and design: lsf_curvature_band.hpp; argument checks: lsf_host_args.hpp): the list,
// the one launch over it and the finish of its partials in block order (all three through lsf_host_band.hpp).  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed curvature_band_args_ok.  info and kappa_max are written on LSF_OK only; on LSF_ERR_NAN the outputs hold
// what was computed.  Returns after the stream is synchronised.
int curvature_band_core(const double* d_phi, const int32_t* d_mask, double* d_kappa, double* d_gauss, double* d_gmag, int nx, int ny, int nz,
                        double dx, double clamp, int64_t* info, double* kappa_max, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing to do, nothing written
        if (info) info[0] = info[1] = info[2] = info[3] = 0;
        if (kappa_max) *kappa_max = 0.0;
        return LSF_OK;
    }
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * CURV_NPART * sizeof(unsigned long long)))) return rc;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const double two_dx = 2. * dx, dx2 = dx * dx, four_dx2 = 4. * (dx * dx);
    const bool clamped = clamp != 0.0;
    const double lim = clamped ? clamp / dx : 0.0, lim2 = lim * lim;
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
    with_flags(
        [&](auto HG, auto HM, auto CL) {
            hipLaunchKernelGGL((k_curvature_band<decltype(HG)::value, decltype(HM)::value, decltype(CL)::value>), grid, blk, 0, st, d_phi,
                               (const int*)bl.L, nL, nx, ny, d_kappa, d_gauss, d_gmag, two_dx, dx2, four_dx2, lim, lim2, part);
        },
        d_gauss != nullptr, d_gmag != nullptr, clamped);
    HIPCHK(hipGetLastError());
    unsigned long long tot[CURV_NPART]; // degenerate, clamped, non-finite, the largest |kappa| as a bit pattern
    if ((rc = block_counts_finish(part, nchunks, CURV_NPART, tot, nullptr, st, true))) return rc;
    const unsigned long long ndeg = tot[0], nclamp = tot[1], nbad = tot[2], amax = tot[3];
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] curvature on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu degenerate, %llu clamped, %llu non-finite\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, ndeg, nclamp, nbad);
    if (nbad)
        return fail(LSF_ERR_NAN, "lsf_curvature_band: " + std::to_string(nbad) + " list cell(s) hold a non-finite kappa, gauss or gmag");
    if (info) info[0] = nL, info[1] = (int64_t)ndeg, info[2] = (int64_t)nclamp, info[3] = 0;
    if (kappa_max) std::memcpy(kappa_max, &amax, sizeof amax);
    return LSF_OK;
}
