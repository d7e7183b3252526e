// lsf_host_points.hpp -- host side of lsf_advect_points and lsf_correct_field (kernels and design: lsf_advect_points.hpp,
// lsf_correct_field.hpp; argument checks: lsf_host_args_points.hpp): the launches and the finish of their per-block partials in
// block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed advect_points_args_ok and every array is device memory.  cfl and info are written on LSF_OK only.
// Returns after the stream is synchronised.
int advect_points_core(const double* d_u, const double* d_v, const double* d_w, const double* d_phi, const double* d_speed, const int32_t* d_mask,
                       int nx, int ny, int nz, double dx, const double xLo[3], double* d_pts, int npts, int order, int scheme, double dt, int nsteps,
                       int32_t* d_status, double* cfl, int64_t* info, hipStream_t st)
{
    int rc;
    PointPlan pp;
    if ((rc = point_plan(pp, (size_t)npts, AP_BLOCK, AP_NPART))) return rc;
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const ApFields F{d_u, d_v, d_w, d_speed};
    const int euler = scheme == LSF_ADVECT_EULER;
    with_flags(
        [&](auto CU, auto HV, auto HS, auto HM) {
            if constexpr (decltype(HV)::value || decltype(HS)::value) // (advect_points_args_ok refuses a call with neither)
                hipLaunchKernelGGL((k_advect_points<decltype(CU)::value, decltype(HV)::value, decltype(HS)::value, decltype(HM)::value>),
                                   dim3((unsigned)pp.nblocks), dim3(AP_BLOCK), 0, st, G, F, d_pts, npts, euler, dt, nsteps, d_status, pp.part);
        },
        order == LSF_SAMPLE_CUBIC, d_u != nullptr, d_speed != nullptr, d_mask != nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long tot[AP_NPART]; // the counts of info, then the largest cfl of a block as a bit pattern
    if ((rc = block_counts_finish(pp.part, pp.nblocks, AP_NPART, tot, info, st, true))) return rc;
    if (cfl) std::memcpy(cfl, &tot[LSF_ADVECT_POINTS_INFO_LEN], sizeof(double));
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] points: %d points, %d steps asked, %llu ok, %llu outside, %llu off the band, %llu flat; %llu steps made, %llu linear fallbacks\n",
                npts, nsteps, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5]);
    return LSF_OK;
}

// the arguments have passed correct_field_args_ok and every array is device memory.  change and info are written on LSF_OK only.
// Returns after the stream is synchronised.
int correct_field_core(double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, const double xLo[3], const double* d_pts,
                       const double* d_rad, int npts, double slack, int32_t* d_status, double* change, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    // the cells the field is corrected on: the list of the mask, in memory order, or the grid
    BandList bl;
    size_t nwork = n;
    const int* L = nullptr;
    if (d_mask) {
        if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, false, st))) return rc;
        nwork = (size_t)std::max(bl.nL, 0), L = bl.L; // (an empty list: no L)
    }
    PointPlan pp;
    if ((rc = ws(c.slot[S_CF_PLUS], n * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_CF_MINUS], n * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_CF_CTL], 2 * sizeof(unsigned long long)))) return rc;
    if ((rc = point_plan(pp, (size_t)npts, CF_BLOCK, CF_NPART))) return rc;
    unsigned long long *plus = (unsigned long long*)c.slot[S_CF_PLUS].p, *minus = (unsigned long long*)c.slot[S_CF_MINUS].p;
    unsigned long long *ctl = (unsigned long long*)c.slot[S_CF_CTL].p, *part = pp.part;
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(unsigned long long), st));
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const dim3 blk(CF_BLOCK), gw((unsigned)((nwork + CF_BLOCK - 1) / CF_BLOCK)), gp((unsigned)pp.nblocks);
    if (nwork) {
        if (d_mask)
            hipLaunchKernelGGL((k_cf_init<true>), gw, blk, 0, st, (const double*)d_phi, L, nwork, plus, minus);
        else
            hipLaunchKernelGGL((k_cf_init<false>), gw, blk, 0, st, (const double*)d_phi, L, nwork, plus, minus);
    }
    // (with an empty list no particle can escape -- its 8 corners would be list cells -- and no key is touched)
    if (d_mask)
        hipLaunchKernelGGL((k_cf_scatter<true>), gp, blk, 0, st, G, d_pts, d_rad, npts, slack, plus, minus, d_status, part);
    else
        hipLaunchKernelGGL((k_cf_scatter<false>), gp, blk, 0, st, G, d_pts, d_rad, npts, slack, plus, minus, d_status, part);
    if (nwork) {
        if (d_mask)
            hipLaunchKernelGGL((k_cf_merge<true>), gw, blk, 0, st, d_phi, L, nwork, (const unsigned long long*)plus, (const unsigned long long*)minus, ctl);
        else
            hipLaunchKernelGGL((k_cf_merge<false>), gw, blk, 0, st, d_phi, L, nwork, (const unsigned long long*)plus, (const unsigned long long*)minus, ctl);
    }
    HIPCHK(hipGetLastError());
    unsigned long long hctl[2];
    HIPCHK(hipMemcpyAsync(hctl, ctl, sizeof hctl, hipMemcpyDeviceToHost, st));
    unsigned long long tot[CF_NPART];
    if ((rc = block_counts_finish(part, pp.nblocks, CF_NPART, tot, nullptr, st))) return rc; // (synchronises)
    if (change) std::memcpy(change, &hctl[1], sizeof(double));
    if (info) {
        for (int m = 0; m < CF_NPART; ++m) info[m] = (int64_t)tot[m];
        info[CF_NPART] = (int64_t)hctl[0];
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] correction: %d particles, %zu cells, %llu in place, %llu escaped, %llu outside, %llu off the band, %llu non-finite, %llu bad radius; %llu points changed\n",
                npts, nwork, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], hctl[0]);
    return LSF_OK;
}
