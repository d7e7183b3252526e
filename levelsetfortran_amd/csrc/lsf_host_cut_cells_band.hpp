// lsf_host_cut_cells_band.hpp -- host side of lsf_cut_cells_band (kernel and design: lsf_cut_cells_band.hpp; argument checks:
// lsf_host_args_cut.hpp): the list, the control words, the two launches over it and the finish of the per-block partials in block
// order (the list, the flags and the counts through lsf_host_band.hpp).  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed cut_cells_args_ok.  volume, vof_min and info are written on LSF_OK only.  Returns after the stream is
// synchronised.
int cut_cells_core(const double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, double iso, double* d_vof, double* d_ax,
                   double* d_ay, double* d_az, double* d_bx, double* d_by, double* d_bz, double* volume, double* vof_min, int64_t* info,
                   hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing written
        if (volume) *volume = 0.0;
        if (vof_min) *vof_min = INFINITY;
        if (info) info[0] = info[1] = info[2] = info[3] = info[4] = 0;
        return LSF_OK;
    }
    // per block one fp64 partial and one 64-bit key (S_PART), four counts (S_PART2)
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * 2 * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART2], (size_t)nchunks * CC_NCNT * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_MS_CTL], MS_CTL_LEN * sizeof(unsigned long long)))) return rc;
    double* part = (double*)c.slot[S_PART].p;
    unsigned long long* key = (unsigned long long*)(part + nchunks);
    unsigned long long* cnt = (unsigned long long*)c.slot[S_PART2].p;
    unsigned long long* ctl = (unsigned long long*)c.slot[S_MS_CTL].p;
    HIPCHK(hipMemsetAsync(ctl, 0, MS_CTL_LEN * sizeof(unsigned long long), st));
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
    // the validation pass of lsf_measure_band comes first; the cell pass leaves at once, before its stores, when it counted anything
    hipLaunchKernelGGL((k_measure_check<false>), grid, blk, 0, st, d_phi, (const double*)nullptr, (const int*)bl.L, nL, nx, ny, iso, ctl);
    with_flags(
        [&](auto HV, auto HA, auto HB) {
            hipLaunchKernelGGL((k_cut_cells_band<decltype(HV)::value, decltype(HA)::value, decltype(HB)::value>), grid, blk, 0, st, d_phi, d_mask,
                               d_vof, d_ax, d_ay, d_az, d_bx, d_by, d_bz, (const int*)bl.L, nL, nx, ny, nz, iso, (const unsigned long long*)ctl, part,
                               key, cnt);
        },
        d_vof != nullptr, d_ax != nullptr, d_bx != nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long bad[MS_CTL_LEN], n[CC_NCNT];
    std::vector<double> hp((size_t)nchunks * 2);
    HIPCHK(hipMemcpyAsync(bad, ctl, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if ((rc = block_counts_finish(cnt, nchunks, CC_NCNT, n, nullptr, st))) return rc; // (the third copy; synchronises)
    if (bad[MS_BAD_F])
        return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: " + std::to_string(bad[MS_BAD_F]) +
                                         " crossed edge(s) of listed cells with a non-finite phi - iso on an endpoint");
    double tot = 0.0;
    unsigned long long kmin = 0x7ff0000000000000ull;
    for (int b = 0; b < nchunks; ++b) { // block order
        unsigned long long k;
        memcpy(&k, &hp[(size_t)nchunks + b], sizeof k);
        tot = tot + hp[b];
        kmin = k < kmin ? k : kmin;
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] cut cells on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu cut, %llu full, %llu open, %llu clamped\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, n[0], n[1], n[2], n[3]);
    if (volume) *volume = tot * ((dx * dx) * dx);
    if (vof_min) memcpy(vof_min, &kmin, sizeof kmin);
    if (info) info[0] = nL, info[1] = (int64_t)n[0], info[2] = (int64_t)n[1], info[3] = (int64_t)n[2], info[4] = (int64_t)n[3];
    return LSF_OK;
}
