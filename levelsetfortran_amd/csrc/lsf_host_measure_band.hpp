// lsf_host_measure_band.hpp -- host side of lsf_measure_band (kernels and design: lsf_measure_band.hpp; argument checks: lsf_host_args.hpp): the list, the
// two launches over it and the finish of the per-block partials in block order (the list, the flags and the counts through
// lsf_host_band.hpp; the fp64 sums here: their order is the contract).  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed measure_band_args_ok.  M and info are written on LSF_OK only.  Returns after the stream is synchronised.
int measure_band_core(const double* d_phi, const int32_t* d_mask, const double* d_q, double* d_cell, int nx, int ny, int nz, double dx,
                      const double xLo[3], double iso, double* M, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing to measure, nothing written
        for (int m = 0; m < LSF_MEASURE_LEN; ++m) M[m] = 0.0;
        if (info) info[0] = info[1] = info[2] = info[3] = info[4] = 0;
        return LSF_OK;
    }
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * MS_NQ * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART2], (size_t)nchunks * MS_NCNT * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_MS_CTL], MS_CTL_LEN * sizeof(unsigned long long)))) return rc;
    double* part = (double*)c.slot[S_PART].p;
    unsigned long long* cnt = (unsigned long long*)c.slot[S_PART2].p;
    unsigned long long* ctl = (unsigned long long*)c.slot[S_MS_CTL].p;
    HIPCHK(hipMemsetAsync(ctl, 0, MS_CTL_LEN * sizeof(unsigned long long), st));
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
    // the validation pass comes first; the measuring pass leaves at once, before its one store, when it counted anything
    with_flags(
        [&](auto HQ, auto HC) {
            hipLaunchKernelGGL((k_measure_check<decltype(HQ)::value>), grid, blk, 0, st, d_phi, d_q, (const int*)bl.L, nL, nx, ny, iso, ctl);
            hipLaunchKernelGGL((k_measure_band<decltype(HQ)::value, decltype(HC)::value>), grid, blk, 0, st, d_phi, d_mask, d_q, d_cell,
                               (const int*)bl.L, nL, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2], iso, (const unsigned long long*)ctl, part, cnt);
        },
        d_q != nullptr, d_cell != nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long bad[MS_CTL_LEN], n[MS_NCNT];
    std::vector<double> hp((size_t)nchunks * MS_NQ);
    HIPCHK(hipMemcpyAsync(bad, ctl, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if ((rc = block_counts_finish(cnt, nchunks, MS_NCNT, n, nullptr, st))) return rc; // (the third copy; synchronises)
    if (bad[MS_BAD_F])
        return fail(LSF_ERR_INVALID, "lsf_measure_band: " + std::to_string(bad[MS_BAD_F]) +
                                         " crossed edge(s) of measured cells with a non-finite phi - iso on an endpoint");
    if (bad[MS_BAD_Q])
        return fail(LSF_ERR_INVALID,
                    "lsf_measure_band: " + std::to_string(bad[MS_BAD_Q]) + " crossed edge(s) of measured cells with a non-finite q on an endpoint");
    double tot[MS_NQ];
    for (int m = 0; m < MS_NQ; ++m) tot[m] = 0.0;
    for (int b = 0; b < nchunks; ++b) // block order
        for (int m = 0; m < MS_NQ; ++m) tot[m] = tot[m] + hp[(size_t)b * MS_NQ + m];
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] measures on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu crossed, %llu triangles, %llu open\n", nL,
                100.0 * nL / (double)bl.n, nchunks, n[0], n[1], n[2]);
    for (int m = 0; m < MS_NQ; ++m) M[m] = tot[m];
    if (info) info[0] = nL, info[1] = (int64_t)n[0], info[2] = (int64_t)n[1], info[3] = (int64_t)n[2], info[4] = (int64_t)n[3];
    return LSF_OK;
}
