// lsf_host_measure_band.hpp -- host side of lsf_measure_band (kernels and design: lsf_measure_band.hpp; argument checks: lsf_host_args.hpp): the list, the
// two launches over it and the finish of the per-block partials in block order.  Included by lsf_api.hip inside its anonymous
// namespace.
#pragma once

// the arguments have passed measure_band_args_ok.  M and info are written on LSF_OK only.  Returns after the stream is synchronised.
int measure_band_core(const double* d_phi, const int32_t* d_mask, const double* d_q, double* d_cell, int nx, int ny, int nz, double dx,
                      const double xLo[3], double iso, double* M, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_count<true>(bl, nullptr, d_mask, nx, ny, nz, dx, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing to measure, nothing written
        for (int m = 0; m < LSF_MEASURE_LEN; ++m) M[m] = 0.0;
        if (info) info[0] = info[1] = info[2] = info[3] = info[4] = 0;
        return LSF_OK;
    }
    // (a grid whose brick keys do not fit 32 bits keeps the memory order: the order of the sum is then that one, still a function of
    // the mask alone)
    if ((rc = band_list_sort(bl, bl.keys_fit(), st))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * MS_NQ * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART2], (size_t)nchunks * MS_NCNT * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_MS_CTL], MS_CTL_LEN * sizeof(unsigned long long)))) return rc;
    double* part = (double*)c.slot[S_PART].p;
    unsigned long long* cnt = (unsigned long long*)c.slot[S_PART2].p;
    unsigned long long* ctl = (unsigned long long*)c.slot[S_MS_CTL].p;
    HIPCHK(hipMemsetAsync(ctl, 0, MS_CTL_LEN * sizeof(unsigned long long), st));
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
    // the validation pass comes first; the measuring pass leaves at once, before its one store, when it counted anything
    if (d_q)
        hipLaunchKernelGGL((k_measure_check<true>), grid, blk, 0, st, d_phi, d_q, (const int*)bl.L, nL, nx, ny, iso, ctl);
    else
        hipLaunchKernelGGL((k_measure_check<false>), grid, blk, 0, st, d_phi, d_q, (const int*)bl.L, nL, nx, ny, iso, ctl);
#define LSF_MS_CALL(HQ, HC) \
    hipLaunchKernelGGL((k_measure_band<HQ, HC>), grid, blk, 0, st, d_phi, d_mask, d_q, d_cell, (const int*)bl.L, nL, nx, ny, nz, dx, xLo[0], xLo[1], \
                       xLo[2], iso, (const unsigned long long*)ctl, part, cnt)
    switch ((d_q ? 2 : 0) | (d_cell ? 1 : 0)) {
    case 0: LSF_MS_CALL(false, false); break;
    case 1: LSF_MS_CALL(false, true); break;
    case 2: LSF_MS_CALL(true, false); break;
    default: LSF_MS_CALL(true, true); break;
    }
#undef LSF_MS_CALL
    HIPCHK(hipGetLastError());
    unsigned long long bad[MS_CTL_LEN];
    std::vector<double> hp((size_t)nchunks * MS_NQ);
    std::vector<unsigned long long> hc((size_t)nchunks * MS_NCNT);
    HIPCHK(hipMemcpyAsync(bad, ctl, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hc.data(), cnt, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad[MS_BAD_F])
        return fail(LSF_ERR_INVALID, "lsf_measure_band: " + std::to_string(bad[MS_BAD_F]) +
                                         " crossed edge(s) of measured cells with a non-finite phi - iso on an endpoint");
    if (bad[MS_BAD_Q])
        return fail(LSF_ERR_INVALID,
                    "lsf_measure_band: " + std::to_string(bad[MS_BAD_Q]) + " crossed edge(s) of measured cells with a non-finite q on an endpoint");
    double tot[MS_NQ];
    unsigned long long n[MS_NCNT] = {0, 0, 0, 0};
    for (int m = 0; m < MS_NQ; ++m) tot[m] = 0.0;
    for (int b = 0; b < nchunks; ++b) { // block order
        for (int m = 0; m < MS_NQ; ++m) tot[m] = tot[m] + hp[(size_t)b * MS_NQ + m];
        for (int m = 0; m < MS_NCNT; ++m) n[m] += hc[(size_t)b * MS_NCNT + m];
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] measures on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu crossed, %llu triangles, %llu open\n", nL,
                100.0 * nL / (double)bl.n, nchunks, n[0], n[1], n[2]);
    for (int m = 0; m < MS_NQ; ++m) M[m] = tot[m];
    if (info) info[0] = nL, info[1] = (int64_t)n[0], info[2] = (int64_t)n[1], info[3] = (int64_t)n[2], info[4] = (int64_t)n[3];
    return LSF_OK;
}
