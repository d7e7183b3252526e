// lsf_host_extend_field.hpp -- host side of lsf_extend_field (kernels and design: lsf_extend_field.hpp; argument checks: lsf_host_args.hpp): the check pass,
// the rounds of 8 raster sweeps, one plain launch per tile plane, and the final count.  Included by lsf_api.hip inside its anonymous
// namespace.
#pragma once

int extend_field_core(double* d_q, const double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, double band, int max_rounds,
                      int* rounds_done, int64_t* changed_trace, int trace_cap, int64_t* info, hipStream_t st)
{
    int rc;
    if (rounds_done) *rounds_done = 0;
    DfGrid g;
    g.NX = nx + 1, g.NY = ny + 1, g.NZ = nz + 1;
    g.nTA = cdiv(g.NX, DF_TX), g.nTB = cdiv(g.NY, DF_TY), g.nTC = cdiv(g.NZ, DF_TZ);
    const size_t n = (size_t)g.NX * g.NY * g.NZ;
    const long long nwords = (long long)g.nTA * g.NY * g.NZ;
    const double far = d_mask ? 0.0 : band * dx;
    Ctx& c = ctx();
    if ((rc = ws(c.slot[S_EXT_WORDS], (size_t)nwords * sizeof(uint32_t)))) return rc;
    if ((rc = ws(c.slot[S_EXT_CNT], EXT_N_COUNTERS * sizeof(unsigned long long)))) return rc;
    uint32_t* words = (uint32_t*)c.slot[S_EXT_WORDS].p;
    unsigned long long* d_cnt = (unsigned long long*)c.slot[S_EXT_CNT].p;
    const dim3 b256(256), gw((unsigned)((nwords + 7) / 8));

    // the check: read-only on all three arrays
    unsigned long long cnt[EXT_N_COUNTERS] = {0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof cnt, st));
    hipLaunchKernelGGL(k_ext_check, gw, b256, 0, st, (const double*)d_q, d_phi, d_mask, g, far, nwords, words, d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cnt[EXT_N_BADPHI])
        return fail(LSF_ERR_INVALID, "lsf_extend_field: " + std::to_string(cnt[EXT_N_BADPHI]) + " point(s) hold a non-finite phi");
    if (cnt[EXT_N_FROZEN] == 0)
        return fail(LSF_ERR_INVALID, d_mask ? "lsf_extend_field: no frozen point (the mask holds no 1)"
                                            : "lsf_extend_field: no frozen point (no |phi| < band*dx)");
    if (cnt[EXT_N_BADQ])
        return fail(LSF_ERR_INVALID, "lsf_extend_field: " + std::to_string(cnt[EXT_N_BADQ]) + " frozen point(s) hold a non-finite q");

    hipLaunchKernelGGL(k_ext_init, gw, b256, 0, st, d_q, g, nwords, (const uint32_t*)words);
    const int nplanes = g.nTA + g.nTB + g.nTC - 2;
    const dim3 gt((unsigned)(g.nTB * g.nTC)), bt(DF_ROWS);
    int nr = 0;
    unsigned long long changed = 0;
    while (nr < max_rounds) {
        HIPCHK(hipMemsetAsync(d_cnt + EXT_N_CHANGED, 0, sizeof(unsigned long long), st));
        for (int s = 0; s < 8; ++s)
            for (int P = 0; P < nplanes; ++P)
                hipLaunchKernelGGL(k_ext_tile_plane, gt, bt, 0, st, d_q, d_phi, (const uint32_t*)words, g, P, RASTER_SIGN[s][0], RASTER_SIGN[s][1],
                                   RASTER_SIGN[s][2], d_cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&changed, d_cnt + EXT_N_CHANGED, sizeof changed, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (changed_trace && nr < trace_cap) changed_trace[nr] = (int64_t)changed;
        ++nr;
        if (changed == 0) break;
    }
    hipLaunchKernelGGL(k_ext_count, gw, b256, 0, st, (const double*)d_q, g, nwords, (const uint32_t*)words, d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt + EXT_N_REACHED, d_cnt + EXT_N_REACHED, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] extend field: %llu frozen points (%.2f %% of the grid), %d round(s) of 8 x %d launches, last count %llu, "
                        "%llu unreached\n",
                cnt[EXT_N_FROZEN], 100.0 * (double)cnt[EXT_N_FROZEN] / (double)n, nr, nplanes, changed, cnt[EXT_N_UNREACHED]);
    if (rounds_done) *rounds_done = nr;
    if (info) info[0] = (int64_t)cnt[EXT_N_FROZEN], info[1] = (int64_t)cnt[EXT_N_REACHED], info[2] = (int64_t)cnt[EXT_N_UNREACHED];
    return LSF_OK;
}
