// lsf_host_distance_fill.hpp -- host side of lsf_distance_fill (kernels and design: lsf_distance_fill.hpp; argument checks: lsf_host_args.hpp): the check
// pass, and the rounds of 8 raster sweeps, one plain launch per tile plane.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

int distance_fill_core(double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, double band, int max_rounds, int* rounds_done,
                       int64_t* changed_trace, int trace_cap, int64_t* frozen_points, hipStream_t st)
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
    if ((rc = ws(c.slot[S_DF_WORDS], (size_t)nwords * sizeof(uint32_t)))) return rc;
    if ((rc = ws(c.slot[S_DF_CNT], DF_N_COUNTERS * sizeof(unsigned long long)))) return rc;
    uint32_t* words = (uint32_t*)c.slot[S_DF_WORDS].p;
    unsigned long long* d_cnt = (unsigned long long*)c.slot[S_DF_CNT].p;
    const dim3 b256(256), gw((unsigned)((nwords + 7) / 8));

    // the check: read-only on the field
    unsigned long long cnt[DF_N_COUNTERS] = {0, 0, 0, 0};
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof cnt, st));
    hipLaunchKernelGGL(k_df_check, gw, b256, 0, st, (const double*)d_phi, d_mask, g, far, nwords, words, d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cnt[DF_N_FROZEN] == 0)
        return fail(LSF_ERR_INVALID, d_mask ? "lsf_distance_fill: no frozen point (the mask holds no 1)"
                                            : "lsf_distance_fill: no frozen point (no |phi| < band*dx)");
    if (cnt[DF_N_NONFINITE])
        return fail(LSF_ERR_INVALID, "lsf_distance_fill: " + std::to_string(cnt[DF_N_NONFINITE]) + " frozen point(s) hold a non-finite value");
    if (cnt[DF_N_JUMP])
        return fail(LSF_ERR_INVALID, "lsf_distance_fill: " + std::to_string(cnt[DF_N_JUMP]) +
                                         " pair(s) of axis neighbours of opposite sign are not both frozen (the frozen set must separate "
                                         "the signs)");

    hipLaunchKernelGGL(k_df_init, gw, b256, 0, st, d_phi, g, nwords, (const uint32_t*)words);
    const int nplanes = g.nTA + g.nTB + g.nTC - 2;
    const dim3 gt((unsigned)(g.nTB * g.nTC)), bt(DF_ROWS);
    int nr = 0;
    unsigned long long changed = 0;
    while (nr < max_rounds) {
        HIPCHK(hipMemsetAsync(d_cnt + DF_N_CHANGED, 0, sizeof(unsigned long long), st));
        for (int s = 0; s < 8; ++s)
            for (int P = 0; P < nplanes; ++P)
                hipLaunchKernelGGL(k_df_tile_plane, gt, bt, 0, st, d_phi, (const uint32_t*)words, g, P, RASTER_SIGN[s][0], RASTER_SIGN[s][1],
                                   RASTER_SIGN[s][2], dx, d_cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&changed, d_cnt + DF_N_CHANGED, sizeof changed, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (changed_trace && nr < trace_cap) changed_trace[nr] = (int64_t)changed;
        ++nr;
        if (changed == 0) break;
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] distance fill: %llu frozen points (%.2f %% of the grid), %d round(s) of 8 x %d launches, last count %llu\n",
                cnt[DF_N_FROZEN], 100.0 * (double)cnt[DF_N_FROZEN] / (double)n, nr, nplanes, changed);
    if (rounds_done) *rounds_done = nr;
    if (frozen_points) *frozen_points = (int64_t)cnt[DF_N_FROZEN];
    return LSF_OK;
}
