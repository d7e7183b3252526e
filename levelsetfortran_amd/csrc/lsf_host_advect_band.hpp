// lsf_host_advect_band.hpp -- host side of lsf_advect_field_band (kernels and design: lsf_advect_band.hpp): validation, the list
// (lsf_host_band.hpp), the scan of the inputs at list cells, the edge pass, the steps (one plain launch per stage over the list) and
// the closing pass.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// one stage launch over the list: the instance for the arithmetic and the terms present
void advect_band_stage_launch(bool strict, const double* A, double* B, const double* P0, const double* d_u, const double* d_v, const double* d_w,
                              const double* d_f, const int* L, int nL, int nchunks, int nx, int ny, int nz, double dx, double dt, double c_old,
                              double c_new, unsigned long long* part, const int* ctl, hipStream_t st)
{
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
    with_stage_instance<false>(strict, d_u != nullptr, d_f != nullptr, [&](auto S, auto HV, auto HF) {
        hipLaunchKernelGGL((k_advect_band_stage<decltype(S)::value, decltype(HV)::value, decltype(HF)::value>), grid, blk, 0, st, A, B, P0, d_u,
                           d_v, d_w, d_f, L, nL, nx, ny, nz, dx, dt, c_old, c_new, part, ctl);
    });
}

// Every error is found before anything is written: the arguments, then the list (the mask is read once), then the inputs at its
// cells.  info and margin are written on LSF_OK only.
int advect_band_core(double* d_phi, const int32_t* d_mask, const double* d_u, const double* d_v, const double* d_w, const double* d_f, int nx,
                     int ny, int nz, double dx, double dt, int steps, int scheme, int mode, int* steps_done, double* cfl, double* change_trace,
                     int trace_cap, int64_t* info, double* margin, hipStream_t st)
{
    int rc;
    if ((rc = advect_field_args_ok(d_phi, d_u, d_v, d_w, d_f, nx, ny, nz, dx, dt, steps, scheme, mode))) return rc;
    if (!d_mask) return fail(LSF_ERR_INVALID, "lsf_advect_field_band: mask is NULL");
    Ctx& c = ctx();
    const bool strict = (mode & LSF_ARITH_STRICT) != 0, rk3 = scheme == LSF_ADVECT_RK3;
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing to do, nothing written
        if (steps_done) *steps_done = 0;
        if (cfl) *cfl = 0.0;
        if (info) info[0] = info[1] = info[2] = 0;
        if (margin) *margin = HUGE_VAL;
        return LSF_OK;
    }
    const int* L = bl.L;
    const int nb = std::min(ADV_SCAN_BLOCKS, cdiv(nL, 256)); // blocks of the scan and of the closing pass
    if ((rc = ws(c.slot[S_PART2], (size_t)nb * 24))) return rc;
    std::vector<unsigned long long> h((size_t)3 * nb);

    // the inputs at list cells: cfl and the non-finite count
    {
        double* pmax = (double*)c.slot[S_PART2].p;
        hipLaunchKernelGGL(k_advect_band_scan, dim3((unsigned)nb), dim3(256), 0, st, d_u, d_v, d_w, d_f, L, nL, pmax, (unsigned long long*)(pmax + nb));
        if ((rc = advect_scan_finish(pmax, nb, dx, dt, cfl, "lsf_advect_field_band", " at list cells", st))) return rc;
    }
    if (steps_done) *steps_done = 0;

    // the edge pass: edge flag and entry sign per list entry, from the mask and the field as they came
    if ((rc = ws(c.slot[S_MB_BAND], (size_t)nL))) return rc;
    unsigned char* flag = (unsigned char*)c.slot[S_MB_BAND].p;
    const dim3 b256(256), gl((unsigned)nchunks);
    hipLaunchKernelGGL(k_advect_band_edge, gl, b256, 0, st, d_mask, (const double*)d_phi, L, nL, nx, ny, nz, flag);

    if (steps > 0) {
        const int tcap = change_trace ? std::max(0, std::min(steps, trace_cap)) : 0;
        if (rk3 && (rc = ws(c.slot[S_PONG2], n * sizeof(double)))) return rc;
        if ((rc = ws(c.slot[S_PART], (size_t)nchunks * sizeof(double)))) return rc;
        // the passes over the grid beyond the list build: the stage buffers start as copies of phi (points outside the list never change
        // in any of them).  The first was the staging of the list build, which is over (in stream order) before the field is copied into it.
        double* w1 = (double*)bl.staging;
        double* w2 = rk3 ? (double*)c.slot[S_PONG2].p : nullptr;
        HIPCHK(hipMemcpyAsync(w1, d_phi, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (rk3) HIPCHK(hipMemcpyAsync(w2, d_phi, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        StopLoop stop;
        if ((rc = stop.begin(c, tcap, st))) return rc;
        unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
        const int* ctl = stop.ctl;
        auto stage = [&](const double* A, double* B, const double* P0, double c_old, double c_new, bool last) {
            advect_band_stage_launch(strict, A, B, P0, d_u, d_v, d_w, d_f, L, nL, nchunks, nx, ny, nz, dx, dt, c_old, c_new, last ? part : nullptr,
                                     ctl, st);
        };
        double* bufs[2] = {d_phi, w1};
        for (int s = 0; s < steps; ++s) {
            if (rk3) rk3_stages(stage, d_phi, w1, w2);
            else stage(bufs[s & 1], bufs[(s + 1) & 1], nullptr, 0.0, 1.0, true);
            hipLaunchKernelGGL(k_advect_finish, dim3(1), dim3(RED_T), 0, st, (const unsigned long long*)part, (long)nchunks, stop.d_trace, tcap,
                               stop.ctl);
            if (stop.poll(s, steps)) break;
        }
        if ((rc = stop.finish())) return rc;
        const int nst = stop.count();
        // Euler, an odd number of steps: the result sits in the second buffer; its list cells are all that differs
        if (!rk3 && (nst & 1)) hipLaunchKernelGGL(k_rb_scatter, gl, b256, 0, st, L, (const double*)w1, nL, d_phi);
        HIPCHK(hipGetLastError());
        if ((rc = stop.verdict(change_trace, tcap, steps_done,
                               "lsf_advect_field_band: a list cell became NaN in step " + std::to_string(nst - 1) + " (0-based)")))
            return rc;
    }

    // the closing pass: edge cells, sign flips among them and the smallest |phi| there, finished in block order
    {
        unsigned long long* pmin = (unsigned long long*)c.slot[S_PART2].p;
        hipLaunchKernelGGL(k_advect_band_close, dim3((unsigned)nb), b256, 0, st, (const double*)d_phi, L, (const unsigned char*)flag, nL, pmin,
                           pmin + nb, pmin + 2 * nb);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h.data(), pmin, (size_t)nb * 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        unsigned long long mn = ADV_INF_BITS, ne = 0, nf = 0;
        for (int b = 0; b < nb; ++b) {
            mn = h[b] < mn ? h[b] : mn;
            ne += h[(size_t)nb + b];
            nf += h[(size_t)2 * nb + b];
        }
        if (info) info[0] = nL, info[1] = (int64_t)ne, info[2] = (int64_t)nf;
        if (margin) std::memcpy(margin, &mn, sizeof mn);
    }
    return LSF_OK;
}
