// lsf_host_evolve_band.hpp -- host side of lsf_evolve_band and lsf_evolve_band_curv (kernels and design: lsf_evolve_band.hpp; the
// stage with the curvature term: lsf_evolve_band_curv.hpp; lsf_evolve_band is bcurv = clamp = 0; argument checks: lsf_host_args.hpp): the scan of the
// inputs over all points, the first list (lsf_host_band.hpp), the steps (stages and sweeps enqueued on the resident list), the checks (one 64-byte
// record read per check) and the rebuilds.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// one stage launch over the list with the curvature term: the instance for the arithmetic and the terms present
void advect_band_curv_stage_launch(bool strict, const double* A, double* B, const double* P0, const double* d_u, const double* d_v,
                                   const double* d_w, const double* d_f, const int* L, int nL, int nchunks, int nx, int ny, int nz, double dx,
                                   double dt, double c_old, double c_new, double bcurv, double lim, unsigned long long* part, const int* ctl,
                                   hipStream_t st)
{
    const dim3 grid((unsigned)nchunks), blk(MB_CH);
    const double two_dx = 2. * dx, dx2 = dx * dx, four_dx2 = 4. * dx2;
    with_stage_instance<true>(strict, d_u != nullptr, d_f != nullptr, [&](auto S, auto HV, auto HF) {
        hipLaunchKernelGGL((k_advect_band_curv_stage<decltype(S)::value, decltype(HV)::value, decltype(HF)::value>), grid, blk, 0, st, A, B, P0,
                           d_u, d_v, d_w, d_f, L, nL, nx, ny, nz, dx, dt, c_old, c_new, bcurv, two_dx, dx2, four_dx2, lim, part, ctl);
    });
}

// Every error is found before anything is written: the arguments, then the inputs at all points.  info and margin are written on
// LSF_OK only; phi and the mask on LSF_OK and LSF_ERR_NAN.
int evolve_band_core(double* d_phi, int32_t* d_mask, const double* d_u, const double* d_v, const double* d_w, const double* d_f, int nx, int ny,
                     int nz, double dx, double dt, int steps, int scheme, int mode, double core, int ring, int reinit_sweeps, double h,
                     int check_every, double bcurv, double clamp, int* steps_done, double* cfl, double* diffusion, double* change_trace,
                     int trace_cap, int64_t* info, double* margin, hipStream_t st)
{
    int rc;
    if ((rc = evolve_band_args_ok(d_phi, d_mask, d_u, d_v, d_w, d_f, nx, ny, nz, dx, dt, steps, scheme, mode, core, ring, reinit_sweeps, h,
                                  check_every, bcurv, clamp)))
        return rc;
    double cfl_all = 0.0; // stays 0 without a velocity and a speed: nothing to scan
    if ((d_u || d_f) && (rc = advect_field_scan(d_u, d_v, d_w, d_f, nx, ny, nz, dx, dt, &cfl_all, st))) return rc;
    const double diff = (bcurv * dt) / (dx * dx);                   // reported, never judged
    const double lim = clamp != 0.0 ? clamp / dx : HUGE_VAL; // no clamp: a bound that no H exceeds
    Ctx& c = ctx();
    const bool strict = (mode & LSF_ARITH_STRICT) != 0, rk3 = scheme == LSF_ADVECT_RK3;
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    const double core_dx = core * dx, far = (core + (double)ring) * dx;
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    if (bl.nL <= 0) { // empty list: the mask is normalised (all 0), nothing else is written
        HIPCHK(hipMemsetAsync(d_mask, 0, n * sizeof(int32_t), st));
        HIPCHK(hipStreamSynchronize(st));
        if (steps_done) *steps_done = 0;
        if (cfl) *cfl = 0.0;
        if (diffusion) *diffusion = diff;
        if (info)
            for (int q = 0; q < LSF_EVOLVE_INFO_LEN; ++q) info[q] = 0;
        if (margin) *margin = HUGE_VAL;
        return LSF_OK;
    }
    // the stage buffers are not the staging of the list build (S_PONG): a rebuild stages a list while they hold the field
    if ((rc = ws(c.slot[S_PONG2], n * sizeof(double)))) return rc;
    if (rk3 && (rc = ws(c.slot[S_PONG3], n * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART2], (size_t)(4 * EVB_CHECK_BLOCKS + EVB_R_WORDS) * sizeof(unsigned long long)))) return rc;
    double* w1 = (double*)c.slot[S_PONG2].p;
    double* w2 = rk3 ? (double*)c.slot[S_PONG3].p : nullptr;
    unsigned long long* cpart = (unsigned long long*)c.slot[S_PART2].p;
    unsigned long long* rec = cpart + 4 * EVB_CHECK_BLOCKS;
    const int tcap = change_trace ? std::max(0, std::min(steps, trace_cap)) : 0;
    StopLoop stop;
    if ((rc = stop.begin(c, tcap, st))) return rc;
    const int* ctl = stop.ctl;

    // what depends on the length of the list: fetched again after every rebuild (ws may move a slot that grows)
    const int* L = nullptr;
    int nL = 0, nchunks = 0;
    unsigned char* flag = nullptr;
    unsigned long long* part = nullptr;
    double* ps = nullptr;
    const dim3 b256(256);
    auto adopt = [&]() -> int {
        int r;
        L = bl.L, nL = bl.nL, nchunks = bl.nchunks;
        if ((r = ws(c.slot[S_MB_BAND], (size_t)nL))) return r;
        if ((r = ws(c.slot[S_PART], (size_t)nchunks * sizeof(double)))) return r;
        if (reinit_sweeps > 0 && (r = ws(c.slot[S_RB_PHIS], (size_t)nL * sizeof(double)))) return r;
        flag = (unsigned char*)c.slot[S_MB_BAND].p, part = (unsigned long long*)c.slot[S_PART].p, ps = (double*)c.slot[S_RB_PHIS].p;
        return LSF_OK;
    };
    if ((rc = adopt())) return rc;

    // from here on phi and the mask are written
    if (cfl) *cfl = cfl_all;
    if (diffusion) *diffusion = diff;
    if (steps_done) *steps_done = 0;
    HIPCHK(hipMemsetAsync(d_mask, 0, n * sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(rec, 0, EVB_R_WORDS * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_evb_set, dim3((unsigned)nchunks), b256, 0, st, L, nL, d_mask);
    hipLaunchKernelGGL(k_evb_edge, dim3((unsigned)nchunks), b256, 0, st, (const int32_t*)d_mask, (const double*)d_phi, L, nL, nx, ny, nz, flag);

    unsigned long long hrec[EVB_R_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool rec_current = false; // hrec describes the list and the field as they are
    auto check = [&]() -> int {
        const int nb = std::min(EVB_CHECK_BLOCKS, cdiv(nL, 256));
        hipLaunchKernelGGL(k_evb_check, dim3((unsigned)nb), b256, 0, st, (const double*)d_phi, L, (const unsigned char*)flag, nL, core_dx, cpart, nb);
        hipLaunchKernelGGL(k_evb_check_finish, dim3(1), b256, 0, st, (const unsigned long long*)cpart, nb, ctl, rec);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hrec, rec, sizeof hrec, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        rec_current = true;
        return LSF_OK;
    };
    int64_t rebuilds = 0;
    auto rebuild = [&]() -> int {
        int r;
        if ((r = ws(c.slot[S_EVB_MASK], n * sizeof(int32_t)))) return r;
        int32_t* scratch = (int32_t*)c.slot[S_EVB_MASK].p;
        const dim3 gl((unsigned)nchunks);
        HIPCHK(hipMemsetAsync(scratch, 0, n * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_evb_dilate, gl, b256, 0, st, (const double*)d_phi, L, nL, nx, ny, nz, core_dx, ring, scratch);
        hipLaunchKernelGGL(k_evb_leave, gl, b256, 0, st, L, nL, (const double*)d_phi, w1, w2, (const int32_t*)scratch, d_mask);
        BandList nw;
        if ((r = band_list_build(nw, scratch, nx, ny, nz, dx, true, st))) return r; // (waits: the old list is no longer in use)
        if (nw.nL <= 0) return fail(LSF_ERR_HIP, "lsf_evolve_band: a rebuild found no core cell"); // (cannot be: the margin cell is one)
        bl = nw;
        if ((r = adopt())) return r;
        const dim3 gn((unsigned)nchunks);
        hipLaunchKernelGGL(k_evb_enter, gn, b256, 0, st, L, nL, far, d_phi, w1, w2, d_mask, part);
        hipLaunchKernelGGL(k_evb_enter_finish, dim3(1), b256, 0, st, (const unsigned long long*)part, nchunks, rec);
        hipLaunchKernelGGL(k_evb_edge, gn, b256, 0, st, (const int32_t*)d_mask, (const double*)d_phi, L, nL, nx, ny, nz, flag);
        HIPCHK(hipGetLastError());
        ++rebuilds;
        rec_current = false;
        return LSF_OK;
    };

    if (steps > 0) {
        // the one pass over the field per buffer: the stage buffers start as copies of phi and equal it off-list from then on
        HIPCHK(hipMemcpyAsync(w1, d_phi, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (rk3) HIPCHK(hipMemcpyAsync(w2, d_phi, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        auto stage = [&](const double* A, double* B, const double* P0, double c_old, double c_new, bool last) {
            if (bcurv == 0.0) // lsf_evolve_band's stage kernel, bit for bit
                advect_band_stage_launch(strict, A, B, P0, d_u, d_v, d_w, d_f, L, nL, nchunks, nx, ny, nz, dx, dt, c_old, c_new, last ? part : nullptr,
                                         ctl, st);
            else
                advect_band_curv_stage_launch(strict, A, B, P0, d_u, d_v, d_w, d_f, L, nL, nchunks, nx, ny, nz, dx, dt, c_old, c_new, bcurv, lim,
                                              last ? part : nullptr, ctl, st);
        };
        for (int s = 0; s < steps; ++s) {
            const dim3 gl((unsigned)nchunks);
            double* cur = d_phi; // the buffer that holds the state
            if (rk3) {
                rk3_stages(stage, d_phi, w1, w2);
            } else {
                stage(d_phi, w1, nullptr, 0.0, 1.0, true);
                cur = w1;
            }
            hipLaunchKernelGGL(k_advect_finish, dim3(1), dim3(RED_T), 0, st, (const unsigned long long*)part, (long)nchunks, stop.d_trace, tcap,
                               stop.ctl);
            if (reinit_sweeps > 0) {
                hipLaunchKernelGGL(k_rb_gather, gl, b256, 0, st, L, (const double*)cur, nL, ps);
                for (int q = 0; q < reinit_sweeps; ++q) { // (the sums of squares go to the partials of the stages: written, never read)
                    double* other = cur == d_phi ? w1 : d_phi;
                    with_flags(
                        [&](auto S) {
                            hipLaunchKernelGGL((k_reinit_band<decltype(S)::value>), gl, b256, 0, st, (const double*)cur, other, (const double*)ps, L, nL,
                                               nx, ny, nz, dx, h, (double*)part, ctl);
                        },
                        strict);
                    cur = other;
                }
            }
            if (cur != d_phi) hipLaunchKernelGGL(k_evb_scatter, gl, b256, 0, st, L, (const double*)w1, nL, d_phi, ctl);
            rec_current = false;
            if ((s + 1) % check_every == 0 || s == steps - 1) {
                if ((rc = check())) return rc;
                if (hrec[EVB_R_STOP] || hrec[EVB_R_FLIPS]) break; // a NaN step, or the surface reached the open edge
                double m;
                std::memcpy(&m, &hrec[EVB_R_MARGIN], sizeof m);
                if (m < core_dx && (rc = rebuild())) return rc;
            }
        }
        if ((rc = stop.finish())) return rc;
        const int nst = stop.count();
        // a NaN step of Euler: the step's result sits in the stage buffer; its list cells are all that differs
        if (!rk3 && stop.stopped()) hipLaunchKernelGGL(k_rb_scatter, dim3((unsigned)nchunks), b256, 0, st, L, (const double*)w1, nL, d_phi);
        HIPCHK(hipGetLastError());
        if ((rc = stop.verdict(change_trace, tcap, steps_done, "lsf_evolve_band: a list cell became NaN in step " + std::to_string(nst - 1) + " (0-based)")))
            return rc;
    }
    if (!rec_current && (rc = check())) return rc;
    if (info) {
        info[0] = nL, info[1] = (int64_t)hrec[EVB_R_OPEN], info[2] = (int64_t)hrec[EVB_R_FLIPS], info[3] = rebuilds;
        info[4] = (int64_t)hrec[EVB_R_ENTERED], info[5] = (int64_t)hrec[EVB_R_WALL];
    }
    if (margin) std::memcpy(margin, &hrec[EVB_R_MARGIN], sizeof(double));
    return LSF_OK;
}
