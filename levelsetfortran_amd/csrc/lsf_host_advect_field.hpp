// lsf_host_advect_field.hpp -- host side of lsf_advect_field (kernels and design: lsf_advect_field.hpp; argument checks: lsf_host_args.hpp): the scan of the
// inputs (CFL number, non-finite values) and the steps, one plain launch per stage.  Included by lsf_api.hip inside its anonymous
// namespace.
#pragma once

// The partials of k_advect_scan or k_advect_band_scan (nb maxima, then nb counts, enqueued on st) finished in block order:
// cfl = (dt * max (|u| + |v| + |w| + |speed|)) / dx; a non-finite input is LSF_ERR_INVALID with its count (`where` ends the message)
int advect_scan_finish(const double* pmax, int nb, double dx, double dt, double* cfl, const char* call, const char* where, hipStream_t st)
{
    HIPCHK(hipGetLastError());
    std::vector<double> h((size_t)2 * nb);
    HIPCHK(hipMemcpyAsync(h.data(), pmax, (size_t)nb * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double m = 0.0;
    unsigned long long bad = 0;
    for (int b = 0; b < nb; ++b) {
        unsigned long long k;
        std::memcpy(&k, &h[(size_t)nb + b], sizeof k);
        bad += k;
        m = h[b] > m ? h[b] : m;
    }
    if (bad) return fail(LSF_ERR_INVALID, std::string(call) + ": " + std::to_string(bad) + " non-finite value(s) in u, v, w, speed" + where);
    if (cfl) *cfl = (dt * m) / dx;
    return LSF_OK;
}

// read-only: the scan of the inputs over all points
int advect_field_scan(const double* d_u, const double* d_v, const double* d_w, const double* d_f, int nx, int ny, int nz, double dx, double dt,
                      double* cfl, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const long n = (long)(nx + 1) * (ny + 1) * (nz + 1);
    const int nb = (int)std::min<long>(ADV_SCAN_BLOCKS, (n + 255) / 256);
    if ((rc = ws(c.slot[S_PART2], (size_t)nb * 16))) return rc;
    double* pmax = (double*)c.slot[S_PART2].p;
    hipLaunchKernelGGL(k_advect_scan, dim3((unsigned)nb), dim3(256), 0, st, d_u, d_v, d_w, d_f, n, pmax, (unsigned long long*)(pmax + nb));
    return advect_scan_finish(pmax, nb, dx, dt, cfl, "lsf_advect_field", "", st);
}

// (strict, hv, hf) as compile-time constants: calls f(S, HV, HF) with std::true_type / std::false_type objects for the arithmetic and
// the terms present.  NONE: the instance without velocity and speed exists (the curvature stage); without it such a call takes the
// speed instance, as the stage launchers always did (the argument checks refuse it before).
template <bool NONE, class Fn>
void with_stage_instance(bool strict, bool hv, bool hf, Fn&& f)
{
    using Y = std::true_type;
    using N = std::false_type;
    auto terms = [&](auto S) {
        if (hv && hf) f(S, Y{}, Y{});
        else if (hv) f(S, Y{}, N{});
        else if (hf || !NONE) f(S, N{}, Y{});
        else if constexpr (NONE) f(S, N{}, N{});
    };
    if (strict) terms(Y{});
    else terms(N{});
}

// The three stages of a TVD-RK3 step (Shu and Osher) through stage(A, B, P0, c_old, c_new, last): phi -> w1, then w2 = 3/4 phi +
// 1/4 t(w1), then phi = 1/3 phi + 2/3 t(w2) in place (a lane reads the old phi at its own point only, before it stores there).
template <class Stage>
void rk3_stages(Stage&& stage, double* phi, double* w1, double* w2)
{
    stage(phi, w1, nullptr, 0.0, 1.0, false);
    stage(w1, w2, phi, 0.75, 0.25, false);
    stage(w2, phi, phi, 1. / 3., 2. / 3., true);
}

// one stage launch: the instance for the arithmetic and the terms present
void advect_stage_launch(bool strict, const double* A, double* B, const double* P0, const double* d_u, const double* d_v, const double* d_w,
                         const double* d_f, int nx, int ny, int nz, double dx, double dt, double c_old, double c_new, unsigned long long* part,
                         const int* ctl, int nbx, int nby, int nbz, hipStream_t st)
{
    const dim3 grid((unsigned)(((long)nbx * nby * nbz + 7) & ~7L)), blk(ADV_BX, ADV_BY);
    with_stage_instance<false>(strict, d_u != nullptr, d_f != nullptr, [&](auto S, auto HV, auto HF) {
        hipLaunchKernelGGL((k_advect_stage<decltype(S)::value, decltype(HV)::value, decltype(HF)::value>), grid, blk, 0, st, A, B, P0, d_u, d_v, d_w,
                           d_f, nx, ny, nz, dx, dt, c_old, c_new, part, ctl, nbx, nby, nbz);
    });
}

// the steps (arguments validated, inputs scanned, steps >= 1).  Workspace: one field for Euler, two for RK3.
int advect_field_steps(double* d_phi, const double* d_u, const double* d_v, const double* d_w, const double* d_f, int nx, int ny, int nz, double dx,
                       double dt, int steps, int scheme, int mode, int* steps_done, double* change_trace, int trace_cap, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const bool strict = (mode & LSF_ARITH_STRICT) != 0, rk3 = scheme == LSF_ADVECT_RK3;
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    const int nbx = cdiv(nx - 1, ADV_BX), nby = cdiv(ny - 1, ADV_BY), nbz = cdiv(nz - 1, ADV_KC);
    const long nblk = (long)nbx * nby * nbz;
    if (nblk > 0x7ffffff0L) return fail(LSF_ERR_INVALID, "lsf_advect_field: too many blocks for one launch");
    const BcWhole bc = bc_whole(nx, ny, nz);
    const int tcap = change_trace ? std::max(0, std::min(steps, trace_cap)) : 0;
    if ((rc = ws(c.slot[S_PONG], n * sizeof(double)))) return rc;
    if (rk3 && (rc = ws(c.slot[S_PONG2], n * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)(nblk + bc.nparts) * sizeof(double)))) return rc;
    StopLoop stop;
    if ((rc = stop.begin(c, tcap, st))) return rc;
    double* w1 = (double*)c.slot[S_PONG].p;
    double* w2 = rk3 ? (double*)c.slot[S_PONG2].p : nullptr;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    double* part_bc = (double*)(part + nblk); // k_bc's sums of squares: written, never read
    int* ctl = stop.ctl;

    auto stage = [&](const double* A, double* B, const double* P0, double c_old, double c_new, bool last) {
        advect_stage_launch(strict, A, B, P0, d_u, d_v, d_w, d_f, nx, ny, nz, dx, dt, c_old, c_new, last ? part : nullptr, ctl, nbx, nby, nbz, st);
        // the extrapolation boundary condition on the stage's output (subs.f90:859-897)
        hipLaunchKernelGGL(k_bc<double>, bc.grid, dim3(64), 0, st, A, B, bc.bx, 0, 0, 0, nx + 1, ny + 1, nz + 1, dx, part_bc, (const int*)ctl, 0, bc.faces);
    };
    double* bufs[2] = {d_phi, w1};
    for (int s = 0; s < steps; ++s) {
        if (rk3) rk3_stages(stage, d_phi, w1, w2);
        else stage(bufs[s & 1], bufs[(s + 1) & 1], nullptr, 0.0, 1.0, true);
        hipLaunchKernelGGL(k_advect_finish, dim3(1), dim3(RED_T), 0, st, (const unsigned long long*)part, nblk, stop.d_trace, tcap, ctl);
        if (stop.poll(s, steps)) break;
    }
    if ((rc = stop.finish())) return rc;
    const int nst = stop.count();
    if (!rk3 && (nst & 1)) HIPCHK(hipMemcpyAsync(d_phi, w1, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    return stop.verdict(change_trace, tcap, steps_done, "lsf_advect_field: the field became NaN in step " + std::to_string(nst - 1) + " (0-based)");
}
