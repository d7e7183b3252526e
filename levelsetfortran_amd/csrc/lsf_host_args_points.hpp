// lsf_host_args_points.hpp -- the argument checks of lsf_advect_points, lsf_correct_field and lsf_reseed_points, in the style and under the rules of
// lsf_host_args.hpp, which it is included after (its shared checks and fail() are used here): pure host code, addresses compared and
// never followed, xLo a host array on both seams, the ORDER of the checks behaviour.  tests/host_args/points_args_main.cpp runs a
// table of argument lists through the first two on the CPU (tests/test_points_cpu.py), tests/host_args/reseed_args_main.cpp through the
// third (tests/test_reseed_cpu.py).
#pragma once

int advect_points_args_ok(const void* u, const void* v, const void* w, const void* phi, const void* speed, const void* mask, int nx, int ny, int nz,
                          double dx, const double* xLo, const void* pts, int npts, int order, int scheme, double dt, int nsteps, const void* status)
{
    int rc;
    if (!pts) return fail(LSF_ERR_INVALID, "lsf_advect_points: pts is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_advect_points: xLo is NULL");
    const int nvel = (u != nullptr) + (v != nullptr) + (w != nullptr);
    if (nvel != 0 && nvel != 3)
        return fail(LSF_ERR_INVALID, "lsf_advect_points: u, v, w are given together or all NULL (" + std::to_string(nvel) + " of 3 given)");
    if (!nvel && !speed) return fail(LSF_ERR_INVALID, "lsf_advect_points: neither a velocity (u, v, w) nor a speed is given");
    if (speed && !phi) return fail(LSF_ERR_INVALID, "lsf_advect_points: speed without phi (the speed acts along the normal of phi)");
    if (phi && !speed) return fail(LSF_ERR_INVALID, "lsf_advect_points: phi without speed");
    if (npts < 1) return fail(LSF_ERR_INVALID, "lsf_advect_points: npts must be >= 1");
    if ((rc = grid_ok("lsf_advect_points", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_advect_points: dx must be finite and > 0");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "lsf_advect_points: xLo must hold three finite values");
    if (!std::isfinite(dt)) return fail(LSF_ERR_INVALID, "lsf_advect_points: dt must be finite");
    if (order != LSF_SAMPLE_LINEAR && order != LSF_SAMPLE_CUBIC) return fail(LSF_ERR_INVALID, "lsf_advect_points: unknown order");
    if (scheme != LSF_ADVECT_RK3 && scheme != LSF_ADVECT_EULER)
        return fail(LSF_ERR_INVALID, "lsf_advect_points: unknown scheme (LSF_ADVECT_RK3 or LSF_ADVECT_EULER)");
    if (nsteps < 1 || nsteps > LSF_ADVECT_POINTS_MAX_STEPS)
        return fail(LSF_ERR_INVALID, "lsf_advect_points: nsteps must be in 1.." + std::to_string(LSF_ADVECT_POINTS_MAX_STEPS));
    const size_t n = grid_points(nx, ny, nz), np = (size_t)npts, fb = n * sizeof(double);
    const void* a[8] = {u, v, w, phi, speed, mask, pts, status};
    const size_t bytes[8] = {fb, fb, fb, fb, fb, n * sizeof(int32_t), 3 * np * sizeof(double), np * sizeof(int32_t)};
    const char* name[8] = {"u", "v", "w", "phi", "speed", "mask", "pts", "status"};
    return overlap_ok("lsf_advect_points", 8, a, bytes, name, 6);
}

int correct_field_args_ok(const void* phi, const void* mask, int nx, int ny, int nz, double dx, const double* xLo, const void* pts, const void* rad,
                          int npts, double slack, const void* status)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_correct_field: phi is NULL");
    if (!pts) return fail(LSF_ERR_INVALID, "lsf_correct_field: pts is NULL");
    if (!rad) return fail(LSF_ERR_INVALID, "lsf_correct_field: rad is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_correct_field: xLo is NULL");
    if (npts < 1) return fail(LSF_ERR_INVALID, "lsf_correct_field: npts must be >= 1");
    if ((rc = grid_ok("lsf_correct_field", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_correct_field: dx must be finite and > 0");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "lsf_correct_field: xLo must hold three finite values");
    if (!finite_nonneg(slack)) return fail(LSF_ERR_INVALID, "lsf_correct_field: slack must be finite and >= 0");
    const size_t n = grid_points(nx, ny, nz), np = (size_t)npts;
    const void* a[5] = {mask, pts, rad, phi, status};
    const size_t bytes[5] = {n * sizeof(int32_t), 3 * np * sizeof(double), np * sizeof(double), n * sizeof(double), np * sizeof(int32_t)};
    const char* name[5] = {"mask", "pts", "rad", "phi", "status"};
    return overlap_ok("lsf_correct_field", 5, a, bytes, name, 3);
}

// (npts + candidates <= 2^31 - 1 is checked on the device's count, lsf_host_reseed.hpp)
int reseed_points_args_ok(const void* phi, const void* mask, int nx, int ny, int nz, double dx, const double* xLo, const void* pts, const void* rad,
                          int npts, int per_cell, double rmin, double rmax, double band, int order, int iters, double tol, const void* status,
                          const int* nout)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_reseed_points: phi is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_reseed_points: xLo is NULL");
    if (!nout) return fail(LSF_ERR_INVALID, "lsf_reseed_points: nout is NULL");
    if (npts < 0) return fail(LSF_ERR_INVALID, "lsf_reseed_points: npts must be >= 0");
    if (npts > 0 && !pts) return fail(LSF_ERR_INVALID, "lsf_reseed_points: pts is NULL with npts > 0");
    if (npts > 0 && !rad) return fail(LSF_ERR_INVALID, "lsf_reseed_points: rad is NULL with npts > 0");
    if ((rc = grid_ok("lsf_reseed_points", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_reseed_points: dx must be finite and > 0");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "lsf_reseed_points: xLo must hold three finite values");
    if (per_cell < 1 || per_cell > LSF_RESEED_MAX_PER_CELL)
        return fail(LSF_ERR_INVALID, "lsf_reseed_points: per_cell must be in 1.." + std::to_string(LSF_RESEED_MAX_PER_CELL));
    if (!std::isfinite(rmin) || !std::isfinite(rmax) || !std::isfinite(band))
        return fail(LSF_ERR_INVALID, "lsf_reseed_points: rmin, rmax and band must be finite");
    if (!(0.0 < rmin && rmin <= rmax)) return fail(LSF_ERR_INVALID, "lsf_reseed_points: 0 < rmin <= rmax is required");
    if (!(rmin < band)) return fail(LSF_ERR_INVALID, "lsf_reseed_points: rmin < band is required");
    if (order != LSF_SAMPLE_LINEAR && order != LSF_SAMPLE_CUBIC) return fail(LSF_ERR_INVALID, "lsf_reseed_points: unknown order");
    if (iters < 1 || iters > LSF_RESEED_MAX_ITERS)
        return fail(LSF_ERR_INVALID, "lsf_reseed_points: iters must be in 1.." + std::to_string(LSF_RESEED_MAX_ITERS));
    if (!finite_nonneg(tol)) return fail(LSF_ERR_INVALID, "lsf_reseed_points: tol must be finite and >= 0");
    // with npts == 0 pts, rad and status are ignored: they are absent here as well
    const size_t n = grid_points(nx, ny, nz), np = (size_t)npts;
    const void* a[5] = {phi, mask, np ? pts : nullptr, np ? rad : nullptr, np ? status : nullptr};
    const size_t bytes[5] = {n * sizeof(double), n * sizeof(int32_t), 3 * np * sizeof(double), np * sizeof(double), np * sizeof(int32_t)};
    const char* name[5] = {"phi", "mask", "pts", "rad", "status"};
    return overlap_ok("lsf_reseed_points", 5, a, bytes, name, 4);
}
