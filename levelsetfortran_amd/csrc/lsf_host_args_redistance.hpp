// lsf_host_args_redistance.hpp -- the argument checks of lsf_redistance_band, in the style and under the rules of lsf_host_args.hpp,
// which it is included after (its shared checks and fail() are used here): pure host code, addresses compared and never followed, the
// ORDER of the checks behaviour.  tests/host_args/redistance_args_main.cpp runs a table of argument lists through it on the CPU
// (tests/test_redistance_band_cpu.py).
#pragma once

// passes_done, changed_trace, change and info are host memory on both seams and are compared with nothing.  (The list pass and the
// foot launch on the device follow: an empty list, a non-finite phi at a list cell, no frozen cell.)
int redistance_band_args_ok(const void* phi, const void* mask, int nx, int ny, int nz, double dx, double near, int iters, double tol,
                            int max_passes, int trace_cap)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_redistance_band: phi is NULL");
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_redistance_band: mask is NULL");
    if ((rc = grid_ok("lsf_redistance_band", nx, ny, nz, 2, "more than 2^31 - 1 points (list entries are 32-bit point indices)"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_redistance_band: dx must be finite and > 0");
    if (!finite_pos(near))
        return fail(LSF_ERR_INVALID, "lsf_redistance_band: near must be finite and > 0 (the frozen cells are those whose foot lies closer than near*dx)");
    if (iters < 1) return fail(LSF_ERR_INVALID, "lsf_redistance_band: iters must be >= 1");
    if (!finite_nonneg(tol)) return fail(LSF_ERR_INVALID, "lsf_redistance_band: tol must be finite and >= 0");
    if (max_passes < 1) return fail(LSF_ERR_INVALID, "lsf_redistance_band: max_passes must be >= 1");
    if (trace_cap < 0) return fail(LSF_ERR_INVALID, "lsf_redistance_band: trace_cap must be >= 0");
    const size_t n = grid_points(nx, ny, nz);
    const void* a[2] = {mask, phi}; // (phi is written while the mask is read)
    const size_t bytes[2] = {n * sizeof(int32_t), n * sizeof(double)};
    const char* name[2] = {"mask", "phi"};
    return overlap_ok("lsf_redistance_band", 2, a, bytes, name, 1);
}
