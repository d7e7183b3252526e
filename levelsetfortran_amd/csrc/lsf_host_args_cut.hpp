// lsf_host_args_cut.hpp -- the argument checks of lsf_cut_cells_band, in the style and under the rules of lsf_host_args.hpp, which it
// is included after (its shared checks and fail() are used here): pure host code, addresses compared and never followed, the ORDER
// of the checks behaviour.  tests/host_args/cut_cells_args_main.cpp runs a table of argument lists through it on the CPU
// (tests/test_host_cut_args_cpu.py).
#pragma once

// volume and vof_min are host scalars on both seams and are compared with nothing
int cut_cells_args_ok(const void* phi, const void* mask, int nx, int ny, int nz, double dx, double iso, const void* vof, const void* ax,
                      const void* ay, const void* az, const void* bx, const void* by, const void* bz, const void* volume)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: phi is NULL");
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: mask is NULL");
    if ((rc = grid_ok("lsf_cut_cells_band", nx, ny, nz, 2, "more than 2^31 - 1 points (list entries are 32-bit point indices)"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: dx must be finite and > 0");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: iso must be finite");
    const int na = (ax != nullptr) + (ay != nullptr) + (az != nullptr), nb = (bx != nullptr) + (by != nullptr) + (bz != nullptr);
    if (na != 0 && na != 3)
        return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: ax, ay, az are given together or all NULL (" + std::to_string(na) + " of 3 given)");
    if (nb != 0 && nb != 3)
        return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: bx, by, bz are given together or all NULL (" + std::to_string(nb) + " of 3 given)");
    if (!vof && !na && !nb && !volume)
        return fail(LSF_ERR_INVALID, "lsf_cut_cells_band: nothing is requested (vof, the apertures, the area vector and volume are all NULL)");
    const size_t n = grid_points(nx, ny, nz), fb = n * sizeof(double);
    const void* a[9] = {phi, mask, vof, ax, ay, az, bx, by, bz};
    const size_t bytes[9] = {fb, n * sizeof(int32_t), fb, fb, fb, fb, fb, fb, fb};
    const char* name[9] = {"phi", "mask", "vof", "ax", "ay", "az", "bx", "by", "bz"};
    return overlap_ok("lsf_cut_cells_band", 9, a, bytes, name, 2);
}
