// lsf_host_args.hpp -- what every call can decide about its arguments without the device.  Pure host code: it depends on
// include/lsf.h, <cmath>, <cstdint>, <string> and a function fail(int, const std::string&) declared before it is included, on no
// device type and on nothing else of the library.  Included by the library inside its anonymous namespace, and by
// tests/host_args/host_args_main.cpp, which runs a table of argument lists through every function here on the CPU
// (tests/test_host_args_cpu.py: return code and message of every case are recorded in tests/golden/host_args_messages.txt).
// The arrays are the caller's, host or device: their addresses are compared, never followed.  xLo and M are host arrays on both
// seams.  Nothing is written anywhere before a call's check has passed.  The ORDER of the checks of a call is behaviour: it decides
// which message a doubly wrong call gets.
#pragma once

// ---- the shared checks ---------------------------------------------------------------------------------------------------------
int check_dims(int nx, int ny, int nz)
{
    if (nx < 2 || ny < 2 || nz < 2) return fail(LSF_ERR_INVALID, "nx, ny, nz must be >= 2");
    if ((double)(nx + 1) * (ny + 1) * (nz + 1) > 9.0e9) return fail(LSF_ERR_INVALID, "field too large");
    // the Jacobi kernels address one k-plane through a buffer descriptor with 32-bit byte offsets
    if ((double)(nx + 1) * (ny + 1) * 8.0 > 2.0e9) return fail(LSF_ERR_INVALID, "a k-plane of the field exceeds 2 GB");
    return LSF_OK;
}
// Grid size of call fn.  min_ext 2: check_dims (a call that differentiates); min_ext 1: every extent >= 1 (a call that only reads
// values).  With `cap` the grid has at most 2^31 - 1 points as well (32-bit point indices), refused in the words of cap.
int grid_ok(const char* fn, int nx, int ny, int nz, int min_ext, const char* cap)
{
    if (min_ext == 2) {
        const int rc = check_dims(nx, ny, nz);
        if (rc) return rc;
    } else if (nx < 1 || ny < 1 || nz < 1)
        return fail(LSF_ERR_INVALID, std::string(fn) + ": nx, ny, nz must be >= 1");
    if (cap && ((double)nx + 1.0) * ((double)ny + 1.0) * ((double)nz + 1.0) > 2147483647.0) return fail(LSF_ERR_INVALID, std::string(fn) + ": " + cap);
    return LSF_OK;
}
bool finite_pos(double x) { return x > 0.0 && std::isfinite(x); }
bool finite_nonneg(double x) { return x >= 0.0 && std::isfinite(x); }
bool finite3(const double* x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]); }
// The arrays a[0..na) of call fn with their own byte sizes and names, the inputs first, the outputs from first_out on.  An output is
// written while the arrays before it are still being read or written: it may share a byte with none of them.  A NULL array is absent.
int overlap_ok(const char* fn, int na, const void* const* a, const size_t* bytes, const char* const* name, int first_out)
{
    for (int i = first_out; i < na; ++i)
        for (int j = 0; j < i; ++j) {
            if (!a[i] || !a[j]) continue;
            const uintptr_t x = (uintptr_t)a[i], y = (uintptr_t)a[j];
            if (x < y ? y - x < bytes[i] : x - y < bytes[j])
                return fail(LSF_ERR_INVALID, std::string(fn) + ": " + name[i] + " overlaps " + name[j]);
        }
    return LSF_OK;
}
size_t grid_points(int nx, int ny, int nz) { return ((size_t)nx + 1) * ((size_t)ny + 1) * ((size_t)nz + 1); }

// ---- one function per call -----------------------------------------------------------------------------------------------------
int mesh_args_ok(int nx, int ny, int nz, double dx, const double* xLo, double width, int flags)
{
    int rc = check_dims(nx, ny, nz);
    if (rc) return rc;
    if (!xLo) return fail(LSF_ERR_INVALID, "NULL pointer");
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "dx must be > 0");
    if (!std::isfinite(width) || width < 1.5)
        return fail(LSF_ERR_INVALID, "lsf_mesh_distance: width must be finite and >= 1.5 (the column fill needs both neighbours of a "
                                     "crossing inside the tube)");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "xLo is not finite");
    if (flags & ~LSF_MESH_UNSIGNED) return fail(LSF_ERR_INVALID, "lsf_mesh_distance: unknown flag");
    return LSF_OK;
}

// (the check pass on the device follows)
int distance_fill_args_ok(const void* phi, const void* mask, int nx, int ny, int nz, double dx, double band, int max_rounds)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "phi is NULL");
    if ((rc = grid_ok("lsf_distance_fill", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "dx must be finite and > 0");
    if (!mask && !finite_pos(band))
        return fail(LSF_ERR_INVALID, "lsf_distance_fill: without a mask, band must be finite and > 0 (the frozen set is |phi| < band*dx)");
    if (max_rounds < 1) return fail(LSF_ERR_INVALID, "lsf_distance_fill: max_rounds must be >= 1");
    return LSF_OK;
}

// (the check pass on the device follows)
int extend_field_args_ok(const void* q, const void* phi, const void* mask, int nx, int ny, int nz, double dx, double band, int max_rounds)
{
    int rc;
    if (!q) return fail(LSF_ERR_INVALID, "lsf_extend_field: q is NULL");
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_extend_field: phi is NULL");
    if ((rc = grid_ok("lsf_extend_field", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_extend_field: dx must be finite and > 0");
    if (!mask && !finite_pos(band))
        return fail(LSF_ERR_INVALID, "lsf_extend_field: without a mask, band must be finite and > 0 (the frozen set is |phi| < band*dx)");
    if (max_rounds < 1) return fail(LSF_ERR_INVALID, "lsf_extend_field: max_rounds must be >= 1");
    return LSF_OK;
}

// lsf_advect_field and lsf_advect_field_band (the scan of the inputs on the device follows)
int advect_field_args_ok(const void* phi, const void* u, const void* v, const void* w, const void* speed, int nx, int ny, int nz, double dx,
                         double dt, int steps, int scheme, int mode)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "phi is NULL");
    const int nvel = (u != nullptr) + (v != nullptr) + (w != nullptr);
    if (nvel != 0 && nvel != 3) return fail(LSF_ERR_INVALID, "lsf_advect_field: u, v, w are given together or all NULL (" + std::to_string(nvel) + " of 3 given)");
    if (!nvel && !speed) return fail(LSF_ERR_INVALID, "lsf_advect_field: neither a velocity (u, v, w) nor a speed is given");
    if ((rc = grid_ok("lsf_advect_field", nx, ny, nz, 2, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "dx must be finite and > 0");
    if (!finite_pos(dt)) return fail(LSF_ERR_INVALID, "lsf_advect_field: dt must be finite and > 0");
    if (steps < 0) return fail(LSF_ERR_INVALID, "lsf_advect_field: steps must be >= 0");
    if (scheme != LSF_ADVECT_RK3 && scheme != LSF_ADVECT_EULER) return fail(LSF_ERR_INVALID, "lsf_advect_field: unknown scheme (LSF_ADVECT_RK3 or LSF_ADVECT_EULER)");
    const int order = mode & LSF_ORDER_MASK;
    if (order == LSF_ORDER_GS)
        return fail(LSF_ERR_INVALID, "lsf_advect_field: LSF_ORDER_GS has no meaning for an explicit step (every stage reads the field as it was); "
                                     "pass LSF_ORDER_JACOBI");
    if (order != LSF_ORDER_JACOBI) return fail(LSF_ERR_INVALID, "unknown ordering");
    return LSF_OK;
}

// lsf_evolve_band (bcurv = clamp = 0) and lsf_evolve_band_curv
int evolve_band_args_ok(const void* phi, const void* mask, const void* u, const void* v, const void* w, const void* speed, int nx, int ny, int nz,
                        double dx, double dt, int steps, int scheme, int mode, double core, int ring, int reinit_sweeps, double h, int check_every,
                        double bcurv, double clamp)
{
    int rc;
    if (!finite_nonneg(bcurv)) return fail(LSF_ERR_INVALID, "lsf_evolve_band_curv: bcurv must be finite and >= 0");
    if (!finite_nonneg(clamp)) return fail(LSF_ERR_INVALID, "lsf_evolve_band_curv: clamp must be finite and >= 0 (0: no clamp)");
    // with bcurv > 0 the term moves the surface and both input groups may be absent: that check alone is answered here
    const bool none = !u && !v && !w && !speed;
    if ((rc = advect_field_args_ok(phi, u, v, w, none && bcurv > 0.0 ? phi : speed, nx, ny, nz, dx, dt, steps, scheme, mode))) return rc;
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_evolve_band: mask is NULL");
    if (!finite_pos(core)) return fail(LSF_ERR_INVALID, "lsf_evolve_band: core must be finite and > 0");
    if (ring < 1 || ring > 8) return fail(LSF_ERR_INVALID, "lsf_evolve_band: ring must be in 1..8");
    if (reinit_sweeps < 0) return fail(LSF_ERR_INVALID, "lsf_evolve_band: reinit_sweeps must be >= 0");
    if (reinit_sweeps > 0 && !finite_pos(h)) return fail(LSF_ERR_INVALID, "lsf_evolve_band: h must be finite and > 0");
    if (check_every < 1) return fail(LSF_ERR_INVALID, "lsf_evolve_band: check_every must be >= 1");
    return LSF_OK;
}

int curvature_band_args_ok(const void* phi, const void* mask, const void* kappa, const void* gauss, const void* gmag, int nx, int ny, int nz,
                           double dx, double clamp)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_curvature_band: phi is NULL");
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_curvature_band: mask is NULL");
    if (!kappa) return fail(LSF_ERR_INVALID, "lsf_curvature_band: kappa is NULL");
    if ((rc = grid_ok("lsf_curvature_band", nx, ny, nz, 2, "more than 2^31 - 1 points (list entries are 32-bit point indices)"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_curvature_band: dx must be finite and > 0");
    if (!finite_nonneg(clamp)) return fail(LSF_ERR_INVALID, "lsf_curvature_band: clamp must be finite and >= 0 (0: no clamp)");
    const size_t fb = grid_points(nx, ny, nz) * sizeof(double);
    const void* a[4] = {phi, kappa, gauss, gmag}; // (the mask is not among them)
    const size_t bytes[4] = {fb, fb, fb, fb};
    const char* name[4] = {"phi", "kappa", "gauss", "gmag"};
    return overlap_ok("lsf_curvature_band", 4, a, bytes, name, 1);
}

// (the plan pass on the device follows)
int extend_band_args_ok(const void* q, const void* phi, const void* mask, const void* known, int nx, int ny, int nz, double dx, double band,
                        int max_passes, int trace_cap)
{
    int rc;
    if (!q) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: q is NULL");
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: phi is NULL");
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: mask is NULL");
    if ((rc = grid_ok("lsf_extend_field_band", nx, ny, nz, 2, "more than 2^31 - 1 points (list entries are 32-bit point indices)"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: dx must be finite and > 0");
    if (!known && !finite_pos(band))
        return fail(LSF_ERR_INVALID, "lsf_extend_field_band: without known, band must be finite and > 0 (the frozen cells are the list cells "
                                     "with |phi| < band*dx)");
    if (max_passes < 1) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: max_passes must be >= 1");
    if (trace_cap < 0) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: trace_cap must be >= 0");
    const size_t fb = grid_points(nx, ny, nz) * sizeof(double);
    const void* a[2] = {phi, q}; // (q against phi only)
    const size_t bytes[2] = {fb, fb};
    const char* name[2] = {"phi", "q"};
    return overlap_ok("lsf_extend_field_band", 2, a, bytes, name, 1);
}

int extract_args_ok(const void* phi, int nx, int ny, int nz, double dx, const double* xLo, double iso, const int* nSurfNode, const int* nSurfElem)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "phi is NULL");
    if (!xLo || !nSurfNode || !nSurfElem) return fail(LSF_ERR_INVALID, "lsf_extract_surface: NULL xLo or count pointer");
    if ((rc = grid_ok("lsf_extract_surface", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "dx must be finite and > 0");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_extract_surface: iso must be finite");
    return LSF_OK;
}

int measure_band_args_ok(const void* phi, const void* mask, const void* q, const void* cell_area, int nx, int ny, int nz, double dx,
                         const double* xLo, double iso, const double* M)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_measure_band: phi is NULL");
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_measure_band: mask is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_measure_band: xLo is NULL");
    if (!M) return fail(LSF_ERR_INVALID, "lsf_measure_band: M is NULL");
    if ((rc = grid_ok("lsf_measure_band", nx, ny, nz, 2, "more than 2^31 - 1 points (list entries are 32-bit point indices)"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_measure_band: dx must be finite and > 0");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_measure_band: iso must be finite");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "lsf_measure_band: xLo must hold three finite values");
    const size_t n = grid_points(nx, ny, nz);
    const void* a[4] = {phi, mask, q, cell_area};
    const size_t bytes[4] = {n * sizeof(double), n * sizeof(int32_t), n * sizeof(double), n * sizeof(double)};
    const char* name[4] = {"phi", "mask", "q", "cell_area"};
    return overlap_ok("lsf_measure_band", 4, a, bytes, name, 3);
}

int sample_points_args_ok(const void* phi, const void* mask, const void* q, int nx, int ny, int nz, double dx, const double* xLo, const void* pts,
                          int npts, int order, double iso, int iters, double tol, const void* val, const void* grad, const void* qval,
                          const void* foot, const void* status)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_sample_points: phi is NULL");
    if (!pts) return fail(LSF_ERR_INVALID, "lsf_sample_points: pts is NULL");
    if (!val) return fail(LSF_ERR_INVALID, "lsf_sample_points: val is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_sample_points: xLo is NULL");
    if (npts < 1) return fail(LSF_ERR_INVALID, "lsf_sample_points: npts must be >= 1");
    if ((rc = grid_ok("lsf_sample_points", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_sample_points: dx must be finite and > 0");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "lsf_sample_points: xLo must hold three finite values");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_sample_points: iso must be finite");
    if (order != LSF_SAMPLE_LINEAR && order != LSF_SAMPLE_CUBIC) return fail(LSF_ERR_INVALID, "lsf_sample_points: unknown order");
    if (iters < 0) return fail(LSF_ERR_INVALID, "lsf_sample_points: iters must be >= 0");
    if (iters >= 1 && !finite_nonneg(tol)) return fail(LSF_ERR_INVALID, "lsf_sample_points: tol must be finite and >= 0");
    if (qval && !q) return fail(LSF_ERR_INVALID, "lsf_sample_points: qval without q");
    if (foot && iters == 0) return fail(LSF_ERR_INVALID, "lsf_sample_points: foot with iters == 0");
    const size_t n = grid_points(nx, ny, nz), np = (size_t)npts;
    const void* a[9] = {phi, mask, q, pts, val, grad, qval, foot, status};
    const size_t bytes[9] = {n * sizeof(double),      n * sizeof(int32_t), n * sizeof(double),      3 * np * sizeof(double), np * sizeof(double),
                             3 * np * sizeof(double), np * sizeof(double), 3 * np * sizeof(double), np * sizeof(int32_t)};
    const char* name[9] = {"phi", "mask", "q", "pts", "val", "grad", "qval", "foot", "status"};
    return overlap_ok("lsf_sample_points", 9, a, bytes, name, 4);
}

int cast_rays_args_ok(const void* phi, const void* mask, const void* q, int nx, int ny, int nz, double dx, const double* xLo, const void* org,
                      const void* dir, int nrays, int order, double iso, double tmin, double tmax, double safety, double smin, double smax, double skip,
                      int refine, int max_steps, const void* thit, const void* hit, const void* grad, const void* qval, const void* status)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_cast_rays: phi is NULL");
    if (!org) return fail(LSF_ERR_INVALID, "lsf_cast_rays: org is NULL");
    if (!dir) return fail(LSF_ERR_INVALID, "lsf_cast_rays: dir is NULL");
    if (!thit) return fail(LSF_ERR_INVALID, "lsf_cast_rays: thit is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_cast_rays: xLo is NULL");
    if (nrays < 1) return fail(LSF_ERR_INVALID, "lsf_cast_rays: nrays must be >= 1");
    if ((rc = grid_ok("lsf_cast_rays", nx, ny, nz, 1, "more than 2^31 - 1 points"))) return rc;
    if (!finite_pos(dx)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: dx must be finite and > 0");
    if (!finite3(xLo)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: xLo must hold three finite values");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: iso must be finite");
    if (order != LSF_SAMPLE_LINEAR && order != LSF_SAMPLE_CUBIC) return fail(LSF_ERR_INVALID, "lsf_cast_rays: unknown order");
    if (!finite_nonneg(tmin)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: tmin must be finite and >= 0");
    if (!(tmax > tmin) || !std::isfinite(tmax)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: tmax must be finite and > tmin");
    if (!(safety > 0.0 && safety <= 1.0)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: safety must lie in (0, 1]");
    if (!finite_pos(smin)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: smin must be finite and > 0");
    if (!(smax >= smin) || !std::isfinite(smax)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: smax must be finite and >= smin");
    if (!finite_pos(skip)) return fail(LSF_ERR_INVALID, "lsf_cast_rays: skip must be finite and > 0");
    if (refine < 0) return fail(LSF_ERR_INVALID, "lsf_cast_rays: refine must be >= 0");
    if (max_steps < 1) return fail(LSF_ERR_INVALID, "lsf_cast_rays: max_steps must be >= 1");
    if (qval && !q) return fail(LSF_ERR_INVALID, "lsf_cast_rays: qval without q");
    const size_t n = grid_points(nx, ny, nz), nr = (size_t)nrays;
    const void* a[10] = {phi, mask, q, org, dir, thit, hit, grad, qval, status};
    const size_t bytes[10] = {n * sizeof(double),       n * sizeof(int32_t),  n * sizeof(double),       3 * nr * sizeof(double), 3 * nr * sizeof(double),
                              nr * sizeof(double),      3 * nr * sizeof(double), 3 * nr * sizeof(double), nr * sizeof(double),     nr * sizeof(int32_t)};
    const char* name[10] = {"phi", "mask", "q", "org", "dir", "thit", "hit", "grad", "qval", "status"};
    return overlap_ok("lsf_cast_rays", 10, a, bytes, name, 5);
}

// (the check launch on the device follows)
int label_band_args_ok(const void* phi, const void* mask, const void* label, int nx, int ny, int nz, double iso, int side, int max_passes,
                       const void* comp, int comp_cap)
{
    int rc;
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_label_band: phi is NULL");
    if (!mask) return fail(LSF_ERR_INVALID, "lsf_label_band: mask is NULL");
    if (!label) return fail(LSF_ERR_INVALID, "lsf_label_band: label is NULL");
    if ((rc = grid_ok("lsf_label_band", nx, ny, nz, 2, "more than 2^31 - 1 points (list entries and labels are 32-bit point indices)"))) return rc;
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_label_band: iso must be finite");
    if (side != LSF_LABEL_INSIDE && side != LSF_LABEL_OUTSIDE && side != LSF_LABEL_BOTH)
        return fail(LSF_ERR_INVALID, "lsf_label_band: side must be LSF_LABEL_INSIDE, LSF_LABEL_OUTSIDE or LSF_LABEL_BOTH");
    if (max_passes < 1) return fail(LSF_ERR_INVALID, "lsf_label_band: max_passes must be >= 1");
    if (comp_cap < 0) return fail(LSF_ERR_INVALID, "lsf_label_band: comp_cap must be >= 0");
    if (!comp && comp_cap > 0) return fail(LSF_ERR_INVALID, "lsf_label_band: comp is NULL with comp_cap > 0");
    const size_t n = grid_points(nx, ny, nz);
    const void* a[3] = {phi, mask, label};
    const size_t bytes[3] = {n * sizeof(double), n * sizeof(int32_t), n * sizeof(int32_t)};
    const char* name[3] = {"phi", "mask", "label"};
    return overlap_ok("lsf_label_band", 3, a, bytes, name, 2);
}
