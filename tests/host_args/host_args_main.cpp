// host_args_main.cpp -- runs a table of argument lists through check_dims and every *_args_ok of
// levelsetfortran_amd/csrc/lsf_host_args.hpp on the CPU and prints one line per case:  name | return code | message
// (the message is what lsf_last_error() would hold; empty on LSF_OK).  tests/test_host_args_cpu.py compares the output with
// tests/golden/host_args_messages.txt, which tests/golden/make_host_args_messages.py recorded from the functions as they were
// before they were rewritten over shared checks.  The functions never follow an array pointer, so the arrays are made-up
// addresses; xLo alone is read and is a real array.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/lsf.h"

namespace {
std::string g_err;
int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
#include "../../levelsetfortran_amd/csrc/lsf_host_args.hpp"

void show(const std::string& name, int rc)
{
    std::printf("%s | %d | %s\n", name.c_str(), rc, rc == LSF_OK ? "" : g_err.c_str());
    g_err.clear();
}

const void* at(uintptr_t a) { return (const void*)a; }
// arrays far apart from each other and from address 0
const void *const PHI = at(0x100000000000), *const MASK = at(0x200000000000), *const Q = at(0x300000000000);
const void *const A4 = at(0x400000000000), *const A5 = at(0x500000000000), *const A6 = at(0x600000000000), *const A7 = at(0x700000000000);
const void *const A8 = at(0x800000000000), *const A9 = at(0x900000000000), *const A10 = at(0xa00000000000);
const double XLO[3] = {-1.0, 0.25, 3.0};
const double XLO_NAN[3] = {0.0, NAN, 0.0}, XLO_INF[3] = {0.0, 0.0, -INFINITY}, XLO_INF0[3] = {INFINITY, 0.0, 0.0};
const int COUNT = 0; // a count pointer's target (never read)

// the argument list of each function with values that pass; a case changes one or two of them
struct Dims { int nx = 2, ny = 2, nz = 2; };
struct Mesh : Dims { double dx = 0.5; const double* xLo = XLO; double width = 3.0; int flags = 0; };
struct Fill : Dims { const void *phi = PHI, *mask = MASK; double dx = 0.5, band = 3.0; int max_rounds = 4; };
struct Ext : Dims { const void *q = Q, *phi = PHI, *mask = MASK; double dx = 0.5, band = 3.0; int max_rounds = 4; };
struct Adv : Dims { const void *phi = PHI, *u = A4, *v = A5, *w = A6, *speed = A7; double dx = 0.5, dt = 0.1; int steps = 3, scheme = LSF_ADVECT_RK3, mode = LSF_ORDER_JACOBI; };
struct Evo : Adv { const void* mask = MASK; double core = 3.0; int ring = 2, reinit_sweeps = 2; double h = 0.1; int check_every = 4; double bcurv = 0.0, clamp = 0.0; };
struct Curv : Dims { const void *phi = PHI, *mask = MASK, *kappa = A4, *gauss = A5, *gmag = A6; double dx = 0.5, clamp = 0.0; };
struct Xb : Dims { const void *q = Q, *phi = PHI, *mask = MASK, *known = A4; double dx = 0.5, band = 3.0; int max_passes = 4, trace_cap = 0; };
struct Surf : Dims { const void* phi = PHI; double dx = 0.5; const double* xLo = XLO; double iso = 0.0; const int *nn = &COUNT, *ne = &COUNT; };
struct Meas : Dims { const void *phi = PHI, *mask = MASK, *q = Q, *cell = A4; double dx = 0.5; const double* xLo = XLO; double iso = 0.0; const double* M = XLO; };
struct Samp : Dims { const void *phi = PHI, *mask = MASK, *q = Q; double dx = 0.5; const double* xLo = XLO; const void* pts = A4; int npts = 5, order = LSF_SAMPLE_CUBIC; double iso = 0.0; int iters = 2; double tol = 1e-9; const void *val = A5, *grad = A6, *qval = A7, *foot = A8, *status = A9; };
struct Cast : Dims { const void *phi = PHI, *mask = MASK, *q = Q; double dx = 0.5; const double* xLo = XLO; const void *org = A4, *dir = A5; int nrays = 5, order = LSF_SAMPLE_CUBIC; double iso = 0.0, tmin = 0.0, tmax = 10.0, safety = 0.9, smin = 0.01, smax = 1.0, skip = 1.0; int refine = 2, max_steps = 100; const void *thit = A6, *hit = A7, *grad = A8, *qval = A9, *status = A10; };
struct Lab : Dims { const void *phi = PHI, *mask = MASK, *label = A4; double iso = 0.0; int side = LSF_LABEL_BOTH, max_passes = 4; const void* comp = A5; int comp_cap = 8; };

int call(const Dims& a) { return check_dims(a.nx, a.ny, a.nz); }
int call(const Mesh& a) { return mesh_args_ok(a.nx, a.ny, a.nz, a.dx, a.xLo, a.width, a.flags); }
int call(const Fill& a) { return distance_fill_args_ok(a.phi, a.mask, a.nx, a.ny, a.nz, a.dx, a.band, a.max_rounds); }
int call(const Ext& a) { return extend_field_args_ok(a.q, a.phi, a.mask, a.nx, a.ny, a.nz, a.dx, a.band, a.max_rounds); }
int call(const Adv& a) { return advect_field_args_ok(a.phi, a.u, a.v, a.w, a.speed, a.nx, a.ny, a.nz, a.dx, a.dt, a.steps, a.scheme, a.mode); }
int call(const Evo& a)
{
    return evolve_band_args_ok(a.phi, a.mask, a.u, a.v, a.w, a.speed, a.nx, a.ny, a.nz, a.dx, a.dt, a.steps, a.scheme, a.mode, a.core, a.ring,
                               a.reinit_sweeps, a.h, a.check_every, a.bcurv, a.clamp);
}
int call(const Curv& a) { return curvature_band_args_ok(a.phi, a.mask, a.kappa, a.gauss, a.gmag, a.nx, a.ny, a.nz, a.dx, a.clamp); }
int call(const Xb& a) { return extend_band_args_ok(a.q, a.phi, a.mask, a.known, a.nx, a.ny, a.nz, a.dx, a.band, a.max_passes, a.trace_cap); }
int call(const Surf& a) { return extract_args_ok(a.phi, a.nx, a.ny, a.nz, a.dx, a.xLo, a.iso, a.nn, a.ne); }
int call(const Meas& a) { return measure_band_args_ok(a.phi, a.mask, a.q, a.cell, a.nx, a.ny, a.nz, a.dx, a.xLo, a.iso, a.M); }
int call(const Samp& a)
{
    return sample_points_args_ok(a.phi, a.mask, a.q, a.nx, a.ny, a.nz, a.dx, a.xLo, a.pts, a.npts, a.order, a.iso, a.iters, a.tol, a.val, a.grad,
                                 a.qval, a.foot, a.status);
}
int call(const Cast& a)
{
    return cast_rays_args_ok(a.phi, a.mask, a.q, a.nx, a.ny, a.nz, a.dx, a.xLo, a.org, a.dir, a.nrays, a.order, a.iso, a.tmin, a.tmax, a.safety,
                             a.smin, a.smax, a.skip, a.refine, a.max_steps, a.thit, a.hit, a.grad, a.qval, a.status);
}
int call(const Lab& a) { return label_band_args_ok(a.phi, a.mask, a.label, a.nx, a.ny, a.nz, a.iso, a.side, a.max_passes, a.comp, a.comp_cap); }

// one case: the passing list of T with the given assignments applied; the assignments are its name
#define CASE(T, ...)                \
    {                               \
        T a;                        \
        __VA_ARGS__;                \
        show(#T ": " #__VA_ARGS__, call(a)); \
    }
// the grid cases of one call: the smallest grid it takes and one below on each axis, the largest it takes, 2^31 points, and what
// check_dims alone refuses
#define GRID_CASES(T)                                 \
    CASE(T, a.nx = a.ny = a.nz = 1)                   \
    CASE(T, a.nx = a.ny = a.nz = 2)                   \
    CASE(T, a.nx = 0, a.ny = a.nz = 1)                \
    CASE(T, a.ny = 0, a.nx = a.nz = 1)                \
    CASE(T, a.nz = 0, a.nx = a.ny = 1)                \
    CASE(T, a.nx = 1)                                 \
    CASE(T, a.ny = 1)                                 \
    CASE(T, a.nz = 1)                                 \
    CASE(T, a.nx = -5)                                \
    CASE(T, a.nx = a.ny = 2047, a.nz = 510)           \
    CASE(T, a.nx = a.ny = 2047, a.nz = 511)           \
    CASE(T, a.nx = 511, a.ny = a.nz = 2047)           \
    CASE(T, a.nx = a.ny = a.nz = 2099)                \
    CASE(T, a.nx = a.ny = 15999)
// a scalar that must be finite and > 0 (or >= 0: then the 0.0 case passes)
#define SCALAR_CASES(T, F) \
    CASE(T, a.F = 0.0)     \
    CASE(T, a.F = -1.0)    \
    CASE(T, a.F = NAN)     \
    CASE(T, a.F = INFINITY) \
    CASE(T, a.F = -INFINITY)
#define XLO_CASES(T)         \
    CASE(T, a.xLo = nullptr) \
    CASE(T, a.xLo = XLO_NAN) \
    CASE(T, a.xLo = XLO_INF) \
    CASE(T, a.xLo = XLO_INF0)

// The overlap cases of one call.  f builds the call's argument list from the na arrays p[0..na), array k having bytes[k] bytes; the
// inputs come first, the outputs from first_out on, and every array begins far from the others and from address 0.  For every output i
// and every array j before it: i begins exactly at the end of j (no shared byte), begins one byte before the end of j, ends exactly at
// the beginning of j, and ends one byte into j.  A pair that the call does not test passes all four.  Then every optional array in turn
// is NULL while the first output (or, when that is the NULL one, phi) lies at address 8: a NULL array is no array at address 0.
template <class F>
void overlap_cases(const std::string& fn, int na, const char* const* name, const size_t* bytes, const bool* optional, int first_out, F f)
{
    const void* p[10];
    auto far_apart = [&] {
        for (int k = 0; k < na; ++k) p[k] = at((uintptr_t)(k + 1) * 0x100000000000);
    };
    for (int i = first_out; i < na; ++i)
        for (int j = 0; j < i; ++j) {
            far_apart();
            const uintptr_t y = (uintptr_t)p[j];
            const struct { const char* what; uintptr_t x; } put[4] = {{" begins at the end of ", y + bytes[j]},
                                                                      {" begins one byte before the end of ", y + bytes[j] - 1},
                                                                      {" ends at the beginning of ", y - bytes[i]},
                                                                      {" ends one byte into ", y - bytes[i] + 1}};
            for (const auto& c : put) {
                p[i] = at(c.x);
                show(fn + ": " + name[i] + c.what + name[j], f(p));
            }
        }
    for (int k = 0; k < na; ++k) {
        if (!optional[k]) continue;
        far_apart();
        const int low = k == first_out ? 0 : first_out;
        p[k] = nullptr, p[low] = at(8);
        show(fn + ": " + name[k] + " NULL, " + name[low] + " at address 8", f(p));
    }
}
} // namespace

int main()
{
    // ---- check_dims (lsf_reinit, lsf_minmax, lsf_narrowband, lsf_phi0, ... call it alone)
    GRID_CASES(Dims)

    // ---- lsf_mesh_distance
    CASE(Mesh, (void)a)
    GRID_CASES(Mesh)
    XLO_CASES(Mesh)
    SCALAR_CASES(Mesh, dx)
    SCALAR_CASES(Mesh, width)
    CASE(Mesh, a.width = 1.5)
    CASE(Mesh, a.width = 1.4999)
    CASE(Mesh, a.flags = LSF_MESH_UNSIGNED)
    CASE(Mesh, a.flags = 2)
    CASE(Mesh, a.flags = -1)
    CASE(Mesh, a.nx = 1, a.xLo = nullptr, a.dx = NAN)
    CASE(Mesh, a.dx = NAN, a.width = NAN, a.xLo = XLO_NAN, a.flags = 2)

    // ---- lsf_distance_fill
    CASE(Fill, (void)a)
    CASE(Fill, a.phi = nullptr)
    CASE(Fill, a.phi = nullptr, a.nx = 0)
    GRID_CASES(Fill)
    SCALAR_CASES(Fill, dx)
    SCALAR_CASES(Fill, band)
    CASE(Fill, a.mask = nullptr)
    CASE(Fill, a.mask = nullptr, a.band = 0.0)
    CASE(Fill, a.mask = nullptr, a.band = NAN)
    CASE(Fill, a.mask = nullptr, a.band = INFINITY)
    CASE(Fill, a.max_rounds = 1)
    CASE(Fill, a.max_rounds = 0)
    CASE(Fill, a.dx = 0.0, a.max_rounds = 0)

    // ---- lsf_extend_field
    CASE(Ext, (void)a)
    CASE(Ext, a.q = nullptr)
    CASE(Ext, a.phi = nullptr)
    CASE(Ext, a.q = nullptr, a.phi = nullptr)
    CASE(Ext, a.q = a.phi)
    GRID_CASES(Ext)
    SCALAR_CASES(Ext, dx)
    SCALAR_CASES(Ext, band)
    CASE(Ext, a.mask = nullptr)
    CASE(Ext, a.mask = nullptr, a.band = 0.0)
    CASE(Ext, a.mask = nullptr, a.band = NAN)
    CASE(Ext, a.mask = nullptr, a.band = INFINITY)
    CASE(Ext, a.max_rounds = 1)
    CASE(Ext, a.max_rounds = 0)

    // ---- lsf_advect_field, lsf_advect_field_band
    CASE(Adv, (void)a)
    CASE(Adv, a.phi = nullptr)
    CASE(Adv, a.u = nullptr)
    CASE(Adv, a.v = a.w = nullptr)
    CASE(Adv, a.u = a.v = a.w = nullptr)
    CASE(Adv, a.speed = nullptr)
    CASE(Adv, a.u = a.v = a.w = a.speed = nullptr)
    CASE(Adv, a.u = a.speed = nullptr, a.nx = 0)
    GRID_CASES(Adv)
    SCALAR_CASES(Adv, dx)
    SCALAR_CASES(Adv, dt)
    CASE(Adv, a.steps = 0)
    CASE(Adv, a.steps = -1)
    CASE(Adv, a.scheme = LSF_ADVECT_EULER)
    CASE(Adv, a.scheme = 2)
    CASE(Adv, a.scheme = -1)
    CASE(Adv, a.mode = LSF_ORDER_GS)
    CASE(Adv, a.mode = LSF_ORDER_GS | LSF_ARITH_STRICT)
    CASE(Adv, a.mode = LSF_ORDER_JACOBI | LSF_ARITH_STRICT)
    CASE(Adv, a.mode = 2)
    CASE(Adv, a.dt = 0.0, a.steps = -1, a.scheme = 2, a.mode = 2)

    // ---- lsf_evolve_band, lsf_evolve_band_curv
    CASE(Evo, (void)a)
    SCALAR_CASES(Evo, bcurv)
    SCALAR_CASES(Evo, clamp)
    CASE(Evo, a.bcurv = 0.5, a.clamp = 2.0)
    CASE(Evo, a.u = a.v = a.w = a.speed = nullptr)
    CASE(Evo, a.u = a.v = a.w = a.speed = nullptr, a.bcurv = 0.5)
    CASE(Evo, a.u = a.speed = nullptr, a.bcurv = 0.5)
    CASE(Evo, a.phi = nullptr, a.bcurv = 0.5)
    CASE(Evo, a.phi = nullptr, a.bcurv = NAN)
    CASE(Evo, a.mask = nullptr)
    CASE(Evo, a.mask = nullptr, a.nx = 1)
    GRID_CASES(Evo)
    SCALAR_CASES(Evo, dx)
    SCALAR_CASES(Evo, dt)
    SCALAR_CASES(Evo, core)
    CASE(Evo, a.ring = 1)
    CASE(Evo, a.ring = 8)
    CASE(Evo, a.ring = 0)
    CASE(Evo, a.ring = 9)
    CASE(Evo, a.reinit_sweeps = -1)
    CASE(Evo, a.reinit_sweeps = 0, a.h = NAN)
    SCALAR_CASES(Evo, h)
    CASE(Evo, a.check_every = 1)
    CASE(Evo, a.check_every = 0)
    CASE(Evo, a.mode = LSF_ORDER_GS, a.core = 0.0)

    // ---- lsf_curvature_band
    CASE(Curv, (void)a)
    CASE(Curv, a.phi = nullptr)
    CASE(Curv, a.mask = nullptr)
    CASE(Curv, a.kappa = nullptr)
    CASE(Curv, a.phi = a.mask = a.kappa = nullptr)
    CASE(Curv, a.gauss = a.gmag = nullptr)
    CASE(Curv, a.kappa = nullptr, a.nx = 1)
    GRID_CASES(Curv)
    SCALAR_CASES(Curv, dx)
    SCALAR_CASES(Curv, clamp)
    CASE(Curv, a.kappa = a.phi)
    CASE(Curv, a.gauss = a.kappa, a.gmag = a.phi)
    CASE(Curv, a.kappa = a.mask)
    CASE(Curv, a.kappa = a.phi, a.dx = 0.0)
    {
        const char* name[5] = {"phi", "mask", "kappa", "gauss", "gmag"};
        const size_t bytes[5] = {27 * 8, 27 * 4, 27 * 8, 27 * 8, 27 * 8};
        const bool optional[5] = {false, false, false, true, true};
        overlap_cases("Curv", 5, name, bytes, optional, 2, [](const void* const* p) {
            Curv a;
            a.phi = p[0], a.mask = p[1], a.kappa = p[2], a.gauss = p[3], a.gmag = p[4];
            return call(a);
        });
    }

    // ---- lsf_extend_field_band
    CASE(Xb, (void)a)
    CASE(Xb, a.q = nullptr)
    CASE(Xb, a.phi = nullptr)
    CASE(Xb, a.mask = nullptr)
    CASE(Xb, a.q = a.phi = a.mask = nullptr)
    CASE(Xb, a.mask = nullptr, a.nx = 1)
    GRID_CASES(Xb)
    SCALAR_CASES(Xb, dx)
    SCALAR_CASES(Xb, band)
    CASE(Xb, a.known = nullptr)
    CASE(Xb, a.known = nullptr, a.band = 0.0)
    CASE(Xb, a.known = nullptr, a.band = NAN)
    CASE(Xb, a.known = nullptr, a.band = INFINITY)
    CASE(Xb, a.max_passes = 1)
    CASE(Xb, a.max_passes = 0)
    CASE(Xb, a.trace_cap = -1)
    CASE(Xb, a.trace_cap = 7)
    CASE(Xb, a.q = a.phi)
    CASE(Xb, a.q = a.mask)
    CASE(Xb, a.q = a.known)
    CASE(Xb, a.q = a.phi, a.trace_cap = -1)
    {
        const char* name[4] = {"phi", "mask", "known", "q"};
        const size_t bytes[4] = {27 * 8, 27 * 4, 27 * 4, 27 * 8};
        const bool optional[4] = {false, false, true, false};
        overlap_cases("Xb", 4, name, bytes, optional, 3, [](const void* const* p) {
            Xb a;
            a.phi = p[0], a.mask = p[1], a.known = p[2], a.q = p[3];
            return call(a);
        });
    }

    // ---- lsf_extract_surface
    CASE(Surf, (void)a)
    CASE(Surf, a.phi = nullptr)
    CASE(Surf, a.xLo = nullptr)
    CASE(Surf, a.nn = nullptr)
    CASE(Surf, a.ne = nullptr)
    CASE(Surf, a.phi = nullptr, a.xLo = nullptr)
    CASE(Surf, a.xLo = XLO_NAN)
    GRID_CASES(Surf)
    SCALAR_CASES(Surf, dx)
    CASE(Surf, a.iso = 0.25)
    CASE(Surf, a.iso = NAN)
    CASE(Surf, a.iso = INFINITY)
    CASE(Surf, a.dx = 0.0, a.iso = NAN)

    // ---- lsf_measure_band
    CASE(Meas, (void)a)
    CASE(Meas, a.phi = nullptr)
    CASE(Meas, a.mask = nullptr)
    CASE(Meas, a.M = nullptr)
    CASE(Meas, a.phi = a.mask = nullptr, a.xLo = a.M = nullptr)
    CASE(Meas, a.q = a.cell = nullptr)
    CASE(Meas, a.M = nullptr, a.nx = 1)
    XLO_CASES(Meas)
    GRID_CASES(Meas)
    SCALAR_CASES(Meas, dx)
    CASE(Meas, a.iso = 0.25)
    CASE(Meas, a.iso = NAN)
    CASE(Meas, a.iso = -INFINITY)
    CASE(Meas, a.iso = NAN, a.xLo = XLO_NAN)
    CASE(Meas, a.cell = a.phi)
    CASE(Meas, a.cell = a.mask)
    CASE(Meas, a.cell = a.q)
    CASE(Meas, a.q = a.phi)
    CASE(Meas, a.cell = a.phi, a.xLo = XLO_INF)
    {
        const char* name[4] = {"phi", "mask", "q", "cell_area"};
        const size_t bytes[4] = {27 * 8, 27 * 4, 27 * 8, 27 * 8};
        const bool optional[4] = {false, false, true, true};
        overlap_cases("Meas", 4, name, bytes, optional, 3, [](const void* const* p) {
            Meas a;
            a.phi = p[0], a.mask = p[1], a.q = p[2], a.cell = p[3];
            return call(a);
        });
    }

    // ---- lsf_sample_points
    CASE(Samp, (void)a)
    CASE(Samp, a.phi = nullptr)
    CASE(Samp, a.pts = nullptr)
    CASE(Samp, a.val = nullptr)
    CASE(Samp, a.phi = a.pts = a.val = nullptr, a.xLo = nullptr)
    CASE(Samp, a.mask = a.q = a.grad = a.qval = a.foot = a.status = nullptr)
    XLO_CASES(Samp)
    CASE(Samp, a.npts = 1)
    CASE(Samp, a.npts = 0)
    CASE(Samp, a.npts = 0, a.nx = 0)
    GRID_CASES(Samp)
    SCALAR_CASES(Samp, dx)
    CASE(Samp, a.dx = NAN, a.xLo = XLO_NAN, a.iso = NAN)
    CASE(Samp, a.iso = NAN)
    CASE(Samp, a.iso = INFINITY)
    CASE(Samp, a.order = LSF_SAMPLE_LINEAR)
    CASE(Samp, a.order = 2)
    CASE(Samp, a.order = -1)
    CASE(Samp, a.iters = -1)
    CASE(Samp, a.iters = 1, a.tol = 0.0)
    SCALAR_CASES(Samp, tol)
    CASE(Samp, a.iters = 0, a.foot = nullptr, a.tol = NAN)
    CASE(Samp, a.iters = 0)
    CASE(Samp, a.q = nullptr)
    CASE(Samp, a.q = a.qval = nullptr)
    CASE(Samp, a.q = nullptr, a.iters = 0)
    CASE(Samp, a.val = a.pts)
    CASE(Samp, a.grad = a.val, a.status = a.phi)
    CASE(Samp, a.pts = a.phi)
    {
        const char* name[9] = {"phi", "mask", "q", "pts", "val", "grad", "qval", "foot", "status"};
        const size_t bytes[9] = {27 * 8, 27 * 4, 27 * 8, 3 * 5 * 8, 5 * 8, 3 * 5 * 8, 5 * 8, 3 * 5 * 8, 5 * 4};
        const bool optional[9] = {false, true, true, false, false, true, true, true, true};
        overlap_cases("Samp", 9, name, bytes, optional, 4, [](const void* const* p) {
            Samp a;
            a.phi = p[0], a.mask = p[1], a.q = p[2], a.pts = p[3], a.val = p[4], a.grad = p[5], a.foot = p[7], a.status = p[8];
            a.qval = p[2] ? p[6] : nullptr; // (qval goes with q)
            return call(a);
        });
    }

    // ---- lsf_cast_rays
    CASE(Cast, (void)a)
    CASE(Cast, a.phi = nullptr)
    CASE(Cast, a.org = nullptr)
    CASE(Cast, a.dir = nullptr)
    CASE(Cast, a.thit = nullptr)
    CASE(Cast, a.phi = a.org = a.dir = a.thit = nullptr, a.xLo = nullptr)
    CASE(Cast, a.mask = a.q = a.hit = a.grad = a.qval = a.status = nullptr)
    XLO_CASES(Cast)
    CASE(Cast, a.nrays = 1)
    CASE(Cast, a.nrays = 0)
    CASE(Cast, a.nrays = 0, a.nx = 0)
    GRID_CASES(Cast)
    SCALAR_CASES(Cast, dx)
    CASE(Cast, a.dx = NAN, a.xLo = XLO_NAN, a.iso = NAN)
    CASE(Cast, a.iso = NAN)
    CASE(Cast, a.iso = -INFINITY)
    CASE(Cast, a.order = LSF_SAMPLE_LINEAR)
    CASE(Cast, a.order = 2)
    SCALAR_CASES(Cast, tmin)
    CASE(Cast, a.tmin = 10.0)
    CASE(Cast, a.tmin = 11.0)
    CASE(Cast, a.tmax = NAN)
    CASE(Cast, a.tmax = INFINITY)
    CASE(Cast, a.tmax = 0.0)
    SCALAR_CASES(Cast, safety)
    CASE(Cast, a.safety = 1.0)
    CASE(Cast, a.safety = 1.0000001)
    SCALAR_CASES(Cast, smin)
    CASE(Cast, a.smin = 1.0)
    CASE(Cast, a.smin = 1.5)
    CASE(Cast, a.smax = NAN)
    CASE(Cast, a.smax = INFINITY)
    CASE(Cast, a.smax = 0.001)
    SCALAR_CASES(Cast, skip)
    CASE(Cast, a.refine = 0)
    CASE(Cast, a.refine = -1)
    CASE(Cast, a.max_steps = 1)
    CASE(Cast, a.max_steps = 0)
    CASE(Cast, a.q = nullptr)
    CASE(Cast, a.q = a.qval = nullptr)
    CASE(Cast, a.q = nullptr, a.max_steps = 0)
    CASE(Cast, a.thit = a.dir)
    CASE(Cast, a.hit = a.thit, a.status = a.phi)
    CASE(Cast, a.dir = a.org)
    {
        const char* name[10] = {"phi", "mask", "q", "org", "dir", "thit", "hit", "grad", "qval", "status"};
        const size_t bytes[10] = {27 * 8, 27 * 4, 27 * 8, 3 * 5 * 8, 3 * 5 * 8, 5 * 8, 3 * 5 * 8, 3 * 5 * 8, 5 * 8, 5 * 4};
        const bool optional[10] = {false, true, true, false, false, false, true, true, true, true};
        overlap_cases("Cast", 10, name, bytes, optional, 5, [](const void* const* p) {
            Cast a;
            a.phi = p[0], a.mask = p[1], a.q = p[2], a.org = p[3], a.dir = p[4], a.thit = p[5], a.hit = p[6], a.grad = p[7], a.status = p[9];
            a.qval = p[2] ? p[8] : nullptr; // (qval goes with q)
            return call(a);
        });
    }

    // ---- lsf_label_band
    CASE(Lab, (void)a)
    CASE(Lab, a.phi = nullptr)
    CASE(Lab, a.mask = nullptr)
    CASE(Lab, a.label = nullptr)
    CASE(Lab, a.phi = a.mask = a.label = nullptr)
    CASE(Lab, a.label = nullptr, a.nx = 1)
    GRID_CASES(Lab)
    CASE(Lab, a.iso = 0.25)
    CASE(Lab, a.iso = NAN)
    CASE(Lab, a.iso = INFINITY)
    CASE(Lab, a.side = LSF_LABEL_INSIDE)
    CASE(Lab, a.side = LSF_LABEL_OUTSIDE)
    CASE(Lab, a.side = 3)
    CASE(Lab, a.side = -1)
    CASE(Lab, a.max_passes = 1)
    CASE(Lab, a.max_passes = 0)
    CASE(Lab, a.comp_cap = 0)
    CASE(Lab, a.comp_cap = -1)
    CASE(Lab, a.comp = nullptr)
    CASE(Lab, a.comp = nullptr, a.comp_cap = 0)
    CASE(Lab, a.comp = nullptr, a.comp_cap = -1)
    CASE(Lab, a.label = a.phi)
    CASE(Lab, a.label = a.mask)
    CASE(Lab, a.label = a.comp)
    CASE(Lab, a.label = a.phi, a.iso = NAN)
    {
        const char* name[3] = {"phi", "mask", "label"};
        const size_t bytes[3] = {27 * 8, 27 * 4, 27 * 4};
        const bool optional[3] = {false, false, false};
        overlap_cases("Lab", 3, name, bytes, optional, 2, [](const void* const* p) {
            Lab a;
            a.phi = p[0], a.mask = p[1], a.label = p[2];
            return call(a);
        });
    }
    return 0;
}
