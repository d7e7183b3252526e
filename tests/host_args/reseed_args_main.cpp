// reseed_args_main.cpp -- runs a table of argument lists through reseed_points_args_ok of
// levelsetfortran_amd/csrc/lsf_host_args_points.hpp on the CPU and prints one line per case:  name | return code | message
// (the message is what lsf_last_error() would hold; empty on LSF_OK).  tests/test_reseed_cpu.py holds what each case must give.
// The function never follows an array pointer, so the arrays are made-up addresses; xLo alone is read and is a real array.
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
#include "../../levelsetfortran_amd/csrc/lsf_host_args_points.hpp"

void show(const std::string& name, int rc)
{
    std::printf("%s | %d | %s\n", name.c_str(), rc, rc == LSF_OK ? "" : g_err.c_str());
    g_err.clear();
}

const void* at(uintptr_t a) { return (const void*)a; }
// arrays far apart from each other and from address 0
const void *const PHI = at(0x400000000000), *const MASK = at(0x600000000000), *const PTS = at(0x700000000000);
const void *const STATUS = at(0x800000000000), *const RAD = at(0x900000000000);
const double XLO[3] = {-1.0, 0.25, 3.0};
const double XLO_NAN[3] = {0.0, NAN, 0.0}, XLO_INF[3] = {0.0, 0.0, -INFINITY};
int g_nout;

// the argument list with values that pass; a case changes one or two of them
struct Res {
    const void *phi = PHI, *mask = MASK;
    int nx = 4, ny = 3, nz = 2;
    double dx = 0.5;
    const double* xLo = XLO;
    const void *pts = PTS, *rad = RAD;
    int npts = 5, per_cell = 16;
    double rmin = 0.1, rmax = 0.5, band = 3.0;
    int order = LSF_SAMPLE_CUBIC, iters = 4;
    double tol = 1e-3;
    const void* status = STATUS;
    const int* nout = &g_nout;
};
int call(const Res& a)
{
    return reseed_points_args_ok(a.phi, a.mask, a.nx, a.ny, a.nz, a.dx, a.xLo, a.pts, a.rad, a.npts, a.per_cell, a.rmin, a.rmax, a.band, a.order, a.iters,
                                 a.tol, a.status, a.nout);
}
template <typename F>
void run(const char* name, F change)
{
    Res a;
    change(a);
    show(name, call(a));
}
const void* off(const void* p, long bytes) { return (const char*)p + bytes; }
} // namespace

int main()
{
    const size_t n = 5 * 4 * 3; // points of the 4 x 3 x 2 grid
    run("valid", [](Res&) {});
    run("valid no optional", [](Res& a) { a.mask = a.status = nullptr; });
    run("valid from scratch", [](Res& a) { a.npts = 0, a.pts = a.rad = a.status = nullptr; });
    run("valid from scratch, stale pointers are ignored", [](Res& a) { a.npts = 0, a.status = PHI; });
    run("valid caps", [](Res& a) { a.per_cell = LSF_RESEED_MAX_PER_CELL, a.iters = LSF_RESEED_MAX_ITERS, a.tol = 0.0; });
    run("valid rmin equals rmax, linear, 1 cell", [](Res& a) { a.rmax = a.rmin, a.order = LSF_SAMPLE_LINEAR, a.nx = a.ny = a.nz = 1, a.per_cell = a.iters = 1; });
    run("phi NULL", [](Res& a) { a.phi = nullptr; });
    run("xLo NULL", [](Res& a) { a.xLo = nullptr; });
    run("nout NULL", [](Res& a) { a.nout = nullptr; });
    run("npts negative", [](Res& a) { a.npts = -1; });
    run("pts NULL", [](Res& a) { a.pts = nullptr; });
    run("rad NULL", [](Res& a) { a.rad = nullptr; });
    run("nx 0", [](Res& a) { a.nx = 0; });
    run("nz negative", [](Res& a) { a.nz = -1; });
    run("too many points", [](Res& a) { a.nx = 2047, a.ny = 1023, a.nz = 1023; });
    run("dx 0", [](Res& a) { a.dx = 0.0; });
    run("dx NaN", [](Res& a) { a.dx = NAN; });
    run("dx inf", [](Res& a) { a.dx = INFINITY; });
    run("xLo NaN", [](Res& a) { a.xLo = XLO_NAN; });
    run("xLo inf", [](Res& a) { a.xLo = XLO_INF; });
    run("per_cell 0", [](Res& a) { a.per_cell = 0; });
    run("per_cell beyond the cap", [](Res& a) { a.per_cell = LSF_RESEED_MAX_PER_CELL + 1; });
    run("rmin NaN", [](Res& a) { a.rmin = NAN; });
    run("rmax inf", [](Res& a) { a.rmax = INFINITY; });
    run("band NaN", [](Res& a) { a.band = NAN; });
    run("rmin 0", [](Res& a) { a.rmin = 0.0; });
    run("rmin negative", [](Res& a) { a.rmin = -0.1; });
    run("rmin above rmax", [](Res& a) { a.rmin = 0.6; });
    run("band equals rmin", [](Res& a) { a.band = 0.1; });
    run("order 2", [](Res& a) { a.order = 2; });
    run("order -1", [](Res& a) { a.order = -1; });
    run("iters 0", [](Res& a) { a.iters = 0; });
    run("iters beyond the cap", [](Res& a) { a.iters = LSF_RESEED_MAX_ITERS + 1; });
    run("tol negative", [](Res& a) { a.tol = -1e-300; });
    run("tol NaN", [](Res& a) { a.tol = NAN; });
    run("tol inf", [](Res& a) { a.tol = INFINITY; });
    run("status is phi", [](Res& a) { a.status = PHI; });
    run("status in the last byte of the mask", [&](Res& a) { a.status = off(MASK, (long)(n * 4) - 1); });
    run("status may just be behind the mask", [&](Res& a) { a.status = off(MASK, (long)(n * 4)); });
    run("status is pts", [](Res& a) { a.status = PTS; });
    run("status ends in rad", [](Res& a) { a.status = off(RAD, -(5 * 4) + 1); });
    run("pts is rad (inputs may alias)", [](Res& a) { a.pts = a.rad; });
    return 0;
}
