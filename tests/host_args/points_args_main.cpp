// points_args_main.cpp -- runs a table of argument lists through advect_points_args_ok and correct_field_args_ok of
// levelsetfortran_amd/csrc/lsf_host_args_points.hpp on the CPU and prints one line per case:  name | return code | message
// (the message is what lsf_last_error() would hold; empty on LSF_OK).  tests/test_points_cpu.py holds what each case must give.
// The functions never follow an array pointer, so the arrays are made-up addresses; xLo alone is read and is a real array.
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
const void *const U = at(0x100000000000), *const V = at(0x200000000000), *const W = at(0x300000000000), *const PHI = at(0x400000000000);
const void *const SPEED = at(0x500000000000), *const MASK = at(0x600000000000), *const PTS = at(0x700000000000);
const void *const STATUS = at(0x800000000000), *const RAD = at(0x900000000000);
const double XLO[3] = {-1.0, 0.25, 3.0};
const double XLO_NAN[3] = {0.0, NAN, 0.0}, XLO_INF[3] = {0.0, 0.0, -INFINITY};

// the argument list of each function with values that pass; a case changes one or two of them
struct Adv {
    const void *u = U, *v = V, *w = W, *phi = PHI, *speed = SPEED, *mask = MASK;
    int nx = 4, ny = 3, nz = 2;
    double dx = 0.5;
    const double* xLo = XLO;
    const void* pts = PTS;
    int npts = 5, order = LSF_SAMPLE_CUBIC, scheme = LSF_ADVECT_RK3;
    double dt = 0.1;
    int nsteps = 3;
    const void* status = STATUS;
};
struct Cor {
    const void *phi = PHI, *mask = MASK;
    int nx = 4, ny = 3, nz = 2;
    double dx = 0.5;
    const double* xLo = XLO;
    const void *pts = PTS, *rad = RAD;
    int npts = 5;
    double slack = 1.0;
    const void* status = STATUS;
};
int call(const Adv& a)
{
    return advect_points_args_ok(a.u, a.v, a.w, a.phi, a.speed, a.mask, a.nx, a.ny, a.nz, a.dx, a.xLo, a.pts, a.npts, a.order, a.scheme, a.dt, a.nsteps,
                                 a.status);
}
int call(const Cor& a) { return correct_field_args_ok(a.phi, a.mask, a.nx, a.ny, a.nz, a.dx, a.xLo, a.pts, a.rad, a.npts, a.slack, a.status); }

template <typename T, typename F>
void run(const char* name, F change)
{
    T a;
    change(a);
    show(name, call(a));
}
const void* off(const void* p, long bytes) { return (const char*)p + bytes; }
} // namespace

int main()
{
    const size_t n = 5 * 4 * 3; // points of the 4 x 3 x 2 grid
    // ---- lsf_advect_points
    run<Adv>("advect valid", [](Adv&) {});
    run<Adv>("advect valid velocity only", [](Adv& a) { a.phi = a.speed = nullptr; });
    run<Adv>("advect valid speed only", [](Adv& a) { a.u = a.v = a.w = nullptr; });
    run<Adv>("advect valid no optional", [](Adv& a) { a.mask = a.status = nullptr; });
    run<Adv>("advect valid negative dt", [](Adv& a) { a.dt = -0.1; });
    run<Adv>("advect valid euler linear", [](Adv& a) { a.scheme = LSF_ADVECT_EULER, a.order = LSF_SAMPLE_LINEAR; });
    run<Adv>("advect valid nsteps cap", [](Adv& a) { a.nsteps = LSF_ADVECT_POINTS_MAX_STEPS; });
    run<Adv>("advect valid 1 cell", [](Adv& a) { a.nx = a.ny = a.nz = 1; });
    run<Adv>("advect pts NULL", [](Adv& a) { a.pts = nullptr; });
    run<Adv>("advect xLo NULL", [](Adv& a) { a.xLo = nullptr; });
    run<Adv>("advect partial velocity 1", [](Adv& a) { a.v = a.w = nullptr; });
    run<Adv>("advect partial velocity 2", [](Adv& a) { a.u = nullptr; });
    run<Adv>("advect no group", [](Adv& a) { a.u = a.v = a.w = a.phi = a.speed = nullptr; });
    run<Adv>("advect speed without phi", [](Adv& a) { a.phi = nullptr; });
    run<Adv>("advect phi without speed", [](Adv& a) { a.speed = nullptr; });
    run<Adv>("advect npts 0", [](Adv& a) { a.npts = 0; });
    run<Adv>("advect npts negative", [](Adv& a) { a.npts = -3; });
    run<Adv>("advect nx 0", [](Adv& a) { a.nx = 0; });
    run<Adv>("advect nz negative", [](Adv& a) { a.nz = -1; });
    run<Adv>("advect too many points", [](Adv& a) { a.nx = 2047, a.ny = 1023, a.nz = 1023; });
    run<Adv>("advect dx 0", [](Adv& a) { a.dx = 0.0; });
    run<Adv>("advect dx negative", [](Adv& a) { a.dx = -0.5; });
    run<Adv>("advect dx NaN", [](Adv& a) { a.dx = NAN; });
    run<Adv>("advect dx inf", [](Adv& a) { a.dx = INFINITY; });
    run<Adv>("advect xLo NaN", [](Adv& a) { a.xLo = XLO_NAN; });
    run<Adv>("advect xLo inf", [](Adv& a) { a.xLo = XLO_INF; });
    run<Adv>("advect dt NaN", [](Adv& a) { a.dt = NAN; });
    run<Adv>("advect dt inf", [](Adv& a) { a.dt = -INFINITY; });
    run<Adv>("advect order 2", [](Adv& a) { a.order = 2; });
    run<Adv>("advect order -1", [](Adv& a) { a.order = -1; });
    run<Adv>("advect scheme 2", [](Adv& a) { a.scheme = 2; });
    run<Adv>("advect nsteps 0", [](Adv& a) { a.nsteps = 0; });
    run<Adv>("advect nsteps beyond the cap", [](Adv& a) { a.nsteps = LSF_ADVECT_POINTS_MAX_STEPS + 1; });
    run<Adv>("advect pts is u", [](Adv& a) { a.pts = U; });
    run<Adv>("advect pts in the last byte of w", [&](Adv& a) { a.pts = off(W, (long)(n * 8) - 1); });
    run<Adv>("advect pts just behind w", [&](Adv& a) { a.pts = off(W, (long)(n * 8)); });
    run<Adv>("advect pts ends in phi", [](Adv& a) { a.pts = off(PHI, -(5 * 3 * 8) + 1); });
    run<Adv>("advect pts is speed", [](Adv& a) { a.pts = SPEED; });
    run<Adv>("advect pts is the mask", [](Adv& a) { a.pts = MASK; });
    run<Adv>("advect status is pts", [](Adv& a) { a.status = PTS; });
    run<Adv>("advect status in the last byte of pts", [](Adv& a) { a.status = off(PTS, 5 * 3 * 8 - 1); });
    run<Adv>("advect status just behind pts", [](Adv& a) { a.status = off(PTS, 5 * 3 * 8); });
    run<Adv>("advect status is v", [](Adv& a) { a.status = V; });
    run<Adv>("advect status is the mask", [](Adv& a) { a.status = MASK; });
    run<Adv>("advect u is v (inputs may alias)", [](Adv& a) { a.v = a.u; });
    // ---- lsf_correct_field
    run<Cor>("correct valid", [](Cor&) {});
    run<Cor>("correct valid no optional", [](Cor& a) { a.mask = a.status = nullptr; });
    run<Cor>("correct valid slack 0", [](Cor& a) { a.slack = 0.0; });
    run<Cor>("correct phi NULL", [](Cor& a) { a.phi = nullptr; });
    run<Cor>("correct pts NULL", [](Cor& a) { a.pts = nullptr; });
    run<Cor>("correct rad NULL", [](Cor& a) { a.rad = nullptr; });
    run<Cor>("correct xLo NULL", [](Cor& a) { a.xLo = nullptr; });
    run<Cor>("correct npts 0", [](Cor& a) { a.npts = 0; });
    run<Cor>("correct ny 0", [](Cor& a) { a.ny = 0; });
    run<Cor>("correct too many points", [](Cor& a) { a.nx = 2047, a.ny = 1023, a.nz = 1023; });
    run<Cor>("correct dx 0", [](Cor& a) { a.dx = 0.0; });
    run<Cor>("correct dx NaN", [](Cor& a) { a.dx = NAN; });
    run<Cor>("correct xLo NaN", [](Cor& a) { a.xLo = XLO_NAN; });
    run<Cor>("correct xLo inf", [](Cor& a) { a.xLo = XLO_INF; });
    run<Cor>("correct slack negative", [](Cor& a) { a.slack = -1e-300; });
    run<Cor>("correct slack NaN", [](Cor& a) { a.slack = NAN; });
    run<Cor>("correct slack inf", [](Cor& a) { a.slack = INFINITY; });
    run<Cor>("correct phi is pts", [](Cor& a) { a.phi = PTS; });
    run<Cor>("correct phi ends in rad", [&](Cor& a) { a.phi = off(RAD, -(long)(n * 8) + 1); });
    run<Cor>("correct phi just before rad", [&](Cor& a) { a.phi = off(RAD, -(long)(n * 8)); });
    run<Cor>("correct phi is the mask", [](Cor& a) { a.phi = MASK; });
    run<Cor>("correct status is phi", [](Cor& a) { a.status = PHI; });
    run<Cor>("correct status is pts", [](Cor& a) { a.status = PTS; });
    run<Cor>("correct status in the last byte of rad", [](Cor& a) { a.status = off(RAD, 5 * 8 - 1); });
    run<Cor>("correct status just behind rad", [](Cor& a) { a.status = off(RAD, 5 * 8); });
    run<Cor>("correct status is the mask", [](Cor& a) { a.status = MASK; });
    run<Cor>("correct pts is rad (inputs may alias)", [](Cor& a) { a.pts = a.rad; });
    return 0;
}
