// redistance_args_main.cpp -- runs a table of argument lists through redistance_band_args_ok of
// levelsetfortran_amd/csrc/lsf_host_args_redistance.hpp on the CPU and prints one line per case:  name | return code | message
// (the message is what lsf_last_error() would hold; empty on LSF_OK).  tests/test_redistance_band_cpu.py holds what each case must
// give.  The function never follows an array pointer, so the arrays are made-up addresses.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/lsf_redistance.h"

namespace {
std::string g_err;
int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
#include "../../levelsetfortran_amd/csrc/lsf_host_args.hpp"
#include "../../levelsetfortran_amd/csrc/lsf_host_args_redistance.hpp"

void show(const std::string& name, int rc)
{
    std::printf("%s | %d | %s\n", name.c_str(), rc, rc == LSF_OK ? "" : g_err.c_str());
    g_err.clear();
}

const void* at(uintptr_t a) { return (const void*)a; }
// arrays far apart from each other and from address 0
const void *const PHI = at(0x100000000000), *const MASK = at(0x200000000000);

// the argument list with values that pass; a case changes one or two of them
struct Redist {
    const void *phi = PHI, *mask = MASK;
    int nx = 4, ny = 3, nz = 2;
    double dx = 0.5, near = 2.5;
    int iters = 8;
    double tol = 1e-9;
    int max_passes = 64, trace_cap = 64;
};
int call(const Redist& a) { return redistance_band_args_ok(a.phi, a.mask, a.nx, a.ny, a.nz, a.dx, a.near, a.iters, a.tol, a.max_passes, a.trace_cap); }

template <typename F>
void run(const char* name, F change)
{
    Redist a;
    change(a);
    show(name, call(a));
}
const void* off(const void* p, long bytes) { return (const char*)p + bytes; }
} // namespace

int main()
{
    const long n = 5 * 4 * 3; // points of the 4 x 3 x 2 grid
    run("valid", [](Redist&) {});
    run("valid 2 cells an axis", [](Redist& a) { a.nx = a.ny = a.nz = 2; });
    run("valid tol 0", [](Redist& a) { a.tol = 0.0; });
    run("valid one iteration, one pass, no trace", [](Redist& a) { a.iters = a.max_passes = 1, a.trace_cap = 0; });
    run("valid tiny near", [](Redist& a) { a.near = 1e-300; });
    run("phi NULL", [](Redist& a) { a.phi = nullptr; });
    run("mask NULL", [](Redist& a) { a.mask = nullptr; });
    run("phi and mask NULL", [](Redist& a) { a.phi = a.mask = nullptr; });
    run("nx 1", [](Redist& a) { a.nx = 1; });
    run("ny 0", [](Redist& a) { a.ny = 0; });
    run("nz negative", [](Redist& a) { a.nz = -1; });
    run("field too large", [](Redist& a) { a.nx = a.ny = a.nz = 2100; });
    run("plane too large", [](Redist& a) { a.nx = a.ny = 16000, a.nz = 2; });
    run("too many points", [](Redist& a) { a.nx = 2047, a.ny = 1023, a.nz = 1023; });
    run("dx 0", [](Redist& a) { a.dx = 0.0; });
    run("dx negative", [](Redist& a) { a.dx = -0.5; });
    run("dx NaN", [](Redist& a) { a.dx = NAN; });
    run("dx inf", [](Redist& a) { a.dx = INFINITY; });
    run("near 0", [](Redist& a) { a.near = 0.0; });
    run("near negative", [](Redist& a) { a.near = -2.5; });
    run("near NaN", [](Redist& a) { a.near = NAN; });
    run("near inf", [](Redist& a) { a.near = INFINITY; });
    run("iters 0", [](Redist& a) { a.iters = 0; });
    run("iters negative", [](Redist& a) { a.iters = -3; });
    run("tol negative", [](Redist& a) { a.tol = -1e-9; });
    run("tol NaN", [](Redist& a) { a.tol = NAN; });
    run("tol inf", [](Redist& a) { a.tol = INFINITY; });
    run("max_passes 0", [](Redist& a) { a.max_passes = 0; });
    run("max_passes negative", [](Redist& a) { a.max_passes = -1; });
    run("trace_cap negative", [](Redist& a) { a.trace_cap = -1; });
    run("dx and near wrong", [](Redist& a) { a.dx = a.near = 0.0; });
    run("iters and max_passes wrong", [](Redist& a) { a.iters = a.max_passes = 0; });
    run("phi is the mask", [](Redist& a) { a.phi = MASK; });
    run("phi in the last byte of the mask", [&](Redist& a) { a.phi = off(MASK, n * 4 - 1); });
    run("valid phi just behind the mask", [&](Redist& a) { a.phi = off(MASK, n * 4); });
    run("phi ends in the mask", [&](Redist& a) { a.phi = off(MASK, -n * 8 + 1); });
    run("valid phi just before the mask", [&](Redist& a) { a.phi = off(MASK, -n * 8); });
    return 0;
}
