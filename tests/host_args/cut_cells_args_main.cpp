// cut_cells_args_main.cpp -- runs a table of argument lists through cut_cells_args_ok of
// levelsetfortran_amd/csrc/lsf_host_args_cut.hpp on the CPU and prints one line per case:  name | return code | message
// (the message is what lsf_last_error() would hold; empty on LSF_OK).  tests/test_host_cut_args_cpu.py holds what each case must
// give.  The function never follows an array pointer, so the arrays are made-up addresses.
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
#include "../../levelsetfortran_amd/csrc/lsf_host_args_cut.hpp"

void show(const std::string& name, int rc)
{
    std::printf("%s | %d | %s\n", name.c_str(), rc, rc == LSF_OK ? "" : g_err.c_str());
    g_err.clear();
}

const void* at(uintptr_t a) { return (const void*)a; }
// arrays far apart from each other and from address 0
const void *const PHI = at(0x100000000000), *const MASK = at(0x200000000000), *const VOF = at(0x300000000000), *const AX = at(0x400000000000);
const void *const AY = at(0x500000000000), *const AZ = at(0x600000000000), *const BX = at(0x700000000000), *const BY = at(0x800000000000);
const void *const BZ = at(0x900000000000), *const VOLUME = at(0xa00000000000);

// the argument list with values that pass; a case changes one or two of them
struct Cut {
    const void *phi = PHI, *mask = MASK;
    int nx = 4, ny = 3, nz = 2;
    double dx = 0.5, iso = 0.25;
    const void *vof = VOF, *ax = AX, *ay = AY, *az = AZ, *bx = BX, *by = BY, *bz = BZ, *volume = VOLUME;
};
int call(const Cut& a) { return cut_cells_args_ok(a.phi, a.mask, a.nx, a.ny, a.nz, a.dx, a.iso, a.vof, a.ax, a.ay, a.az, a.bx, a.by, a.bz, a.volume); }

template <typename F>
void run(const char* name, F change)
{
    Cut a;
    change(a);
    show(name, call(a));
}
const void* off(const void* p, long bytes) { return (const char*)p + bytes; }
} // namespace

int main()
{
    const long n = 5 * 4 * 3; // points of the 4 x 3 x 2 grid
    run("valid", [](Cut&) {});
    run("valid vof only", [](Cut& a) { a.ax = a.ay = a.az = a.bx = a.by = a.bz = a.volume = nullptr; });
    run("valid apertures only", [](Cut& a) { a.vof = a.bx = a.by = a.bz = a.volume = nullptr; });
    run("valid area vector only", [](Cut& a) { a.vof = a.ax = a.ay = a.az = a.volume = nullptr; });
    run("valid volume only", [](Cut& a) { a.vof = a.ax = a.ay = a.az = a.bx = a.by = a.bz = nullptr; });
    run("valid 2 cells an axis", [](Cut& a) { a.nx = a.ny = a.nz = 2; });
    run("valid negative iso", [](Cut& a) { a.iso = -3.0; });
    run("phi NULL", [](Cut& a) { a.phi = nullptr; });
    run("mask NULL", [](Cut& a) { a.mask = nullptr; });
    run("phi and mask NULL", [](Cut& a) { a.phi = a.mask = nullptr; });
    run("nx 1", [](Cut& a) { a.nx = 1; });
    run("ny 0", [](Cut& a) { a.ny = 0; });
    run("nz negative", [](Cut& a) { a.nz = -1; });
    run("field too large", [](Cut& a) { a.nx = a.ny = a.nz = 2100; });
    run("plane too large", [](Cut& a) { a.nx = a.ny = 16000, a.nz = 2; });
    run("too many points", [](Cut& a) { a.nx = 2047, a.ny = 1023, a.nz = 1023; });
    run("dx 0", [](Cut& a) { a.dx = 0.0; });
    run("dx negative", [](Cut& a) { a.dx = -0.5; });
    run("dx NaN", [](Cut& a) { a.dx = NAN; });
    run("dx inf", [](Cut& a) { a.dx = INFINITY; });
    run("iso NaN", [](Cut& a) { a.iso = NAN; });
    run("iso inf", [](Cut& a) { a.iso = -INFINITY; });
    run("apertures 1 of 3", [](Cut& a) { a.ay = a.az = nullptr; });
    run("apertures 2 of 3", [](Cut& a) { a.ax = nullptr; });
    run("area vector 1 of 3", [](Cut& a) { a.bx = a.by = nullptr; });
    run("area vector 2 of 3", [](Cut& a) { a.bz = nullptr; });
    run("both groups incomplete", [](Cut& a) { a.ax = a.bx = nullptr; });
    run("nothing requested", [](Cut& a) { a.vof = a.ax = a.ay = a.az = a.bx = a.by = a.bz = a.volume = nullptr; });
    run("vof is phi", [](Cut& a) { a.vof = PHI; });
    run("vof in the last byte of phi", [&](Cut& a) { a.vof = off(PHI, n * 8 - 1); });
    run("valid vof just behind phi", [&](Cut& a) { a.vof = off(PHI, n * 8); });
    run("vof ends in phi", [&](Cut& a) { a.vof = off(PHI, -n * 8 + 1); });
    run("vof is the mask", [](Cut& a) { a.vof = MASK; });
    run("vof in the last byte of the mask", [&](Cut& a) { a.vof = off(MASK, n * 4 - 1); });
    run("valid vof just behind the mask", [&](Cut& a) { a.vof = off(MASK, n * 4); });
    run("ax is phi", [](Cut& a) { a.ax = PHI; });
    run("ax is vof", [](Cut& a) { a.ax = VOF; });
    run("ay is the mask", [](Cut& a) { a.ay = MASK; });
    run("ay is ax", [](Cut& a) { a.ay = AX; });
    run("az in the last byte of ay", [&](Cut& a) { a.az = off(AY, n * 8 - 1); });
    run("valid az just behind ay", [&](Cut& a) { a.az = off(AY, n * 8); });
    run("az is vof", [](Cut& a) { a.az = VOF; });
    run("bx is az", [](Cut& a) { a.bx = AZ; });
    run("bx is phi", [](Cut& a) { a.bx = PHI; });
    run("by is bx", [](Cut& a) { a.by = BX; });
    run("by is the mask", [](Cut& a) { a.by = MASK; });
    run("bz is by", [](Cut& a) { a.bz = BY; });
    run("bz is vof", [](Cut& a) { a.bz = VOF; });
    run("bz ends in ax", [&](Cut& a) { a.bz = off(AX, -n * 8 + 1); });
    run("valid mask is phi (inputs may alias)", [](Cut& a) { a.mask = PHI; });
    return 0;
}
