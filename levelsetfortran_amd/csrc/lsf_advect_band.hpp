// lsf_advect_band.hpp -- level-set transport on the cells of a caller's mask only: lsf_advect_field_band (include/lsf.h).
//
// lsf_advect_field runs three WENO5 stages over every interior cell; the stage behind it in a time loop (lsf_reinit_band) visits a
// list.  Here the transport operator of lsf_advect_field.hpp (axis_pair without the y quirk, advect_rhs -- both used unchanged) is
// applied to the list of lsf_reinit_band,
//     LIST = { interior points with mask == 1 on entry },
// built by the same machinery (band_list_count<true> / band_list_sort: brick-sorted 32-bit point indices).  A stage is ONE launch
// over the list (k_advect_band_stage, modelled on k_reinit_band): one lane per list cell, MB_CH consecutive entries -- a few
// neighbouring bricks -- per block.  A lane decodes (i, j, k) from its point index, gathers its stencil from the stage's input
// field (19 values when the cell is WENO, 7 otherwise), u, v, w, speed and the step's old phi at its own point, and stores the
// blend at its own point of the output field.  The stage buffers are FULL fields that start as copies of phi: off-list points never
// change in any of them, so a stencil point outside the list reads phi as it came, whatever the stage.
//
// Bounds: lsf_band_cell.hpp.  The edge pass reads the mask at the six neighbours of an interior point (band_listed6); u, v, w,
// speed, the old phi and the store are at the lane's own point.
//
// The trace is lsf_advect_field's: the last stage of a step reduces the bit pattern of |new - old| (wave_umax_x) to one partial per
// block and k_advect_finish, reused as it is, closes the step.  Plain launches only: no atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_advect_field.hpp"
#include "lsf_band_cell.hpp"
#include "lsf_minmax_band.hpp"

namespace lsf {

constexpr int ADVB_EDGE = 1, ADVB_NEG = 2; // the byte of the edge pass: the entry is an edge cell | phi < 0 on entry

// One stage: list cell e of chunk blockIdx.x.  A = the stage's input field, Bout = its output (never A); P0 = the field at the start
// of the step, or nullptr: out = t = a - dt R(a); with P0: out = c_old * P0 + c_new * t.  P0 may BE Bout (stage 3 of RK3 writes the
// caller's field in place): a lane reads P0 at its own point only, before it stores there.  partials != nullptr: the last stage of
// a step, one maximum of |out - old| per block (old = P0, or A when there is none) as a bit pattern.
template <bool STRICT, bool HASV, bool HASF>
__global__ __launch_bounds__(MB_CH) void k_advect_band_stage(const double* __restrict__ A, double* Bout, const double* P0,
                                                             const double* __restrict__ U, const double* __restrict__ V,
                                                             const double* __restrict__ W, const double* __restrict__ F,
                                                             const int* __restrict__ L, int nL, int nx, int ny, int nz, double dx, double dt,
                                                             double c_old, double c_new, unsigned long long* __restrict__ partials,
                                                             const int* __restrict__ done)
{
    if (done[CTL_STOP]) return;
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long acc = 0ull;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        int i, j, k;
        band_decode(p, nx, ny, i, j, k);
        const bool weno_ok = i > 3 && i < nx - 4 && j > 3 && j < ny - 4 && k > 3 && k < nz - 4;
        const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
        const double* c = A + p;
        double qx[7], qy[7], qz[7];
        const double phic = c[0];
        band_stencil7(c, rs, ps, weno_ok, qx, qy, qz);
        double u = 0.0, v = 0.0, w = 0.0, f = 0.0;
        if constexpr (HASV) u = U[p], v = V[p], w = W[p];
        if constexpr (HASF) f = F[p];
        const bool blend = P0 != nullptr;
        const double old = blend ? P0[p] : phic;
        const double inv_dx = 1.0 / dx, floor2 = 1.E-99 * dx * dx / 13.0;
        double ax, bx, ay, by, az, bz;
        axis_pair<STRICT>(qx, weno_ok, false, dx, floor2, ax, bx);
        axis_pair<STRICT>(qy, weno_ok, false, dx, floor2, ay, by);
        axis_pair<STRICT>(qz, weno_ok, false, dx, floor2, az, bz);
        const double R = advect_rhs<STRICT, HASV, HASF>(ax, bx, ay, by, az, bz, u, v, w, f, inv_dx);
        const double out = stage_blend<STRICT>(phic, dt, R, blend, c_old, old, c_new);
        Bout[p] = out;
        acc = (unsigned long long)__double_as_longlong(__builtin_fabs(out - old));
    }
    if (partials) {
        acc = block_umax<MB_CH / 64>(wave_umax_x(acc), threadIdx.x);
        if (threadIdx.x == 0) partials[blockIdx.x] = acc;
    }
}

// The inputs AT LIST CELLS, once per call: the largest |u| + |v| + |w| + |speed| (absent fields left out, added left to right) and
// the number of non-finite values.  One pair of partials per block; the host finishes (at most ADV_SCAN_BLOCKS pairs), as with
// k_advect_scan, whose body this is.  Nothing of the inputs outside the list is read: a NaN there is legal.
static __global__ __launch_bounds__(256) void k_advect_band_scan(const double* __restrict__ U, const double* __restrict__ V,
                                                                 const double* __restrict__ W, const double* __restrict__ F,
                                                                 const int* __restrict__ L, int nL, double* __restrict__ pmax,
                                                                 unsigned long long* __restrict__ pcnt)
{
    advect_scan_body<true>(U, V, W, F, L, nL, pmax, pcnt);
}

// The edge pass, once per call, before the first step: one byte per list entry.  ADVB_EDGE: at least one of the six axis
// neighbours is not in LIST (band_listed6); ADVB_NEG: phi < 0 on entry.
static __global__ __launch_bounds__(256) void k_advect_band_edge(const int32_t* __restrict__ mask, const double* __restrict__ phi,
                                                                 const int* __restrict__ L, int nL, int nx, int ny, int nz,
                                                                 unsigned char* __restrict__ flag)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nL) return;
    const unsigned p = (unsigned)L[e];
    int i, j, k;
    band_decode(p, nx, ny, i, j, k);
    const bool in = band_listed6(mask + p, i, j, k, nx, ny, nz, nx + 1, (long)(nx + 1) * (ny + 1));
    flag[e] = (unsigned char)((in ? 0 : ADVB_EDGE) | (phi[p] < 0.0 ? ADVB_NEG : 0));
}

// The closing pass, once per call: over the edge cells, the smallest |phi| as a bit pattern (at most that of +inf: on LSF_OK no list
// cell is NaN) and the number of cells whose (phi < 0) differs from the entry's; the number of edge cells too.  One triple of
// partials per block (at most ADV_SCAN_BLOCKS); the host finishes them in block order.
static __global__ __launch_bounds__(256) void k_advect_band_close(const double* __restrict__ phi, const int* __restrict__ L,
                                                                  const unsigned char* __restrict__ flag, int nL,
                                                                  unsigned long long* __restrict__ pmin, unsigned long long* __restrict__ pedge,
                                                                  unsigned long long* __restrict__ pflip)
{
    __shared__ unsigned long long rmn[4], re[4], rf[4];
    unsigned long long mn = ADV_INF_BITS, ne = 0ull, nf = 0ull;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < nL; e += 256L * gridDim.x) {
        const int fl = flag[e];
        if (fl & ADVB_EDGE) {
            const double x = phi[L[e]];
            const unsigned long long b = (unsigned long long)__double_as_longlong(__builtin_fabs(x));
            mn = b < mn ? b : mn;
            ne += 1ull;
            nf += (unsigned long long)((x < 0.0) != ((fl & ADVB_NEG) != 0));
        }
    }
    // counts and a minimum: the wave-level pieces of lsf_block_reduce.hpp, one barrier
    mn = wave_umin(mn);
    wave_usum_each(ne, nf);
    if ((threadIdx.x & 63) == 0) rmn[threadIdx.x >> 6] = mn, re[threadIdx.x >> 6] = ne, rf[threadIdx.x >> 6] = nf;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = rmn[0];
        for (int q = 1; q < 4; ++q) t = rmn[q] < t ? rmn[q] : t;
        pmin[blockIdx.x] = t;
        pedge[blockIdx.x] = (re[0] + re[1]) + (re[2] + re[3]);
        pflip[blockIdx.x] = (rf[0] + rf[1]) + (rf[2] + rf[3]);
    }
}

} // namespace lsf
