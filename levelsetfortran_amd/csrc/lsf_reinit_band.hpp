// lsf_reinit_band.hpp -- reinitialisation (subs.f90:717-931) on the cells of a caller's mask only: lsf_reinit_band.
//
// lsf_reinit* updates every interior cell in every sweep, yet the stages behind it (min/max flow, order-8 gradients, node
// advection) read phi only where phiNB / phiSB are 1.  Here the cells to update are listed once per call,
//     LIST = { interior points with mask == 1 on entry }
// with the list build of the min/max band (lsf_minmax_band.hpp: collect -> offsets -> gather -> sort by 8 x 8 x 4 bricks; the
// membership rule is the mask alone, k_mb_collect<true>), and a sweep is ONE launch over the list: one lane per list cell, 256
// consecutive list cells -- a few neighbouring bricks -- per block.  A lane decodes (i, j, k) from its point index, gathers the 19
// values of its stencil from the field as it was at the start of the sweep, applies cell_update<STRICT> (lsf_cell.hpp: the update
// k_reinit_jacobi applies, same weno_ok rule) and stores the new value into the OTHER field buffer: two full fields in rotation
// (the caller's and the workspace's second field, filled by one copy at entry).  Every list cell is written in every sweep and no
// other point ever is, so the buffer a sweep writes is complete when the sweep ends; when the last sweep has written the
// workspace's buffer its list cells are scattered into the caller's field (k_rb_scatter).  Beyond the list build and that one copy
// nothing is proportional to the grid: a sweep costs what the list costs.
//
// The sign field phiS (subs.f90:731) is read at list cells only and kept as a compact array in list order.  Wall points are never
// written and the extrapolation boundary condition (subs.f90:859-897) is not applied: points outside the list keep their values.
// The RMS of a sweep is sqrt(sum over list cells (new - old)^2 / nL): one partial per block, added in a fixed order (k_finish).
// Plain launches only: nothing here waits for another block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_band_cell.hpp"
#include "lsf_minmax_band.hpp"

namespace lsf {

// the sign field at the list cells, in list order (phi on entry, or the caller's phiS)
static __global__ __launch_bounds__(256) void k_rb_gather(const int* __restrict__ L, const double* __restrict__ F, int nL, double* __restrict__ v)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nL) v[e] = F[L[e]];
}

// end of a call whose last sweep wrote the second field: its list cells into the caller's field
static __global__ __launch_bounds__(256) void k_rb_scatter(const int* __restrict__ L, const double* __restrict__ G, int nL, double* __restrict__ F)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nL) {
        const int p = L[e];
        F[p] = G[p];
    }
}

// One sweep: list cell e of chunk blockIdx.x.  A = the field at the start of the sweep, Bout = the other field buffer, phiS = the
// compact sign field.  Bounds: lsf_band_cell.hpp (band_stencil7 forms every address that is not the lane's own).
template <bool STRICT>
__global__ __launch_bounds__(MB_CH) void k_reinit_band(const double* __restrict__ A, double* __restrict__ Bout, const double* __restrict__ phiS,
                                                       const int* __restrict__ L, int nL, int nx, int ny, int nz, double dx, double h,
                                                       double* __restrict__ partials, const int* __restrict__ done)
{
    __shared__ double red[MB_CH / 64];
    if (done[CTL_STOP]) return;
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    double acc = 0.0;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        int i, j, k;
        band_decode(p, nx, ny, i, j, k);
        const bool weno_ok = i > 3 && i < nx - 4 && j > 3 && j < ny - 4 && k > 3 && k < nz - 4;
        const double* c = A + p;
        const double phic = c[0];
        double qx[7], qy[7], qz[7];
        const unsigned sx = (unsigned)(nx + 1), sy = (unsigned)(ny + 1);
        band_stencil7(c, sx, (long)sx * sy, weno_ok, qx, qy, qz);
        const double inv_dx = 1.0 / dx, floor2 = 1.E-99 * dx * dx / 13.0;
        const double newv = cell_update<STRICT>(qx, qy, qz, weno_ok, phiS[e], dx, inv_dx, floor2, h);
        Bout[p] = newv;
        const double dlt = newv - phic;
        acc = dlt * dlt;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

} // namespace lsf
