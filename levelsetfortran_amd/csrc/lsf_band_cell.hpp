// lsf_band_cell.hpp -- what a lane of a band kernel does with its list cell before any arithmetic: the decode of the point index,
// the joint WENO rule, the gather of the 7-point stencils and the "all six neighbours are in LIST" test.
//
// Bounds, stated once for every kernel that works on a list (DESIGN.md sections 4.2 / 4.12): no address is formed outside the
// field, by construction and not by a range check.  A list entry is an interior point: k_mb_collect<true> (lsf_minmax_band.hpp)
// keeps 1..n-1 on each axis only, and the host refuses fields beyond 2^31 - 1 points, so an entry is a non-negative 32-bit index
// below the number of points.  An interior point has every point at an offset in {-1, 0, 1}^3 inside the field: 0 <= i-1 and
// i+1 <= nx, likewise j and k.  The first-order branch of band_stencil7 reads +-1 on each axis and nothing else; band_listed6
// reads the mask at the same six points.  The WENO branch reads +-3 on each axis and is taken only if weno_ok holds:
// 4 <= i <= nx-5, 4 <= j <= ny-5 and 4 <= k <= nz-5, where i-3 >= 1 and i+3 <= nx-2 (likewise j, k).  Whatever else a kernel
// reads or writes is at the lane's own point or its own list entry, unless its header says otherwise; lanes with e >= nL touch no
// memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsf {

// (i, j, k) of a point index
__device__ __forceinline__ void band_decode(unsigned p, int nx, int ny, int& i, int& j, int& k)
{
    const unsigned sx = (unsigned)(nx + 1), sy = (unsigned)(ny + 1);
    const unsigned q = p / sx;
    i = (int)(p - q * sx), k = (int)(q / sy), j = (int)(q - (unsigned)k * sy);
}

// The reference's joint WENO rule -- cells 4..n-5 on all three axes, first-order differences otherwise -- is
//     weno_ok = i > 3 && i < nx - 4 && j > 3 && j < ny - 4 && k > 3 && k < nz - 4
// and stays written out in the three kernels that use it (k_reinit_band, k_advect_band_stage, k_advect_band_curv_stage): inside a
// function -- its own, or a per-cell body shared by the stage kernels -- it is folded into one mask before the function is
// inlined, the divisions of the decode are then no longer skipped for i <= 3, and the machine code of every stage kernel changes.

// The stencils of the interior point at c along x, y and z (rs, ps: the strides of a row and a plane): q[3] is the cell,
// q[3 +- m] the points m away.  Without weno_ok only q[2..4] are read; the others are 0.0 and never consumed.
__device__ __forceinline__ void band_stencil7(const double* c, long rs, long ps, bool weno_ok, double (&qx)[7], double (&qy)[7], double (&qz)[7])
{
    const double phic = c[0];
    if (weno_ok) { // 4 <= i <= nx-5 and likewise j, k: +-3 on every axis lies inside the field
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            qx[m] = m == 3 ? phic : c[m - 3];
            qy[m] = m == 3 ? phic : c[(m - 3) * rs];
            qz[m] = m == 3 ? phic : c[(m - 3) * ps];
        }
    } else { // an interior point: +-1 on every axis lies inside the field
#pragma unroll
        for (int m = 0; m < 7; ++m) qx[m] = qy[m] = qz[m] = 0.0;
        qx[2] = c[-1], qx[3] = phic, qx[4] = c[1];
        qy[2] = c[-rs], qy[3] = phic, qy[4] = c[rs];
        qz[2] = c[-ps], qz[3] = phic, qz[4] = c[ps];
    }
}

// All six axis neighbours of the interior point (i, j, k) at m are in LIST: a neighbour is in LIST if it is interior on that axis
// (the other two coordinates are this cell's) and its mask is 1; a wall point never is, any other mask value means "not in the list".
__device__ __forceinline__ bool band_listed6(const int32_t* m, int i, int j, int k, int nx, int ny, int nz, long rs, long ps)
{
    return (i > 1 && m[-1] == 1) && (i < nx - 1 && m[1] == 1) && (j > 1 && m[-rs] == 1) && (j < ny - 1 && m[rs] == 1) &&
           (k > 1 && m[-ps] == 1) && (k < nz - 1 && m[ps] == 1);
}

} // namespace lsf
