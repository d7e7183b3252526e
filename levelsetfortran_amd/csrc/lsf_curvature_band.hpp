// lsf_curvature_band.hpp -- mean and Gaussian curvature of the level sets on the cells of a caller's mask: lsf_curvature_band
// (include/lsf.h).
//
// The list is lsf_reinit_band's,
//     LIST = { interior points with mask == 1 on entry },
// built by the same machinery (band_list_count<true> / band_list_sort: brick-sorted 32-bit point indices).  The call is ONE launch
// over the list (k_curvature_band, modelled on k_reinit_band / k_advect_band_stage): one lane per list cell, MB_CH consecutive
// entries -- a few neighbouring bricks -- per block.  A lane decodes (i, j, k) from its point index, gathers the 19 values of its
// stencil (the cell, +-1 on each axis, the 12 edge diagonals) through L1/L2, evaluates the statement of the header without
// contraction and stores up to three values at its own point.  The optional outputs are chosen by template instance: a lane never
// branches on them and an instance without gauss does not compute K.
//
// Bounds: lsf_band_cell.hpp.  What is this kernel's own: every stencil point, the 12 diagonals among them, is at an offset in
// {-1, 0, 1}^3 of an interior point.  The stores are at the lane's own point.
//
// The report: per block three counts (degenerate, clamped and non-finite cells) and the bit pattern of the largest |kappa| as stored
// (wave_umax_x of lsf_block_reduce.hpp; every NaN lies above +inf, and on LSF_OK there is none), finished by the host in block order.
// Counts are integers and the maximum is one of bit patterns, so no order of reduction reaches a result.  One plain launch: no
// atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_band_cell.hpp"
#include "lsf_block_reduce.hpp"
#include "lsf_minmax_band.hpp"

namespace lsf {

constexpr double CURV_DEGENERATE_G2 = 1e-24; // g2 below this: a flat spot, H = K = 0
constexpr int CURV_NPART = 4;                // partials per block: degenerate, clamped, non-finite, max |kappa| (bits)

// The nine derivatives of the header's statement at one interior point q: second-order central differences of the 19 values
// s(a, b, c), evaluated as written, without contraction.  Shared with k_advect_band_curv_stage (lsf_evolve_band_curv.hpp).
struct CurvD {
    double px, py, pz, pxx, pyy, pzz, pxy, pxz, pyz;
};

__device__ __forceinline__ CurvD curv_derivs(const double* __restrict__ q, long rs, long ps, double two_dx, double dx2, double four_dx2)
{
#pragma clang fp contract(off)
    // s(a, b, c) of the header: an interior point, so +-1 on every axis lies inside the field
    const double c = q[0];
    const double xm = q[-1], xp = q[1], ym = q[-rs], yp = q[rs], zm = q[-ps], zp = q[ps];
    const double xpyp = q[1 + rs], xpym = q[1 - rs], xmyp = q[-1 + rs], xmym = q[-1 - rs];
    const double xpzp = q[1 + ps], xpzm = q[1 - ps], xmzp = q[-1 + ps], xmzm = q[-1 - ps];
    const double ypzp = q[rs + ps], ypzm = q[rs - ps], ymzp = q[-rs + ps], ymzm = q[-rs - ps];
    CurvD d;
    d.px = (xp - xm) / two_dx, d.py = (yp - ym) / two_dx, d.pz = (zp - zm) / two_dx;
    d.pxx = ((xp - 2. * c) + xm) / dx2, d.pyy = ((yp - 2. * c) + ym) / dx2, d.pzz = ((zp - 2. * c) + zm) / dx2;
    d.pxy = (((xpyp - xpym) - xmyp) + xmym) / four_dx2;
    d.pxz = (((xpzp - xpzm) - xmzp) + xmzm) / four_dx2;
    d.pyz = (((ypzp - ypzm) - ymzp) + ymzm) / four_dx2;
    return d;
}

// H of the statement before the clamp, with g2, g = sqrt(g2) and the DEGENERATE flag (then H = 0.0)
__device__ __forceinline__ double curv_mean(const CurvD& d, double& g2, double& g, bool& deg)
{
#pragma clang fp contract(off)
    const double px = d.px, py = d.py, pz = d.pz, pxx = d.pxx, pyy = d.pyy, pzz = d.pzz;
    g2 = (px * px + py * py) + pz * pz;
    g = __builtin_sqrt(g2);
    deg = g2 < CURV_DEGENERATE_G2; // a NaN g2 is not degenerate
    const double num = ((px * px) * (pyy + pzz) + (py * py) * (pxx + pzz)) + (pz * pz) * (pxx + pyy);
    const double mix = ((px * py) * d.pxy + (px * pz) * d.pxz) + (py * pz) * d.pyz;
    const double H = (num - 2. * mix) / (g2 * g);
    return deg ? 0.0 : H;
}

// List cell e of chunk blockIdx.x.  two_dx = 2.*dx, dx2 = dx*dx, four_dx2 = 4.*(dx*dx), computed once on the host; lim = clamp / dx
// and lim2 = lim*lim likewise, used when CLAMP.  part: CURV_NPART words per block.
template <bool HASK, bool HASG, bool CLAMP>
__global__ __launch_bounds__(MB_CH) void k_curvature_band(const double* __restrict__ phi, const int* __restrict__ L, int nL, int nx, int ny,
                                                          double* __restrict__ kappa, double* __restrict__ gauss, double* __restrict__ gmag,
                                                          double two_dx, double dx2, double four_dx2, double lim, double lim2,
                                                          unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[MB_CH / 64][CURV_NPART];
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long ndeg = 0ull, nclamp = 0ull, nbad = 0ull, amax = 0ull;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
        bool deg;
        double g2, g;
        const CurvD d = curv_derivs(phi + p, rs, ps, two_dx, dx2, four_dx2);
        double H = curv_mean(d, g2, g, deg);
        bool clamped = false;
        if constexpr (CLAMP) {
            clamped = H > lim || H < -lim;
            if (H > lim) H = lim;
            if (H < -lim) H = -lim;
        }
        bool bad = !__builtin_isfinite(H);
        kappa[p] = H;
        if constexpr (HASK) {
            const double px = d.px, py = d.py, pz = d.pz, pxx = d.pxx, pyy = d.pyy, pzz = d.pzz, pxy = d.pxy, pxz = d.pxz, pyz = d.pyz;
            const double A = ((px * px) * (pyy * pzz - pyz * pyz) + (py * py) * (pxx * pzz - pxz * pxz)) + (pz * pz) * (pxx * pyy - pxy * pxy);
            const double B = ((px * py) * (pxz * pyz - pxy * pzz) + (py * pz) * (pxy * pxz - pyz * pxx)) + (px * pz) * (pxy * pyz - pxz * pyy);
            double K = (A + 2. * B) / (g2 * g2);
            if (deg) K = 0.0;
            if constexpr (CLAMP) {
                clamped = clamped || K > lim2 || K < -lim2;
                if (K > lim2) K = lim2;
                if (K < -lim2) K = -lim2;
            }
            bad = bad || !__builtin_isfinite(K);
            gauss[p] = K;
        }
        if constexpr (HASG) {
            bad = bad || !__builtin_isfinite(g);
            gmag[p] = g;
        }
        ndeg = deg ? 1ull : 0ull, nclamp = clamped ? 1ull : 0ull, nbad = bad ? 1ull : 0ull;
        amax = (unsigned long long)__double_as_longlong(__builtin_fabs(H));
    }
    // counts and a maximum: the wave-level pieces of lsf_block_reduce.hpp, one LDS array, one barrier
    amax = wave_umax_x(amax);
    wave_usum_each(ndeg, nclamp, nbad);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* r = red[threadIdx.x >> 6];
        r[0] = ndeg, r[1] = nclamp, r[2] = nbad, r[3] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[CURV_NPART] = {red[0][0], red[0][1], red[0][2], red[0][3]};
        for (int w = 1; w < MB_CH / 64; ++w) {
            t[0] += red[w][0], t[1] += red[w][1], t[2] += red[w][2];
            t[3] = red[w][3] > t[3] ? red[w][3] : t[3];
        }
        unsigned long long* o = part + (size_t)blockIdx.x * CURV_NPART;
        o[0] = t[0], o[1] = t[1], o[2] = t[2], o[3] = t[3];
    }
}

} // namespace lsf
