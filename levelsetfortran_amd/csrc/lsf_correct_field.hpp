// lsf_correct_field.hpp -- the scatter from marker particles back to the grid, the correction step of the particle level set
// (Enright, Fedkiw, Ferziger, Mitchell 2002): lsf_correct_field (include/lsf.h).
//
// Three plain launches in stream order:
//   k_cf_init     plus = minus = key(phi) at every point of the list (with a mask) or of the grid, key the order-preserving 64-bit
//                 transform b ^ (b >> 63 ? ~0 : 1 << 63) of the bit pattern b: unsigned comparison of keys is the total order of the
//                 doubles, -0.0 below +0.0.
//   k_cf_scatter  one lane per particle, in the caller's order: classifies it (radius, pt_locate, the band rule on the 8 corners of
//                 its cell by pt_in_band, the LINEAR value by sp_stencil -- all of lsf_point_stencil.hpp -- read from phi itself: phi
//                 is not written until the merge, so that IS the field as it was on entry) and, for an escaped particle, offers cand = s (r - d) to
//                 the 8 corners: atomicMax on plus for s > 0, atomicMin on minus otherwise, on unsigned long long, each filtered by
//                 a plain read first (a stale value only lets a useless atomic through).  Maxima and minima of integers: the result
//                 is a function of the set of particles, not of their order.  No floating-point atomic, no CAS loop.
//   k_cf_merge    over the list or the grid: phi = fabs(plus) <= fabs(minus) ? plus : minus, stored where the bits change; the count
//                 of such points and the largest fabs(new - old) as a bit pattern, per block, then one atomicAdd and one atomicMax of
//                 integers per block that has something to report.
//
// Bounds.  A particle reaches k_cf_scatter's loads only behind pt_locate ("Bounds" of lsf_point_stencil.hpp): the 8 corners
// i0, i0 + 1 are the points whose mask and phi are read and whose keys are offered to, at 64-bit offsets below
// (nx+1)(ny+1)(nz+1), the size of both key fields.  Under a
// mask an escaped particle's 8 corners are all in the list (interior points with mask == 1), so every key it touches was set by
// k_cf_init.  A list entry is an interior point index below the number of points (lsf_band_cell.hpp).  Lanes with t >= npts, or
// e beyond the list or the grid, touch no memory.  No loop waits for another block; every loop has 8 trips.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"
#include "lsf_block_reduce.hpp"
#include "lsf_point_stencil.hpp"

namespace lsf {

constexpr int CF_BLOCK = 256;
constexpr int CF_NPART = 6; // the status counts of info

__device__ __forceinline__ unsigned long long cf_key(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double cf_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? (1ull << 63) : ~0ull)));
}

// entry e of the list L (LIST) or point e of the grid; n: entries or points
template <bool LIST>
__global__ __launch_bounds__(CF_BLOCK) void k_cf_init(const double* __restrict__ phi, const int* __restrict__ L, size_t n,
                                                      unsigned long long* __restrict__ plus, unsigned long long* __restrict__ minus)
{
    const size_t e = (size_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    if (e >= n) return;
    const size_t p = LIST ? (size_t)(unsigned)L[e] : e;
    const unsigned long long k = cf_key(phi[p]);
    plus[p] = k, minus[p] = k;
}

// Particle t of block blockIdx.x.  pts: (npts, 3) in Fortran order.  status may be NULL.  part: CF_NPART counts per block.
template <bool HAS_MASK>
__global__ __launch_bounds__(CF_BLOCK) void k_cf_scatter(SpGrid G, const double* __restrict__ pts, const double* __restrict__ rad, int npts,
                                                         double slack, unsigned long long* plus, unsigned long long* minus,
                                                         int32_t* __restrict__ status, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * CF_BLOCK + threadIdx.x, N = (size_t)npts;
    int st = -1; // no particle
    if (t < N) {
        const double ra = rad[t];
        const double x[3] = {pts[t], pts[t + N], pts[t + 2 * N]};
        int i0[3];
        double tt[3];
        if (!__builtin_isfinite(ra) || ra == 0.0)
            st = LSF_CORRECT_BADRADIUS;
        // The INSIDE test comes first: nothing below may run for a particle that fails it (see "Bounds" above).
        else if (!pt_locate<false>(x[0], G.x0, G.dx, G.nx, i0[0], tt[0]) || !pt_locate<false>(x[1], G.y0, G.dx, G.ny, i0[1], tt[1]) ||
                 !pt_locate<false>(x[2], G.z0, G.dx, G.nz, i0[2], tt[2]))
            st = LSF_CORRECT_OUTSIDE;
        else if (HAS_MASK && !pt_in_band<2>(G, i0))
            st = LSF_CORRECT_OFFBAND;
        else {
            SpSample o;
            sp_stencil<false, false>(G, nullptr, i0, tt, o);
            const double r = __builtin_fabs(ra), s = ra > 0.0 ? 1. : -1.;
            if (!__builtin_isfinite(o.v))
                st = LSF_CORRECT_NONFINITE;
            else if (s * o.v < -(slack * r)) {
                st = LSF_CORRECT_ESCAPED;
                const size_t rs = (size_t)G.nx + 1, ps = rs * ((size_t)G.ny + 1);
                const size_t base = (size_t)i0[0] + rs * (size_t)i0[1] + ps * (size_t)i0[2];
                const double lo[3] = {G.x0, G.y0, G.z0};
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int oa = c & 1, ob = (c >> 1) & 1, oc = c >> 2;
                    const double e0 = (lo[0] + (double)(i0[0] + oa) * G.dx) - x[0], e1 = (lo[1] + (double)(i0[1] + ob) * G.dx) - x[1],
                                 e2 = (lo[2] + (double)(i0[2] + oc) * G.dx) - x[2];
                    const double d = __builtin_sqrt((e0 * e0 + e1 * e1) + e2 * e2);
                    const unsigned long long key = cf_key(s * (r - d));
                    const size_t p = base + (size_t)oa + rs * (size_t)ob + ps * (size_t)oc;
                    if (ra > 0.0) {
                        if (key > plus[p]) atomicMax(plus + p, key);
                    } else {
                        if (key < minus[p]) atomicMin(minus + p, key);
                    }
                }
            } else
                st = LSF_CORRECT_INPLACE;
        }
        if (status) status[t] = st;
    }
    unsigned long long cnt[CF_NPART];
#pragma unroll
    for (int m = 0; m < CF_NPART; ++m) cnt[m] = st == m;
    block_usum_out<CF_BLOCK / 64>(cnt, (int)threadIdx.x, part + (size_t)blockIdx.x * CF_NPART);
}

// entry e of the list L (LIST) or point e of the grid.  ctl[0]: points whose bits changed; ctl[1]: the largest fabs(new - old) among
// them as a bit pattern.  Both zero before the launch.
template <bool LIST>
__global__ __launch_bounds__(CF_BLOCK) void k_cf_merge(double* __restrict__ phi, const int* __restrict__ L, size_t n,
                                                       const unsigned long long* __restrict__ plus, const unsigned long long* __restrict__ minus,
                                                       unsigned long long* __restrict__ ctl)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[CF_BLOCK / 64];
    const size_t e = (size_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    unsigned long long cnt = 0, chg = 0;
    if (e < n) {
        const size_t p = LIST ? (size_t)(unsigned)L[e] : e;
        const double old = phi[p], fp = cf_unkey(plus[p]), fm = cf_unkey(minus[p]);
        const double nw = __builtin_fabs(fp) <= __builtin_fabs(fm) ? fp : fm;
        if (__double_as_longlong(nw) != __double_as_longlong(old)) {
            phi[p] = nw;
            cnt = 1;
            chg = (unsigned long long)__double_as_longlong(__builtin_fabs(nw - old));
        }
    }
    cnt = wave_usum(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    chg = block_umax<CF_BLOCK / 64>(wave_umax_x(chg), (int)threadIdx.x); // (its barrier publishes red as well)
    if (threadIdx.x == 0) {
        cnt = lds_usum<CF_BLOCK / 64>(red, 1);
        if (cnt) {
            atomicAdd(ctl, cnt);
            atomicMax(ctl + 1, chg);
        }
    }
}

} // namespace lsf
