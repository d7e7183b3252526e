// lsf_advect_points.hpp -- points carried through the fields that move phi, x' = (u, v, w)(x) + speed(x) grad phi(x) / |grad phi(x)|,
// by TVD-RK3 or Euler in fields frozen for the call: lsf_advect_points (include/lsf.h).
//
// One lane per point, in the caller's order (k_advect_points, AP_BLOCK lanes per block, one block per AP_BLOCK consecutive points).
// The loop over the steps runs inside the kernel; the stages of a step are one loop whose body holds the one inlined sample
// (ap_rhs): pt_sample of lsf_point_stencil.hpp -- locate, the joint stencil rule, the band rule -- with ap_eval on the admitted
// stencil: sp_stencil for the value and gradient of phi with the value of speed, and pt_values3 for u, v and w under one set of
// weights, so that each component equals val of tests/sample_ref.py bit for bit.  Everything is evaluated as the header writes it,
// left to right, without contraction: the result is the numpy statement's (tests/points_ref.py) bit for bit.
//
// Bounded.  The step loop runs at most nsteps <= LSF_ADVECT_POINTS_MAX_STEPS trips of at most 3 stages; a point that fails leaves
// it.  No lane waits for another block; no value of a field, NaN included, can keep a lane.
//
// Bounds: "Bounds" of lsf_point_stencil.hpp, for every position of every stage.  u, v, w and speed are fields of the size of phi.
// Loads and stores of pts and status go to the lane's own entries t, t + npts, t + 2 npts (64-bit) of arrays of 3 npts and npts
// entries.  Lanes with t >= npts touch no memory.
//
// The report: per block the six counts of info and the bit pattern of the block's cfl (the per-lane integers through wave_usum_each,
// the cfl through wave_umax_x and block_umax, whose barrier also publishes the counts), finished by the host in block order.
// Integer sums and a maximum of bit patterns: no order of reduction reaches a result.  One plain launch, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"
#include "lsf_block_reduce.hpp"
#include "lsf_point_stencil.hpp"

namespace lsf {

constexpr int AP_BLOCK = 256;                               // points per block
constexpr int AP_NPART = LSF_ADVECT_POINTS_INFO_LEN + 1; // the counts of info, then the cfl as a bit pattern

struct ApFields {
    const double *u, *v, *w, *speed;
};

// K on an admitted stencil: LSF_POINTS_OK or LSF_POINTS_FLAT
template <bool CUBIC, bool HAS_VEL, bool HAS_SPEED>
__device__ __forceinline__ int ap_eval(const SpGrid& G, const ApFields& F, const int (&lo)[3], const double (&t)[3], double (&k)[3])
{
#pragma clang fp contract(off)
    double U[3] = {0., 0., 0.};
    if constexpr (HAS_VEL) pt_values3<CUBIC>(G, F.u, F.v, F.w, lo, t, U);
    if constexpr (HAS_SPEED) {
        SpSample s;
        sp_stencil<CUBIC, true>(G, F.speed, lo, t, s);
        const double m = (s.g0 * s.g0 + s.g1 * s.g1) + s.g2 * s.g2;
        if (m == 0.0) return LSF_POINTS_FLAT;
        const double nrm = __builtin_sqrt(m);
        if constexpr (HAS_VEL)
            k[0] = U[0] + (s.q * s.g0) / nrm, k[1] = U[1] + (s.q * s.g1) / nrm, k[2] = U[2] + (s.q * s.g2) / nrm;
        else
            k[0] = (s.q * s.g0) / nrm, k[1] = (s.q * s.g1) / nrm, k[2] = (s.q * s.g2) / nrm;
    } else
        k[0] = U[0], k[1] = U[1], k[2] = U[2];
    return LSF_POINTS_OK;
}

// One sample of the right-hand side at (x, y, z): LSF_POINTS_OK, _OUTSIDE, _OFFBAND or _FLAT; k is written on OK only, linear on OK and on FLAT.
template <bool CUBIC, bool HAS_VEL, bool HAS_SPEED, bool HAS_MASK>
__device__ __forceinline__ int ap_rhs(const SpGrid& G, const ApFields& F, double x, double y, double z, double (&k)[3], bool& linear)
{
    return pt_sample<CUBIC, HAS_MASK, false>(G, x, y, z, linear, [&](auto cubic, const int(&lo)[3], const double(&t)[3]) __attribute__((always_inline)) {
        return ap_eval<decltype(cubic)::value, HAS_VEL, HAS_SPEED>(G, F, lo, t, k);
    });
}

__device__ __forceinline__ bool ap_inside(const SpGrid& G, double x, double y, double z)
{
    int i;
    double t;
    return pt_locate<false>(x, G.x0, G.dx, G.nx, i, t) && pt_locate<false>(y, G.y0, G.dx, G.ny, i, t) && pt_locate<false>(z, G.z0, G.dx, G.nz, i, t);
}

// Point t of block blockIdx.x.  pts: (npts, 3) in Fortran order, in and out.  status may be NULL.  part: AP_NPART words per block.
template <bool CUBIC, bool HAS_VEL, bool HAS_SPEED, bool HAS_MASK>
__global__ __launch_bounds__(AP_BLOCK) void k_advect_points(SpGrid G, ApFields F, double* __restrict__ pts, int npts, int euler, double dt,
                                                            int nsteps, int32_t* __restrict__ status, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[AP_BLOCK / 64][LSF_ADVECT_POINTS_INFO_LEN];
    const size_t t = (size_t)blockIdx.x * AP_BLOCK + threadIdx.x, N = (size_t)npts;
    int st = -1; // no point
    unsigned long long ndone = 0, nfall = 0, cfl = 0;
    if (t < N) {
        double x0 = pts[t], x1 = pts[t + N], x2 = pts[t + 2 * N];
        if (!ap_inside(G, x0, x1, x2))
            st = LSF_POINTS_OUTSIDE; // returned bit for bit: nothing is stored
        else {
            st = LSF_POINTS_OK;
            const int nstage = euler ? 1 : 3;
            for (int n = 0; n < nsteps; ++n) {
                double y0 = x0, y1 = x1, y2 = x2;
                unsigned long long c = 0; // the step's largest fabs(dt * k_A) / dx, as a bit pattern
                int why = LSF_POINTS_OK;
#pragma unroll 1
                for (int sg = 0; sg < nstage; ++sg) {
                    double k[3];
                    bool lin = false;
                    why = ap_rhs<CUBIC, HAS_VEL, HAS_SPEED, HAS_MASK>(G, F, y0, y1, y2, k, lin);
                    if (why != LSF_POINTS_OK) break;
                    if (CUBIC && lin) ++nfall;
                    const double d0 = dt * k[0], d1 = dt * k[1], d2 = dt * k[2];
                    const unsigned long long c0 = (unsigned long long)__double_as_longlong(__builtin_fabs(d0) / G.dx),
                                             c1 = (unsigned long long)__double_as_longlong(__builtin_fabs(d1) / G.dx),
                                             c2 = (unsigned long long)__double_as_longlong(__builtin_fabs(d2) / G.dx);
                    c = c0 > c ? c0 : c, c = c1 > c ? c1 : c, c = c2 > c ? c2 : c;
                    if (sg == 0)
                        y0 = x0 + d0, y1 = x1 + d1, y2 = x2 + d2;
                    else if (sg == 1)
                        y0 = 0.75 * x0 + 0.25 * (y0 + d0), y1 = 0.75 * x1 + 0.25 * (y1 + d1), y2 = 0.75 * x2 + 0.25 * (y2 + d2);
                    else
                        y0 = (1. / 3.) * x0 + (2. / 3.) * (y0 + d0), y1 = (1. / 3.) * x1 + (2. / 3.) * (y1 + d1),
                        y2 = (1. / 3.) * x2 + (2. / 3.) * (y2 + d2);
                }
                if (why == LSF_POINTS_OK && !ap_inside(G, y0, y1, y2)) why = LSF_POINTS_OUTSIDE;
                if (why != LSF_POINTS_OK) { // the point keeps the position of its last completed step
                    st = why;
                    break;
                }
                x0 = y0, x1 = y1, x2 = y2;
                ++ndone;
                cfl = c > cfl ? c : cfl;
            }
            if (ndone) pts[t] = x0, pts[t + N] = x1, pts[t + 2 * N] = x2;
        }
        if (status) status[t] = st;
    }
    unsigned long long n0 = st == LSF_POINTS_OK, n1 = st == LSF_POINTS_OUTSIDE, n2 = st == LSF_POINTS_OFFBAND, n3 = st == LSF_POINTS_FLAT;
    wave_usum_each(n0, n1, n2, n3, ndone, nfall);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* r = red[threadIdx.x >> 6];
        r[0] = n0, r[1] = n1, r[2] = n2, r[3] = n3, r[4] = ndone, r[5] = nfall;
    }
    cfl = block_umax<AP_BLOCK / 64>(wave_umax_x(cfl), (int)threadIdx.x); // (its barrier publishes red as well)
    if (threadIdx.x == 0) {
        unsigned long long* o = part + (size_t)blockIdx.x * AP_NPART;
        for (int m = 0; m < LSF_ADVECT_POINTS_INFO_LEN; ++m) o[m] = lds_usum<AP_BLOCK / 64>(&red[0][m], LSF_ADVECT_POINTS_INFO_LEN);
        o[LSF_ADVECT_POINTS_INFO_LEN] = cfl;
    }
}

} // namespace lsf
