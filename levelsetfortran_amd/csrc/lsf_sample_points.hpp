// lsf_sample_points.hpp -- the field, its gradient, a second field and the foot point on phi = iso at arbitrary points:
// lsf_sample_points (include/lsf.h).
//
// A pure gather: one lane per point, in the caller's order (k_sample_points, SP_BLOCK lanes per block, one block per SP_BLOCK
// consecutive points; the grid never needs a stride because npts is an int).  A lane samples its point with sp_sample of
// lsf_point_stencil.hpp -- locate, the joint stencil rule, the band rule, the 2 x 2 x 2 or 4 x 4 x 4 values gathered through L1/L2 and
// contracted as they arrive -- and the projection (pt_foot) repeats the same sample at the moved point.  Everything is evaluated as
// the header writes it, left to right, without contraction, so the result is the numpy statement's (tests/sample_ref.py) bit for bit.
//
// Bounds: "Bounds" of lsf_point_stencil.hpp, for the caller's point and for the moved point of every projection step.  Stores go to
// the lane's own entries t, t + npts, t + 2 npts (64-bit) of arrays of npts and 3 npts entries.  Lanes with t >= npts touch no memory.
//
// The report: per block the six counts of info (wave ballots, then block_usum_out of lsf_block_reduce.hpp), finished by the host in block order.
// Integer counts: no order of reduction reaches a result.  One plain launch: no atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"
#include "lsf_block_reduce.hpp"
#include "lsf_point_stencil.hpp"

namespace lsf {

constexpr int SP_BLOCK = 256; // points per block
constexpr int SP_NPART = LSF_SAMPLE_INFO_LEN;

// Point t of block blockIdx.x.  pts, grad, foot: (npts, 3) in Fortran order.  grad, qval (HAS_Q), foot (PROJECT) and status may be
// NULL.  tol_dx = tol * dx, computed once on the host.  part: SP_NPART counts per block.
template <bool CUBIC, bool HAS_Q, bool HAS_MASK, bool PROJECT>
__global__ __launch_bounds__(SP_BLOCK) void k_sample_points(SpGrid G, const double* __restrict__ q, const double* __restrict__ pts, int npts,
                                                            double iso, int iters, double tol_dx, double* __restrict__ val,
                                                            double* __restrict__ grad, double* __restrict__ qval, double* __restrict__ foot,
                                                            int32_t* __restrict__ status, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * SP_BLOCK + threadIdx.x, N = (size_t)npts;
    int st = -1; // no point
    bool fallback = false;
    if (t < N) {
        const double nan = __builtin_nan("");
        const double x0 = pts[t], x1 = pts[t + N], x2 = pts[t + 2 * N];
        SpSample s;
        st = sp_sample<CUBIC, HAS_Q, HAS_MASK>(G, q, x0, x1, x2, s);
        const bool own = st == LSF_SAMPLE_OK;
        fallback = CUBIC && own && s.linear;
        val[t] = own ? s.v : nan;
        if (grad) grad[t] = own ? s.g0 : nan, grad[t + N] = own ? s.g1 : nan, grad[t + 2 * N] = own ? s.g2 : nan;
        if constexpr (HAS_Q)
            if (qval) qval[t] = own ? s.q : nan;
        if constexpr (PROJECT) {
            double y0 = x0, y1 = x1, y2 = x2;
            if (own) // s is the sample at y = x, the first of the iteration
                st = pt_foot<CUBIC, HAS_MASK>(G, iso, iters, tol_dx, s, y0, y1, y2);
            else
                y0 = y1 = y2 = nan;
            if (foot) foot[t] = y0, foot[t + N] = y1, foot[t + 2 * N] = y2;
        }
        if (status) status[t] = st;
    }
    unsigned long long cnt[SP_NPART] = {wave_count(st == LSF_SAMPLE_OK),   wave_count(st == LSF_SAMPLE_OUTSIDE), wave_count(st == LSF_SAMPLE_OFFBAND),
                                        wave_count(fallback),              wave_count(st == LSF_SAMPLE_FLAT),    wave_count(st == LSF_SAMPLE_NOT_CONVERGED)};
    block_usum_out<SP_BLOCK / 64, true>(cnt, (int)threadIdx.x, part + (size_t)blockIdx.x * SP_NPART);
}

} // namespace lsf
