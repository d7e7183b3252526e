// lsf_cast_rays.hpp -- the first hit of a ray with phi = iso, band-aware: lsf_cast_rays (include/lsf.h).
//
// One lane per ray, in the caller's order (k_cast_rays, CR_BLOCK lanes per block, one block per CR_BLOCK consecutive rays).  A lane
// normalises its direction, clips the ray to the grid box by slabs and then runs ONE loop that holds both the march and the
// bisections: each trip takes one ray sample -- sp_sample<.., RAY> of lsf_point_stencil.hpp: the locate step with the header's
// tolerance, the band rule, the values -- at the lane's current t and then either marches (a step off the last on-list value, a
// stride of skip*dx off the list) or halves its bracket.  The sample body is inlined once, at the head of that loop, so lanes of a
// wave that are in different phases still share its gathers; a lane that has finished waits at the loop's end for the longest ray of
// its wave.  The secant step and the one full sample at the hit (the only place q is read) follow the loop, where the wave has
// converged again.  Everything is evaluated as the header writes it, left to right, without contraction, so the result is the
// numpy statement's (tests/cast_ref.py) bit for bit.
//
// Bounded.  The loop runs at most (max_steps + 1) + refine trips: a marching trip that does not end the ray counts one step and the
// trip after the max_steps-th ends it with LSF_CAST_STEPS; a ray bisects exactly `refine` times.  The trip count is the loop's own
// bound as well, so no value of phi, NaN included, and no ray can keep a lane.  No lane waits for another block.
//
// Bounds: "Bounds" of lsf_point_stencil.hpp, in its ray form.  NaN, +-inf and 1e300 never get that far: such a ray is LSF_CAST_BAD
// before it is clipped.  Stores go to the lane's own entries r, r + nrays, r + 2 nrays (64-bit) of arrays of nrays and 3 nrays
// entries.  Lanes with r >= nrays touch no memory.
//
// The report: per block the nine counts of info (wave ballots and wave_usum, then block_usum_out of lsf_block_reduce.hpp), finished by the host in block order.
// Integer counts: no order of reduction reaches a result.  One plain launch: no atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"
#include "lsf_block_reduce.hpp"
#include "lsf_point_stencil.hpp"

namespace lsf {

constexpr int CR_BLOCK = 256; // rays per block
constexpr int CR_NPART = LSF_CAST_INFO_LEN;

struct CrParams {
    double iso, tmin, tmax, safety;
    double smin_dx, smax_dx, skip_dx; // smin * dx, smax * dx, skip * dx, computed once on the host
    int refine, max_steps;
};

// One axis of the header's clip.  false: the ray runs along the slab and outside it.
__device__ __forceinline__ bool cr_slab(double o, double u, double lo, double dx, int n, double& t0, double& t1)
{
#pragma clang fp contract(off)
    const double hi = lo + (double)n * dx;
    if (u == 0.0) return o >= lo && o <= hi;
    const double a = (lo - o) / u, b = (hi - o) / u;
    t0 = cr_fmax(t0, cr_fmin(a, b));
    t1 = cr_fmin(t1, cr_fmax(a, b));
    return true;
}

__device__ __forceinline__ bool cr_crossing(double e, double er) { return e == 0.0 || ((e > 0.0) != (er > 0.0)); }

// Ray r of block blockIdx.x.  org, dir, hit, grad: (nrays, 3) in Fortran order.  hit, grad, qval (HAS_Q) and status may be NULL.
// part: CR_NPART counts per block.
template <bool CUBIC, bool HAS_MASK, bool HAS_Q>
__global__ __launch_bounds__(CR_BLOCK) void k_cast_rays(SpGrid G, const double* __restrict__ q, const double* __restrict__ org,
                                                        const double* __restrict__ dir, int nrays, CrParams P, double* __restrict__ thit,
                                                        double* __restrict__ hit, double* __restrict__ grad, double* __restrict__ qval,
                                                        int32_t* __restrict__ status, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    const size_t r = (size_t)blockIdx.x * CR_BLOCK + threadIdx.x, N = (size_t)nrays;
    const double nan = __builtin_nan("");
    int st = -1;                       // no ray, or not decided yet
    unsigned long long ns = 0, nk = 0; // samples of phi taken, off-list strides
    bool inner = false, found = false; // e < 0 at the first reference; the bracket [tr, tb] holds the hit
    double o0 = 0, o1 = 0, o2 = 0, u0 = 0, u1 = 0, u2 = 0;
    double th = nan, tr = 0, er = 0, tb = 0, eb = 0;
    if (r < N) {
        o0 = org[r], o1 = org[r + N], o2 = org[r + 2 * N];
        const double d0 = dir[r], d1 = dir[r + N], d2 = dir[r + 2 * N];
        const double L = __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        double t0 = P.tmin, t1 = P.tmax;
        if (!(__builtin_isfinite(o0) && __builtin_isfinite(o1) && __builtin_isfinite(o2) && __builtin_isfinite(d0) && __builtin_isfinite(d1) &&
              __builtin_isfinite(d2)) ||
            !(L > 0.0) || !__builtin_isfinite(L))
            st = LSF_CAST_BAD;
        else {
            u0 = d0 / L, u1 = d1 / L, u2 = d2 / L;
            if (!cr_slab(o0, u0, G.x0, G.dx, G.nx, t0, t1) || !cr_slab(o1, u1, G.y0, G.dx, G.ny, t0, t1) ||
                !cr_slab(o2, u2, G.z0, G.dx, G.nz, t0, t1) || !(t0 <= t1))
                st = LSF_CAST_NOGRID;
        }
        if (st < 0) {
            double t = t0;
            bool have = false, gap = false, last = false, refining = false;
            int k = 0, left = P.refine; // marching steps made, bisections left
            const long trips = (long)P.max_steps + 1 + (long)P.refine;
            for (long it = 0; it < trips; ++it) {
                SpSample s;
                const int c = sp_sample<CUBIC, false, HAS_MASK, true>(G, nullptr, o0 + t * u0, o1 + t * u1, o2 + t * u2, s);
                const bool on = c == LSF_SAMPLE_OK;
                if (on) ++ns;
                const double e = on ? s.v - P.iso : 0.0;
                if (refining) {
                    if (!on) {
                        st = LSF_CAST_LOST;
                        break;
                    }
                    if (cr_crossing(e, er))
                        tb = t, eb = e;
                    else
                        tr = t, er = e;
                    if (--left == 0) {
                        found = true;
                        break;
                    }
                    t = 0.5 * (tr + tb);
                    continue;
                }
                if (c == LSF_SAMPLE_OUTSIDE) {
                    st = LSF_CAST_MISS, th = t;
                    break;
                }
                double step;
                if (HAS_MASK && !on) { // off the list: nothing of phi was read
                    gap = true, ++nk;
                    step = P.skip_dx;
                } else {
                    if (!have) {
                        have = true, inner = e < 0.0;
                        tr = t, er = e, gap = false;
                        if (e == 0.0) { // a hit at this very t: the bracket is [t, t]
                            tb = t, eb = e, found = true;
                            break;
                        }
                    } else if (cr_crossing(e, er)) {
                        if (gap) {
                            st = LSF_CAST_LOST;
                            break;
                        }
                        tb = t, eb = e;
                        if (left == 0) {
                            found = true;
                            break;
                        }
                        refining = true;
                        t = 0.5 * (tr + tb);
                        continue;
                    } else
                        tr = t, er = e, gap = false;
                    step = cr_fmin(cr_fmax(P.safety * __builtin_fabs(er), P.smin_dx), P.smax_dx);
                }
                if (last) {
                    st = LSF_CAST_MISS, th = t;
                    break;
                }
                if (k == P.max_steps) {
                    st = LSF_CAST_STEPS;
                    break;
                }
                ++k;
                t = t + step;
                if (!(t < t1)) t = t1, last = true;
            }
            if (st < 0 && !found) st = LSF_CAST_STEPS; // (the trips cannot run out first: see "Bounded" above)
        }
    }
    // the secant step and the full sample at the hit, with q: outside the loop, where the wave is together again
    double h0 = nan, h1 = nan, h2 = nan, g0 = nan, g1 = nan, g2 = nan, qv = nan;
    if (found) {
        const double quo = (er * (tb - tr)) / (eb - er);
        th = (eb != er && __builtin_isfinite(quo)) ? tr - quo : tr;
        th = cr_fmin(cr_fmax(th, tr), tb);
        const double p0 = o0 + th * u0, p1 = o1 + th * u1, p2 = o2 + th * u2;
        SpSample s;
        if (sp_sample<CUBIC, HAS_Q, HAS_MASK, true>(G, q, p0, p1, p2, s) == LSF_SAMPLE_OK) {
            ++ns;
            st = LSF_CAST_HIT;
            h0 = p0, h1 = p1, h2 = p2, g0 = s.g0, g1 = s.g1, g2 = s.g2;
            if constexpr (HAS_Q) qv = s.q;
        } else
            st = LSF_CAST_LOST;
    }
    if (r < N) {
        thit[r] = (st == LSF_CAST_HIT || st == LSF_CAST_MISS) ? th : nan;
        if (hit) hit[r] = h0, hit[r + N] = h1, hit[r + 2 * N] = h2;
        if (grad) grad[r] = g0, grad[r + N] = g1, grad[r + 2 * N] = g2;
        if constexpr (HAS_Q)
            if (qval) qval[r] = qv;
        if (status) status[r] = st;
    }
    unsigned long long cnt[CR_NPART] = {wave_count(st == LSF_CAST_HIT),  wave_count(st == LSF_CAST_MISS), wave_count(st == LSF_CAST_NOGRID),
                                        wave_count(st == LSF_CAST_BAD),  wave_count(st == LSF_CAST_LOST), wave_count(st == LSF_CAST_STEPS),
                                        wave_usum(ns),                   wave_usum(nk),                   wave_count(inner)};
    block_usum_out<CR_BLOCK / 64, true>(cnt, (int)threadIdx.x, part + (size_t)blockIdx.x * CR_NPART);
}

} // namespace lsf
