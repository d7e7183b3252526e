// lsf_cast_rays.hpp -- the first hit of a ray with phi = iso, band-aware: lsf_cast_rays (include/lsf.h).
//
// One lane per ray, in the caller's order (k_cast_rays, CR_BLOCK lanes per block, one block per CR_BLOCK consecutive rays).  A lane
// normalises its direction, clips the ray to the grid box by slabs and then runs ONE loop that holds both the march and the
// bisections: each trip takes one ray sample -- cr_sample: the locate step of the header with its tolerance, the band rule with its
// loads side by side (cr_in_band) and sp_stencil of lsf_sample_points.hpp, unchanged, for the values -- at the lane's current t and
// then either marches (a step off the last on-list value, a stride of skip*dx off the list) or halves its bracket.  The sample body
// is inlined once, at the head of that loop, so lanes of a wave that are in different phases still share its gathers; a lane that
// has finished waits at the loop's end for the longest ray of its wave.  The secant step and the one full sample at the hit (the only place q is read) follow the loop, where the wave has
// converged again.  Everything is evaluated as the header writes it, left to right, without contraction, so the result is the
// numpy statement's (tests/cast_ref.py) bit for bit.
//
// Bounded.  The loop runs at most (max_steps + 1) + refine trips: a marching trip that does not end the ray counts one step and the
// trip after the max_steps-th ends it with LSF_CAST_STEPS; a ray bisects exactly `refine` times.  The trip count is the loop's own
// bound as well, so no value of phi, NaN included, and no ray can keep a lane.  No lane waits for another block.
//
// Bounds.  The test of cr_locate, made in double BEFORE any conversion to an integer, is the only thing between a wild ray and an
// out-of-bounds load: it admits -1e-6 <= s <= n + 1e-6 and s is clamped into [0, n] behind it, so 0 <= i0 <= n - 1 as in
// lsf_sample_points and sp_stencil's own argument holds (corners i0, i0 + 1 in 0..n; cubic only where 1 <= i0 <= n - 2).  NaN, +-inf
// and 1e300 never get that far: such a ray is LSF_CAST_BAD before it is clipped.  Stores go to the lane's own entries r, r + nrays,
// r + 2 nrays (64-bit) of arrays of nrays and 3 nrays entries.  Lanes with r >= nrays touch no memory.
//
// The report: per block the nine counts of info (wave ballots for the statuses, wave sums by shuffles for the samples and strides,
// the four waves added by lane 0), finished by the host in block order.  Integer counts: no order of reduction reaches a result.
// One plain launch: no atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"
#include "lsf_sample_points.hpp"

namespace lsf {

constexpr int CR_BLOCK = 256; // rays per block
constexpr int CR_NPART = LSF_CAST_INFO_LEN;

struct CrParams {
    double iso, tmin, tmax, safety;
    double smin_dx, smax_dx, skip_dx; // smin * dx, smax * dx, skip * dx, computed once on the host
    int refine, max_steps;
};

// the header's fmax / fmin: b where a is NaN, else a where b is NaN or a >= b (a <= b), else b -- the first argument on a tie
__device__ __forceinline__ double cr_fmax(double a, double b) { return a != a ? b : ((b != b || a >= b) ? a : b); }
__device__ __forceinline__ double cr_fmin(double a, double b) { return a != a ? b : ((b != b || a <= b) ? a : b); }

// One axis of the header's ray sample.  false: refused, and then i0 and t mean nothing and must not be used.
__device__ __forceinline__ bool cr_locate(double x, double lo, double dx, int n, int& i0, double& t)
{
#pragma clang fp contract(off)
    double s = (x - lo) / dx;
    // in double, before any integer exists: NaN fails both comparisons, +-inf and 1e300 one of them
    if (!(s >= -1e-6 && s <= (double)n + 1e-6)) return false;
    s = cr_fmin(cr_fmax(s, 0.), (double)n);
    const int f = (int)__builtin_floor(s); // 0 <= s <= n <= 2^31 - 2: the conversion is exact
    i0 = f < n - 1 ? f : n - 1;            // the upper wall belongs to the last cell with t = 1
    t = s - (double)i0;
    return true;
}

// The band rule of sp_stencil for the K^3 stencil whose lowest point is lo -- every point an interior point (1..n-1 on each axis)
// with mask == 1 -- with the mask values read side by side.  sp_stencil's own test leaves at the first value that is not 1, which the
// compiler can only build as a chain of K^3 load - wait - branch steps: a march takes that test at every sample, and an on-list
// cubic sample would wait for 64 memory latencies in a row.  Here the loads carry no branch: every stencil point exists whatever the
// mask holds (cr_locate), so all of them may be issued before the first arrives.  The 2 x 2 x 2 corners of the cell come first and
// decide alone for most off-list strides (one latency, 8 loads); the other 56 values of a cubic stencil follow in one more.
template <int K>
__device__ __forceinline__ bool cr_in_band(const SpGrid& G, const int (&lo)[3])
{
    if (!(lo[0] >= 1 && lo[0] + K - 1 <= G.nx - 1 && lo[1] >= 1 && lo[1] + K - 1 <= G.ny - 1 && lo[2] >= 1 && lo[2] + K - 1 <= G.nz - 1)) return false;
    const long rs = (long)G.nx + 1, ps = rs * ((long)G.ny + 1);
    const int32_t* __restrict__ m = G.mask + ((long)lo[0] + rs * (long)lo[1] + ps * (long)lo[2]);
    constexpr int C = K == 4 ? 1 : 0; // where the cell's corners sit in the stencil
    int in = 1;
#pragma unroll
    for (int c = C; c < C + 2; ++c)
#pragma unroll
        for (int b = C; b < C + 2; ++b)
#pragma unroll
            for (int a = C; a < C + 2; ++a) in &= m[a + rs * b + ps * c] == 1;
    if constexpr (K == 4) {
        if (!in) return false;
#pragma unroll
        for (int c = 0; c < K; ++c)
#pragma unroll
            for (int b = 0; b < K; ++b)
#pragma unroll
                for (int a = 0; a < K; ++a)
                    if (a < C || a >= C + 2 || b < C || b >= C + 2 || c < C || c >= C + 2) in &= m[a + rs * b + ps * c] == 1;
    }
    return in != 0;
}

// One ray sample: LSF_SAMPLE_OK, _OUTSIDE or _OFFBAND; o is written on OK only.  sp_sample with cr_locate in front and the band test
// by cr_in_band: sp_stencil itself is instantiated without a mask and computes the values.
template <bool CUBIC, bool HAS_Q, bool HAS_MASK>
__device__ __forceinline__ int cr_sample(const SpGrid& G, const double* __restrict__ q, double x, double y, double z, SpSample& o)
{
    int i0[3];
    double t[3];
    // The test comes first: nothing below may run for a point that fails it (see "Bounds" above).
    if (!cr_locate(x, G.x0, G.dx, G.nx, i0[0], t[0]) || !cr_locate(y, G.y0, G.dx, G.ny, i0[1], t[1]) ||
        !cr_locate(z, G.z0, G.dx, G.nz, i0[2], t[2]))
        return LSF_SAMPLE_OUTSIDE;
    if constexpr (CUBIC) {
        if (i0[0] >= 1 && i0[0] <= G.nx - 2 && i0[1] >= 1 && i0[1] <= G.ny - 2 && i0[2] >= 1 && i0[2] <= G.nz - 2) {
            const int lo[3] = {i0[0] - 1, i0[1] - 1, i0[2] - 1};
            if constexpr (HAS_MASK)
                if (!cr_in_band<4>(G, lo)) return LSF_SAMPLE_OFFBAND;
            sp_stencil<true, HAS_Q, false>(G, q, lo, t, o);
            return LSF_SAMPLE_OK;
        }
    }
    if constexpr (HAS_MASK)
        if (!cr_in_band<2>(G, i0)) return LSF_SAMPLE_OFFBAND;
    sp_stencil<false, HAS_Q, false>(G, q, i0, t, o);
    return LSF_SAMPLE_OK;
}

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

__device__ __forceinline__ unsigned long long cr_wave_sum(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, d), hi = __shfl_xor((unsigned)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// Ray r of block blockIdx.x.  org, dir, hit, grad: (nrays, 3) in Fortran order.  hit, grad, qval (HAS_Q) and status may be NULL.
// part: CR_NPART counts per block.
template <bool CUBIC, bool HAS_MASK, bool HAS_Q>
__global__ __launch_bounds__(CR_BLOCK) void k_cast_rays(SpGrid G, const double* __restrict__ q, const double* __restrict__ org,
                                                        const double* __restrict__ dir, int nrays, CrParams P, double* __restrict__ thit,
                                                        double* __restrict__ hit, double* __restrict__ grad, double* __restrict__ qval,
                                                        int32_t* __restrict__ status, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[CR_BLOCK / 64][CR_NPART];
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
                // the ray's point passes the test of cr_sample before anything is loaded for it
                const int c = cr_sample<CUBIC, false, HAS_MASK>(G, nullptr, o0 + t * u0, o1 + t * u1, o2 + t * u2, s);
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
        if (cr_sample<CUBIC, HAS_Q, HAS_MASK>(G, q, p0, p1, p2, s) == LSF_SAMPLE_OK) {
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
    unsigned long long cnt[CR_NPART];
    cnt[0] = __popcll(__ballot(st == LSF_CAST_HIT));
    cnt[1] = __popcll(__ballot(st == LSF_CAST_MISS));
    cnt[2] = __popcll(__ballot(st == LSF_CAST_NOGRID));
    cnt[3] = __popcll(__ballot(st == LSF_CAST_BAD));
    cnt[4] = __popcll(__ballot(st == LSF_CAST_LOST));
    cnt[5] = __popcll(__ballot(st == LSF_CAST_STEPS));
    cnt[6] = cr_wave_sum(ns);
    cnt[7] = cr_wave_sum(nk);
    cnt[8] = __popcll(__ballot(inner));
    if ((threadIdx.x & 63) == 0)
        for (int m = 0; m < CR_NPART; ++m) red[threadIdx.x >> 6][m] = cnt[m];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* o = part + (size_t)blockIdx.x * CR_NPART;
        for (int m = 0; m < CR_NPART; ++m) {
            unsigned long long s = red[0][m];
            for (int w = 1; w < CR_BLOCK / 64; ++w) s += red[w][m];
            o[m] = s;
        }
    }
}

} // namespace lsf
