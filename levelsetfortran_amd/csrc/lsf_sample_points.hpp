// lsf_sample_points.hpp -- the field, its gradient, a second field and the foot point on phi = iso at arbitrary points:
// lsf_sample_points (include/lsf.h).
//
// A pure gather: one lane per point, in the caller's order (k_sample_points, SP_BLOCK lanes per block, one block per SP_BLOCK
// consecutive points; the grid never needs a stride because npts is an int).  A lane locates its point, picks the stencil by the joint
// rule of the header, checks the band, gathers the 2 x 2 x 2 or 4 x 4 x 4 values through L1/L2 and contracts them as they arrive: a
// row of 4 along x becomes one value (and one x-derivative), the 4 rows of a plane become three numbers (value, d/dx, d/dy), the 4
// planes become the value and the three derivatives.  At most 4 + 4 row results and 4 + 4 + 4 plane results are live; the 64 values
// never are.  Everything is evaluated as the header writes it, left to right, without contraction, so the result is the numpy
// statement's (tests/sample_ref.py) bit for bit.  The projection repeats the same sample at the moved point.
//
// Bounds.  The INSIDE test of sp_locate, made in double BEFORE any conversion to an integer, is the only thing between a wild
// coordinate (NaN, +-inf, 1e300, a point of another mesh) and an out-of-bounds load: a point that fails it returns before an index
// exists.  It comes first for the caller's point and for the moved point of every projection step.  Behind it 0 <= s <= n, so
// 0 <= i0 <= n - 1 after the min and the corners i0, i0 + 1 lie in 0..n; the cubic stencil is taken only where 1 <= i0 <= n - 2, so
// i0 - 1 >= 0 and i0 + 2 <= n.  The host refuses fields beyond 2^31 - 1 points; offsets are formed in 64 bits all the same.  Stores
// go to the lane's own entries t, t + npts, t + 2 npts (64-bit) of arrays of npts and 3 npts entries.  Lanes with t >= npts touch no
// memory.
//
// The report: per block the six counts of info (wave ballots, the four waves added by lane 0), finished by the host in block order.
// Integer counts: no order of reduction reaches a result.  One plain launch: no atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"

namespace lsf {

constexpr int SP_BLOCK = 256; // points per block
constexpr int SP_NPART = LSF_SAMPLE_INFO_LEN;

struct SpGrid {
    const double* phi;
    const int32_t* mask;
    int nx, ny, nz;
    double dx, x0, y0, z0;
};

struct SpSample {
    double v, g0, g1, g2, q;
    bool linear; // the 2 x 2 x 2 stencil was used
};

// One axis of the header's "Locate".  false: not INSIDE, and then i0 and t mean nothing and must not be used.
__device__ __forceinline__ bool sp_locate(double x, double lo, double dx, int n, int& i0, double& t)
{
#pragma clang fp contract(off)
    const double s = (x - lo) / dx;
    // in double, before any integer exists: NaN fails both comparisons, +-inf and 1e300 one of them
    if (!(s >= 0.0 && s <= (double)n)) return false;
    const int f = (int)__builtin_floor(s); // 0 <= s <= n <= 2^31 - 2: the conversion is exact
    i0 = f < n - 1 ? f : n - 1;            // the upper wall belongs to the last cell with t = 1
    t = s - (double)i0;
    return true;
}

template <bool CUBIC>
__device__ __forceinline__ void sp_weights(double t, double (&w)[CUBIC ? 4 : 2], double (&d)[CUBIC ? 4 : 2])
{
#pragma clang fp contract(off)
    if constexpr (CUBIC) {
        w[0] = 0.5 * (((2. - t) * t - 1.) * t);
        w[1] = 0.5 * ((3. * t - 5.) * t * t + 2.);
        w[2] = 0.5 * (((4. - 3. * t) * t + 1.) * t);
        w[3] = 0.5 * ((t - 1.) * t * t);
        d[0] = 0.5 * ((4. - 3. * t) * t - 1.);
        d[1] = 0.5 * ((9. * t - 10.) * t);
        d[2] = 0.5 * ((8. - 9. * t) * t + 1.);
        d[3] = 0.5 * ((3. * t - 2.) * t);
    } else {
        w[0] = 1. - t, w[1] = t;
        d[0] = -1., d[1] = 1.;
    }
}

template <int K>
__device__ __forceinline__ double sp_dot(const double (&w)[K], const double (&a)[K])
{
#pragma clang fp contract(off)
    double r = w[0] * a[0] + w[1] * a[1];
    if constexpr (K == 4) {
        r = r + w[2] * a[2];
        r = r + w[3] * a[3];
    }
    return r;
}

// The K^3 stencil whose lowest point is `base` (a 64-bit point index): band test, then value and gradient of phi and the value of q.
// Returns false for OFFBAND (nothing computed).  lo[A] is the lowest stencil index on axis A (for the interior rule of the band).
template <bool CUBIC, bool HAS_Q, bool HAS_MASK>
__device__ __forceinline__ bool sp_stencil(const SpGrid& G, const double* __restrict__ q, const int (&lo)[3], const double (&t)[3], SpSample& o)
{
#pragma clang fp contract(off)
    constexpr int K = CUBIC ? 4 : 2;
    const long rs = (long)G.nx + 1, ps = rs * ((long)G.ny + 1);
    const long base = (long)lo[0] + rs * (long)lo[1] + ps * (long)lo[2];
    if constexpr (HAS_MASK) {
        // IN: an interior point (1..n-1 on each axis) with mask == 1 -- the LIST rule of lsf_reinit_band
        bool in = lo[0] >= 1 && lo[0] + K - 1 <= G.nx - 1 && lo[1] >= 1 && lo[1] + K - 1 <= G.ny - 1 && lo[2] >= 1 && lo[2] + K - 1 <= G.nz - 1;
        const int32_t* __restrict__ m = G.mask + base;
#pragma unroll
        for (int c = 0; c < K; ++c)
#pragma unroll
            for (int b = 0; b < K; ++b)
#pragma unroll
                for (int a = 0; a < K; ++a) in = in && m[a + rs * b + ps * c] == 1;
        if (!in) return false;
    }
    double wx[K], dx_[K], wy[K], dy_[K], wz[K], dz_[K];
    sp_weights<CUBIC>(t[0], wx, dx_);
    sp_weights<CUBIC>(t[1], wy, dy_);
    sp_weights<CUBIC>(t[2], wz, dz_);
    const double* __restrict__ f = G.phi + base;
    double p[K], px[K], py[K], pq[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double r[K], rd[K], rq[K];
#pragma unroll
        for (int b = 0; b < K; ++b) {
            double a[K];
#pragma unroll
            for (int i = 0; i < K; ++i) a[i] = f[i + rs * b + ps * c];
            r[b] = sp_dot<K>(wx, a);
            rd[b] = sp_dot<K>(dx_, a);
            if constexpr (HAS_Q) {
                double aq[K];
#pragma unroll
                for (int i = 0; i < K; ++i) aq[i] = q[base + i + rs * b + ps * c];
                rq[b] = sp_dot<K>(wx, aq);
            }
        }
        p[c] = sp_dot<K>(wy, r);
        px[c] = sp_dot<K>(wy, rd);
        py[c] = sp_dot<K>(dy_, r);
        if constexpr (HAS_Q) pq[c] = sp_dot<K>(wy, rq);
    }
    o.v = sp_dot<K>(wz, p);
    o.g0 = sp_dot<K>(wz, px) / G.dx;
    o.g1 = sp_dot<K>(wz, py) / G.dx;
    o.g2 = sp_dot<K>(dz_, p) / G.dx;
    if constexpr (HAS_Q) o.q = sp_dot<K>(wz, pq);
    o.linear = !CUBIC;
    return true;
}

// One sample by the rules of the header: LSF_SAMPLE_OK, _OUTSIDE or _OFFBAND; o is written on OK only.
template <bool CUBIC, bool HAS_Q, bool HAS_MASK>
__device__ __forceinline__ int sp_sample(const SpGrid& G, const double* __restrict__ q, double x, double y, double z, SpSample& o)
{
    int i0[3];
    double t[3];
    // The INSIDE test comes first: nothing below may run for a point that fails it (see "Bounds" above).
    if (!sp_locate(x, G.x0, G.dx, G.nx, i0[0], t[0]) || !sp_locate(y, G.y0, G.dx, G.ny, i0[1], t[1]) ||
        !sp_locate(z, G.z0, G.dx, G.nz, i0[2], t[2]))
        return LSF_SAMPLE_OUTSIDE;
    if constexpr (CUBIC) {
        // the joint rule: cubic only where 1 <= i0 <= n - 2 on all three axes, so that i0 - 1 >= 0 and i0 + 2 <= n
        if (i0[0] >= 1 && i0[0] <= G.nx - 2 && i0[1] >= 1 && i0[1] <= G.ny - 2 && i0[2] >= 1 && i0[2] <= G.nz - 2) {
            const int lo[3] = {i0[0] - 1, i0[1] - 1, i0[2] - 1};
            return sp_stencil<true, HAS_Q, HAS_MASK>(G, q, lo, t, o) ? LSF_SAMPLE_OK : LSF_SAMPLE_OFFBAND;
        }
    }
    return sp_stencil<false, HAS_Q, HAS_MASK>(G, q, i0, t, o) ? LSF_SAMPLE_OK : LSF_SAMPLE_OFFBAND;
}

// Point t of block blockIdx.x.  pts, grad, foot: (npts, 3) in Fortran order.  grad, qval (HAS_Q), foot (PROJECT) and status may be
// NULL.  tol_dx = tol * dx, computed once on the host.  part: SP_NPART counts per block.
template <bool CUBIC, bool HAS_Q, bool HAS_MASK, bool PROJECT>
__global__ __launch_bounds__(SP_BLOCK) void k_sample_points(SpGrid G, const double* __restrict__ q, const double* __restrict__ pts, int npts,
                                                            double iso, int iters, double tol_dx, double* __restrict__ val,
                                                            double* __restrict__ grad, double* __restrict__ qval, double* __restrict__ foot,
                                                            int32_t* __restrict__ status, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[SP_BLOCK / 64][SP_NPART];
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
            if (own) {
                // s is the sample at y = x, the first of the loop.  `iters` moves, and one more sample for the test after the last.
                st = LSF_SAMPLE_NOT_CONVERGED;
                for (int it = 0;; ++it) {
                    const double e = s.v - iso;
                    if (!(__builtin_fabs(e) > tol_dx)) {
                        st = LSF_SAMPLE_OK;
                        break;
                    }
                    if (it == iters) break;
                    const double m = (s.g0 * s.g0 + s.g1 * s.g1) + s.g2 * s.g2;
                    if (m == 0.0) {
                        st = LSF_SAMPLE_FLAT;
                        break;
                    }
                    y0 = y0 - (e * s.g0) / m, y1 = y1 - (e * s.g1) / m, y2 = y2 - (e * s.g2) / m;
                    // the moved point passes the INSIDE test of sp_sample before anything is loaded for it
                    const int s2 = sp_sample<CUBIC, false, HAS_MASK>(G, nullptr, y0, y1, y2, s);
                    if (s2 != LSF_SAMPLE_OK) {
                        st = s2;
                        break;
                    }
                }
            } else
                y0 = y1 = y2 = nan;
            if (foot) foot[t] = y0, foot[t + N] = y1, foot[t + 2 * N] = y2;
        }
        if (status) status[t] = st;
    }
    unsigned long long cnt[SP_NPART];
    cnt[0] = __popcll(__ballot(st == LSF_SAMPLE_OK));
    cnt[1] = __popcll(__ballot(st == LSF_SAMPLE_OUTSIDE));
    cnt[2] = __popcll(__ballot(st == LSF_SAMPLE_OFFBAND));
    cnt[3] = __popcll(__ballot(fallback));
    cnt[4] = __popcll(__ballot(st == LSF_SAMPLE_FLAT));
    cnt[5] = __popcll(__ballot(st == LSF_SAMPLE_NOT_CONVERGED));
    if ((threadIdx.x & 63) == 0)
        for (int m = 0; m < SP_NPART; ++m) red[threadIdx.x >> 6][m] = cnt[m];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* o = part + (size_t)blockIdx.x * SP_NPART;
        for (int m = 0; m < SP_NPART; ++m) {
            unsigned long long s = red[0][m];
            for (int w = 1; w < SP_BLOCK / 64; ++w) s += red[w][m];
            o[m] = s;
        }
    }
}

} // namespace lsf
