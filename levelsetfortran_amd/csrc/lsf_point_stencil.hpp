// lsf_point_stencil.hpp -- what the calls that work on points share on the device (lsf_sample_points, lsf_cast_rays,
// lsf_advect_points, lsf_correct_field, lsf_reseed_points): the locate step, the band rule, the K^3 contractions, the sample at a
// position and the foot iteration.  Everything is evaluated as include/lsf.h writes it, left to right, without contraction.
//
// Bounds.  The test of pt_locate, made in double BEFORE any conversion to an integer, is the only thing between a wild coordinate
// (NaN, +-inf, 1e300, a point of another mesh, a position born of a non-finite field value) and an out-of-bounds load: a position
// that fails it returns before an index exists, and pt_sample makes it first for every position it is given.  Behind it
// 0 <= s <= n (the ray form admits -1e-6 <= s <= n + 1e-6 and clamps s into [0, n]), so 0 <= i0 <= n - 1 after the min and the
// corners i0, i0 + 1 lie in 0..n; the cubic stencil is taken only where 1 <= i0 <= n - 2, so i0 - 1 >= 0 and i0 + 2 <= n.  Every
// stencil point therefore exists whatever the mask holds.  The hosts refuse fields beyond 2^31 - 1 points; offsets are formed in 64
// bits all the same.  Every field handed to sp_stencil or pt_values3 has the size of phi and is read at these offsets only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/lsf.h"

namespace lsf {

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

// what pt_sample answers; the calls hand these on as their own statuses without a mapping
enum { PT_OK = 0, PT_OUTSIDE = 1, PT_OFFBAND = 2 };
static_assert(LSF_SAMPLE_OK == PT_OK && LSF_SAMPLE_OUTSIDE == PT_OUTSIDE && LSF_SAMPLE_OFFBAND == PT_OFFBAND, "lsf_sample_points, lsf_cast_rays, lsf_reseed_points");
static_assert(LSF_POINTS_OK == PT_OK && LSF_POINTS_OUTSIDE == PT_OUTSIDE && LSF_POINTS_OFFBAND == PT_OFFBAND, "lsf_advect_points");

// the header's fmax / fmin: b where a is NaN, else a where b is NaN or a >= b (a <= b), else b -- the first argument on a tie
__device__ __forceinline__ double cr_fmax(double a, double b) { return a != a ? b : ((b != b || a >= b) ? a : b); }
__device__ __forceinline__ double cr_fmin(double a, double b) { return a != a ? b : ((b != b || a <= b) ? a : b); }

// One axis of the header's "Locate"; RAY: with the tolerance of the ray sample.  false: refused, and then i0 and t mean nothing
// and must not be used.
template <bool RAY>
__device__ __forceinline__ bool pt_locate(double x, double lo, double dx, int n, int& i0, double& t)
{
#pragma clang fp contract(off)
    double s = (x - lo) / dx;
    // in double, before any integer exists: NaN fails both comparisons, +-inf and 1e300 one of them
    if constexpr (RAY) {
        if (!(s >= -1e-6 && s <= (double)n + 1e-6)) return false;
        s = cr_fmin(cr_fmax(s, 0.), (double)n);
    } else if (!(s >= 0.0 && s <= (double)n))
        return false;
    const int f = (int)__builtin_floor(s); // 0 <= s <= n <= 2^31 - 2: the conversion is exact
    i0 = f < n - 1 ? f : n - 1;            // the upper wall belongs to the last cell with t = 1
    t = s - (double)i0;
    return true;
}

// The band rule for the K^3 stencil whose lowest point is lo: every point an interior point (1..n-1 on each axis) with mask == 1 --
// the LIST rule of lsf_reinit_band.  The mask values are read side by side, without a branch between them: every stencil point
// exists (see "Bounds"), so all loads may be issued before the first arrives, where a test that leaves at the first value that is
// not 1 is a chain of K^3 load - wait - branch steps.  The 2 x 2 x 2 corners of the cell come first and decide alone for most
// off-list positions (one latency, 8 loads); the other 56 values of a cubic stencil follow in one more.
template <int K>
__device__ __forceinline__ bool pt_in_band(const SpGrid& G, const int (&lo)[3])
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

// Value and gradient of phi and (HAS_Q) the value of q on the K^3 stencil whose lowest point is lo.  No band test.  The values are
// contracted as they arrive: a row of K along x becomes one value (and one x-derivative), the K rows of a plane become three numbers
// (value, d/dx, d/dy), the K planes the value and the three derivatives.  At most K + K row results and 3 K plane results are live;
// the K^3 values never are.
template <bool CUBIC, bool HAS_Q>
__device__ __forceinline__ void sp_stencil(const SpGrid& G, const double* __restrict__ q, const int (&lo)[3], const double (&t)[3], SpSample& o)
{
#pragma clang fp contract(off)
    constexpr int K = CUBIC ? 4 : 2;
    const long rs = (long)G.nx + 1, ps = rs * ((long)G.ny + 1);
    const long base = (long)lo[0] + rs * (long)lo[1] + ps * (long)lo[2];
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
}

// The values of three fields on the same stencil under one set of weights: sp_stencil's value, three times, without a gradient.
// (One routine for this and sp_stencil costs registers in the cubic kernels: profiles/point_refactor.txt.)
template <bool CUBIC>
__device__ __forceinline__ void pt_values3(const SpGrid& G, const double* u, const double* v, const double* w, const int (&lo)[3],
                                           const double (&t)[3], double (&U)[3])
{
#pragma clang fp contract(off)
    constexpr int K = CUBIC ? 4 : 2;
    const long rs = (long)G.nx + 1, ps = rs * ((long)G.ny + 1);
    const long base = (long)lo[0] + rs * (long)lo[1] + ps * (long)lo[2];
    double wx[K], wy[K], wz[K], dd[K];
    sp_weights<CUBIC>(t[0], wx, dd);
    sp_weights<CUBIC>(t[1], wy, dd);
    sp_weights<CUBIC>(t[2], wz, dd);
    const double* __restrict__ f[3] = {u + base, v + base, w + base};
    double p[3][K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double r[3][K];
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                double a[K];
#pragma unroll
                for (int i = 0; i < K; ++i) a[i] = f[m][i + rs * b + ps * c];
                r[m][b] = sp_dot<K>(wx, a);
            }
#pragma unroll
        for (int m = 0; m < 3; ++m) p[m][c] = sp_dot<K>(wy, r[m]);
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) U[m] = sp_dot<K>(wz, p[m]);
}

// One sample at (x, y, z) by the rules of the header: the three locates (PT_OUTSIDE; see "Bounds": nothing else may run for a
// position that fails them), the joint rule -- cubic only where 1 <= i0 <= n - 2 on all three axes -- the band rule where there is a
// mask (PT_OFFBAND), then eval(std::bool_constant<cubic stencil>, lo, t) on the admitted stencil, whose answer (PT_OK, or a status
// of the caller's own) is handed on.  linear: the 2 x 2 x 2 stencil served; written wherever eval ran, whatever it answered.
template <bool CUBIC, bool HAS_MASK, bool RAY, class Eval>
__device__ __forceinline__ int pt_sample(const SpGrid& G, double x, double y, double z, bool& linear, Eval&& eval)
{
    int i0[3];
    double t[3];
    if (!pt_locate<RAY>(x, G.x0, G.dx, G.nx, i0[0], t[0]) || !pt_locate<RAY>(y, G.y0, G.dx, G.ny, i0[1], t[1]) ||
        !pt_locate<RAY>(z, G.z0, G.dx, G.nz, i0[2], t[2]))
        return PT_OUTSIDE;
    if constexpr (CUBIC) {
        if (i0[0] >= 1 && i0[0] <= G.nx - 2 && i0[1] >= 1 && i0[1] <= G.ny - 2 && i0[2] >= 1 && i0[2] <= G.nz - 2) {
            const int lo[3] = {i0[0] - 1, i0[1] - 1, i0[2] - 1};
            if constexpr (HAS_MASK)
                if (!pt_in_band<4>(G, lo)) return PT_OFFBAND;
            linear = false;
            return eval(std::true_type{}, lo, t);
        }
    }
    if constexpr (HAS_MASK)
        if (!pt_in_band<2>(G, i0)) return PT_OFFBAND;
    linear = true;
    return eval(std::false_type{}, i0, t);
}

// The sample of lsf_sample_points: LSF_SAMPLE_OK, _OUTSIDE or _OFFBAND; o is written on OK only (eval always answers OK here).  RAY: the ray sample of
// lsf_cast_rays.
template <bool CUBIC, bool HAS_Q, bool HAS_MASK, bool RAY = false>
__device__ __forceinline__ int sp_sample(const SpGrid& G, const double* __restrict__ q, double x, double y, double z, SpSample& o)
{
    return pt_sample<CUBIC, HAS_MASK, RAY>(G, x, y, z, o.linear, [&](auto cubic, const int(&lo)[3], const double(&t)[3]) __attribute__((always_inline)) {
        sp_stencil<decltype(cubic)::value, HAS_Q>(G, q, lo, t, o);
        return (int)PT_OK;
    });
}

// The foot iteration: Newton steps along the interpolant's gradient from y onto phi = goal.  s is the sample at y on entry.  Up to
// `iters` moves, and one more sample for the test after the last.  Returns LSF_SAMPLE_OK, _NOT_CONVERGED, _FLAT, or the status of
// the moved point's sample that was not OK; y is the last position reached.
template <bool CUBIC, bool HAS_MASK>
__device__ __forceinline__ int pt_foot(const SpGrid& G, double goal, int iters, double tol_dx, SpSample& s, double& y0, double& y1, double& y2)
{
#pragma clang fp contract(off)
    for (int it = 0;; ++it) {
        const double e = s.v - goal;
        if (!(__builtin_fabs(e) > tol_dx)) return LSF_SAMPLE_OK;
        if (it == iters) return LSF_SAMPLE_NOT_CONVERGED;
        const double m = (s.g0 * s.g0 + s.g1 * s.g1) + s.g2 * s.g2;
        if (m == 0.0) return LSF_SAMPLE_FLAT;
        y0 = y0 - (e * s.g0) / m, y1 = y1 - (e * s.g1) / m, y2 = y2 - (e * s.g2) / m;
        const int s2 = sp_sample<CUBIC, false, HAS_MASK>(G, nullptr, y0, y1, y2, s);
        if (s2 != LSF_SAMPLE_OK) return s2;
    }
}

} // namespace lsf
