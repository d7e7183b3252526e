// lsf_advect_field.hpp -- level-set transport on the whole grid: lsf_advect_field (include/lsf.h).
//
//     phi_t + u . grad(phi) + F |grad(phi)| = 0,      explicit in time (TVD-RK3 of Shu and Osher, or forward Euler)
//
// No reference counterpart ("Currently has no capability to do moving geometry", the reference's README).  The one-sided
// derivatives are the reference's WENO5 pair (lsf_cell.hpp: axis_pair, weno subs.f90:489-711) WITHOUT the p5 = 0 quirk of its y
// axis (subs.f90:576), which belongs to its reinit; the WENO rule is its joint one (cells 4..n-5 on all three axes, first-order
// differences otherwise).  The velocity term is upwinded component by component, the normal-speed term is the Godunov
// Hamiltonian of the reinit update switched on the sign of the speed instead of the sign of phi (axis_godunov).
//
// One launch per stage over the interior (k_advect_stage), modelled on k_reinit_jacobi (lsf_kernels.hpp): 64 consecutive lanes
// along x, 4 rows per block, a march of ADV_KC planes along z with a 7-deep register window, x and y stencil points through
// L1 / L2.  Per lane and plane u, v, w, speed, the step's old phi and the store are one coalesced 8-byte access each.  A stage
// writes t = a - dt R(a) (stage 1, Euler) or c_old * old + c_new * t (stages 2 and 3): whether the old field is loaded is a
// wave-uniform test of its pointer.  The last stage of a step also reduces max |new - old| (a pointer test again): one partial
// per block, k_advect_finish closes the step.  Plain launches only: no block waits for another, no atomics.
//
// Every load offset lies inside its plane BY CONSTRUCTION (an offset that wrapped below zero passed the
// descriptor's range check at 512^3): a lane works only if its cell is interior (1..n-1), reads +-1 then, and +-3 only if the
// cell is 4..n-5 on that axis; the planes of the z window are clamped to 0..nz.  The descriptor's range is a second line only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_block_reduce.hpp"
#include "lsf_kernels.hpp"

namespace lsf {

constexpr int ADV_BX = 64, ADV_BY = 4; // a block: 64 cells along x by 4 rows
constexpr int ADV_KC = 32;             // planes a block marches (tests/test_gpu_advect_field.py has a grid longer than this)
constexpr int ADV_SCAN_BLOCKS = 1024;  // most blocks of the input scan (k_advect_scan): its partials are finished on the host

// |new - old| is reduced as the bit pattern of a non-negative double: as unsigned integers these order like the numbers, +inf is
// the largest of them and every NaN (sign cleared) lies above +inf -- one integer maximum gives "the largest change, NaN if any
// is NaN" whatever the order of the operands, so the trace is the same from run to run and between the seams.
constexpr unsigned long long ADV_INF_BITS = 0x7ff0000000000000ull;

// R = u . grad(phi) + F |grad(phi)| of one cell from its three pairs of one-sided derivatives (include/lsf.h, lsf_advect_field).
// STRICT: true derivatives, evaluated as written, left to right, no contraction.  FAST: derivatives times dx (axis_pair<false>),
// one multiplication by 1/dx at the end, contraction allowed.
template <bool STRICT, bool HASV, bool HASF>
__device__ __forceinline__ double advect_rhs(double ax, double bx, double ay, double by, double az, double bz, double u, double v, double w,
                                             double f, double inv_dx)
{
    if constexpr (STRICT) {
#pragma clang fp contract(off)
        double T = 0.0, N = 0.0;
        if constexpr (HASV) {
            const double up = u > 0. ? u : 0., un = u < 0. ? u : 0.;
            const double vp = v > 0. ? v : 0., vn = v < 0. ? v : 0.;
            const double wp = w > 0. ? w : 0., wn = w < 0. ? w : 0.;
            T = ((up * ax + un * bx) + (vp * ay + vn * by)) + (wp * az + wn * bz);
        }
        if constexpr (HASF) {
            const double S = (axis_godunov<true>(f, ax, bx) + axis_godunov<true>(f, ay, by)) + axis_godunov<true>(f, az, bz);
            // the IEEE square root by the hardware sequence without its frame where the operand allows it (sqrt_unframed)
            const double g = __builtin_expect(S >= 1.0e-200 && S <= 1.0e200, 1) ? sqrt_unframed(S) : __builtin_sqrt(S);
            N = f * g;
        }
        return HASV && HASF ? T + N : (HASV ? T : N);
    } else {
        double R = 0.0;
        if constexpr (HASF) {
            const double S = (axis_godunov<false>(f, ax, bx) + axis_godunov<false>(f, ay, by)) + axis_godunov<false>(f, az, bz); // times dx^2
            // sqrt(S) = S y0 refined once with the residual (finish_update<false>); S = 0: g = 0
            const double y0 = __builtin_amdgcn_rsq(__builtin_fmax(S, 1e-300));
            const double g0 = S * y0;
            const double g = __builtin_fma(__builtin_fma(-g0, g0, S), 0.5 * y0, g0);
            R = f * (g * inv_dx);
        }
        if constexpr (HASV) {
            const double up = __builtin_fmax(u, 0.), un = __builtin_fmin(u, 0.);
            const double vp = __builtin_fmax(v, 0.), vn = __builtin_fmin(v, 0.);
            const double wp = __builtin_fmax(w, 0.), wn = __builtin_fmin(w, 0.);
            const double T = __builtin_fma(up, ax, un * bx) + __builtin_fma(vp, ay, vn * by) + __builtin_fma(wp, az, wn * bz);
            R = __builtin_fma(T, inv_dx, R);
        }
        return R;
    }
}

// What a stage stores for one cell: t = a - dt R (TRANSPORT) + dt C (CURV, lsf_evolve_band_curv.hpp), or c_old * old + c_new * t
// when the stage blends.  STRICT: as written, no contraction.  Shared by the stage kernels of the grid and of the band.
template <bool STRICT, bool TRANSPORT = true, bool CURV = false>
__device__ __forceinline__ double stage_blend(double phic, double dt, double R, bool blend, double c_old, double old, double c_new, double C = 0.0)
{
    if constexpr (STRICT) {
#pragma clang fp contract(off)
        double t = phic;
        if constexpr (TRANSPORT) t = phic - dt * R;
        if constexpr (CURV) t = t + dt * C;
        return blend ? c_old * old + c_new * t : t;
    } else {
        double t = phic;
        if constexpr (TRANSPORT) t = __builtin_fma(-dt, R, phic);
        if constexpr (CURV) t = __builtin_fma(dt, C, t);
        return blend ? __builtin_fma(c_old, old, c_new * t) : t;
    }
}

// One stage over the interior cells 1..n-1.  A = the stage's input field, Bout = its output (never A); P0 = the field at the start
// of the step, or nullptr: out = t = a - dt R(a); with P0: out = c_old * P0 + c_new * t.  P0 may BE Bout (stage 3 of RK3 writes the
// caller's field in place): a lane reads P0 at its own point only, before it stores there.  partials != nullptr: the last stage
// of a step, one maximum of |out - old| per block (old = P0, or A when there is none) as a bit pattern.
// The launch is one-dimensional, padded to a multiple of 8 and numbered XCD-aware like k_reinit_jacobi_strict_sh: XCD x takes the
// logical blocks [x * per, (x + 1) * per), x fastest, then y, then the chunks along z.
template <bool STRICT, bool HASV, bool HASF>
__global__ __launch_bounds__(ADV_BX* ADV_BY) void k_advect_stage(const double* __restrict__ A, double* Bout, const double* P0,
                                                                  const double* __restrict__ U, const double* __restrict__ V,
                                                                  const double* __restrict__ W, const double* __restrict__ F, int nx, int ny,
                                                                  int nz, double dx, double dt, double c_old, double c_new,
                                                                  unsigned long long* __restrict__ partials, const int* __restrict__ done,
                                                                  int nbx, int nby, int nbz)
{
    if (done && done[CTL_STOP]) return;
    const unsigned per = gridDim.x >> 3;
    const unsigned L = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (L >= (unsigned)nbx * (unsigned)nby * (unsigned)nbz) return; // padding
    const int bxi = (int)(L % (unsigned)nbx), byi = (int)((L / (unsigned)nbx) % (unsigned)nby), bzi = (int)(L / ((unsigned)nbx * (unsigned)nby));
    const int li = 1 + bxi * ADV_BX + (int)threadIdx.x, lj = 1 + byi * ADV_BY + (int)threadIdx.y;
    const int k0 = 1 + bzi * ADV_KC, k1 = min(k0 + ADV_KC, nz);
    const long sx = nx + 1, sxy = (long)(nx + 1) * (ny + 1);
    unsigned long long acc = 0ull;
    if (li < nx && lj < ny) { // an interior column: 1 <= li <= nx-1, 1 <= lj <= ny-1
        const bool ij_weno = li > 3 && li < nx - 4 && lj > 3 && lj < ny - 4;
        const double inv_dx = 1.0 / dx, floor2 = 1.E-99 * dx * dx / 13.0;
        // one buffer descriptor per k-plane (the scalar unit rebuilds it every step) + the lane's 32-bit byte offset in the plane
        const unsigned plane_bytes = 8u * (unsigned)sxy, rowb = 8u * (unsigned)sx;
        const unsigned col = 8u * (unsigned)(li + sx * lj);
        auto desc = [&](const double* base) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), 0, (int)plane_bytes, 0x00020000); };
        auto at = [](__amdgpu_buffer_rsrc_t r, unsigned boff) -> double {
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            const u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, boff, 0, 0);
            return __hiloint2double((int)v.y, (int)v.x);
        };
        auto ldz = [&](int k) -> double { return at(desc(A + sxy * min(max(k, 0), nz)), col); }; // planes beyond a wall: never consumed
        double qz[7];
#pragma unroll
        for (int m = 0; m < 6; ++m) qz[m + 1] = ldz(k0 - 3 + m);
        for (int k = k0; k < k1; ++k) {
#pragma unroll
            for (int m = 0; m < 6; ++m) qz[m] = qz[m + 1];
            qz[6] = ldz(k + 3);
            const bool weno_ok = ij_weno && k > 3 && k < nz - 4;
            const double phic = qz[3];
            const auto P = desc(A + sxy * k);
            double qx[7], qy[7];
#pragma unroll
            for (int m = 0; m < 7; ++m) qx[m] = qy[m] = 0.0;
            qx[3] = qy[3] = phic;
            if (weno_ok) { // 4 <= li <= nx-5, 4 <= lj <= ny-5: li-3 .. li+3 are in the row, lj-3 .. lj+3 in the plane
#pragma unroll
                for (int m = 0; m < 7; ++m)
                    if (m != 3) {
                        qx[m] = at(P, col - 24u + 8u * (unsigned)m);
                        qy[m] = at(P, col - 3u * rowb + (unsigned)m * rowb);
                    }
            } else { // li +- 1 in 0..nx, lj +- 1 in 0..ny
                qx[2] = at(P, col - 8u), qx[4] = at(P, col + 8u);
                qy[2] = at(P, col - rowb), qy[4] = at(P, col + rowb);
            }
            double u = 0.0, v = 0.0, w = 0.0, f = 0.0;
            if constexpr (HASV) u = at(desc(U + sxy * k), col), v = at(desc(V + sxy * k), col), w = at(desc(W + sxy * k), col);
            if constexpr (HASF) f = at(desc(F + sxy * k), col);
            const bool blend = P0 != nullptr;
            const double old = blend ? at(desc(P0 + sxy * k), col) : phic;
            double ax, bx, ay, by, az, bz;
            axis_pair<STRICT>(qx, weno_ok, false, dx, floor2, ax, bx);
            axis_pair<STRICT>(qy, weno_ok, false, dx, floor2, ay, by);
            axis_pair<STRICT>(qz, weno_ok, false, dx, floor2, az, bz);
            const double R = advect_rhs<STRICT, HASV, HASF>(ax, bx, ay, by, az, bz, u, v, w, f, inv_dx);
            const double out = stage_blend<STRICT>(phic, dt, R, blend, c_old, old, c_new);
            {
                typedef unsigned u2 __attribute__((ext_vector_type(2)));
                u2 s;
                s.x = (unsigned)__double2loint(out);
                s.y = (unsigned)__double2hiint(out);
                __builtin_amdgcn_raw_buffer_store_b64(s, desc(Bout + sxy * k), col, 0, 0);
            }
            const unsigned long long d = (unsigned long long)__double_as_longlong(__builtin_fabs(out - old));
            acc = d > acc ? d : acc;
        }
    }
    if (partials) {
        acc = wave_umax_x(acc);
        const int tid = threadIdx.x + ADV_BX * threadIdx.y;
        acc = block_umax<ADV_BX * ADV_BY / 64>(acc, tid);
        if (tid == 0) partials[L] = acc;
    }
}

// End of a step: the maximum of the blocks' partials -> trace[step] (NaN if any change was NaN), the step counter, the NaN verdict.
// CTL_STOP: later launches of the call leave at once; CTL_COUNT = steps completed; CTL_NAN: a change was NaN
static __global__ __launch_bounds__(RED_T) void k_advect_finish(const unsigned long long* __restrict__ partials, long nPart, double* __restrict__ trace,
                                                                int trace_cap, int* __restrict__ ctl)
{
    __shared__ unsigned long long red[RED_T];
    if (ctl[CTL_STOP]) return;
    unsigned long long t[4] = {0ull, 0ull, 0ull, 0ull}; // four loads in flight per round
    long p = threadIdx.x;
    for (; p + 3L * RED_T < nPart; p += 4L * RED_T) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long x = partials[p + (long)q * RED_T];
            t[q] = x > t[q] ? x : t[q];
        }
    }
    for (; p < nPart; p += RED_T) {
        const unsigned long long x = partials[p];
        t[0] = x > t[0] ? x : t[0];
    }
    const unsigned long long a = t[0] > t[1] ? t[0] : t[1], b = t[2] > t[3] ? t[2] : t[3];
    red[threadIdx.x] = a > b ? a : b;
    __syncthreads();
    for (int s = RED_T / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long bits = red[0];
        const bool nan = bits > ADV_INF_BITS;
        const int n = ctl[CTL_COUNT];
        if (n < trace_cap) trace[n] = nan ? __builtin_nan("") : __longlong_as_double((long long)bits);
        ctl[CTL_COUNT] = n + 1;
        if (nan) ctl[CTL_STOP] = 1, ctl[CTL_NAN] = 1;
    }
}

// The inputs, once per call: the largest |u| + |v| + |w| + |speed| over all points (absent fields left out, added left to right)
// and the number of non-finite values.  One pair of partials per block; the host finishes (at most ADV_SCAN_BLOCKS pairs).
// The body scans n entries: the points 0 .. n-1 themselves (LIST false, k_advect_scan) or the points L[0 .. n-1] (LIST true,
// k_advect_band_scan of lsf_advect_band.hpp).
template <bool LIST>
__device__ __forceinline__ void advect_scan_body(const double* __restrict__ U, const double* __restrict__ V, const double* __restrict__ W,
                                                 const double* __restrict__ F, const int* __restrict__ L, long n, double* __restrict__ pmax,
                                                 unsigned long long* __restrict__ pcnt)
{
#pragma clang fp contract(off)
    __shared__ double rm[4];
    __shared__ unsigned long long rc[4];
    double m = 0.0;
    unsigned long long c = 0ull;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += 256L * gridDim.x) {
        long p = e;
        if constexpr (LIST) p = L[e];
        double s = 0.0;
        if (U) {
            const double a = U[p], b = V[p], d = W[p];
            c += (unsigned long long)(!__builtin_isfinite(a)) + (unsigned long long)(!__builtin_isfinite(b)) + (unsigned long long)(!__builtin_isfinite(d));
            s = (__builtin_fabs(a) + __builtin_fabs(b)) + __builtin_fabs(d);
        }
        if (F) {
            const double a = F[p];
            c += (unsigned long long)(!__builtin_isfinite(a));
            s = s + __builtin_fabs(a);
        }
        m = __builtin_fmax(m, s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = __builtin_fmax(m, __shfl_xor(m, o, 64));
    c = wave_usum(c);
    if ((threadIdx.x & 63) == 0) rm[threadIdx.x >> 6] = m, rc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        pmax[blockIdx.x] = __builtin_fmax(__builtin_fmax(rm[0], rm[1]), __builtin_fmax(rm[2], rm[3]));
        pcnt[blockIdx.x] = (rc[0] + rc[1]) + (rc[2] + rc[3]);
    }
}

static __global__ __launch_bounds__(256) void k_advect_scan(const double* __restrict__ U, const double* __restrict__ V, const double* __restrict__ W,
                                                            const double* __restrict__ F, long n, double* __restrict__ pmax,
                                                            unsigned long long* __restrict__ pcnt)
{
    advect_scan_body<false>(U, V, W, F, nullptr, n, pmax, pcnt);
}

} // namespace lsf
