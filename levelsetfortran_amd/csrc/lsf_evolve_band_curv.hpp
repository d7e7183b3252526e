// lsf_evolve_band_curv.hpp -- the stage of lsf_evolve_band_curv (include/lsf.h): the transport stage of lsf_advect_band.hpp with the
// centrally differenced parabolic term bcurv * kappa * |grad(phi)| evaluated from the stage's own input field.
//
//     phi_t + u . grad(phi) + F |grad(phi)| = bcurv * kappa * |grad(phi)|
//
// k_advect_band_curv_stage is k_advect_band_stage with one more term, built from the same pieces (band_decode and band_stencil7 of
// lsf_band_cell.hpp, axis_pair, advect_rhs, stage_blend, block_umax): one lane per list cell, MB_CH consecutive entries per block.
// The two kernels stay two bodies: a per-cell function shared between them is optimised on its own before it is inlined and
// changes the machine code of both (see lsf_band_cell.hpp on the WENO rule).  A lane gathers from the stage's
// input field the cell, +-1 on each axis and the 12 edge diagonals (the 19 values of lsf_curvature_band.hpp) and, where a velocity
// or a speed is present and the cell is WENO, +-2 and +-3 on each axis (31 values in all); it reads u, v, w, speed and the step's old
// phi at its own point and stores the blend at its own point of the output field.  The curvature arithmetic is curv_derivs /
// curv_mean of lsf_curvature_band.hpp, uncontracted in STRICT and in FAST alike.  The instance without velocity and speed is pure
// curvature flow: it holds no transport code and gathers 19 values.  The partials / done protocol and the in-place stage 3 are those
// of k_advect_band_stage.
//
// Bounds: lsf_band_cell.hpp.  What is this kernel's own: every one of the 19 curvature values, the 12 diagonals among them, is at an
// offset in {-1, 0, 1}^3 of an interior point.
//
// Plain launches only: no atomics, no block waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_advect_band.hpp"
#include "lsf_curvature_band.hpp"

namespace lsf {

// One stage: list cell e of chunk blockIdx.x; A, Bout, P0, c_old, c_new, partials and done as in k_advect_band_stage.  out = t or
// c_old * P0 + c_new * t with t = (a - dt R0(a)) + dt * (bcurv * (H * g)).  two_dx = 2.*dx, dx2 = dx*dx, four_dx2 = 4.*(dx*dx) and
// lim = clamp / dx are computed once on the host; without a clamp lim = +inf, which no H exceeds.
template <bool STRICT, bool HASV, bool HASF>
__global__ __launch_bounds__(MB_CH) void k_advect_band_curv_stage(const double* __restrict__ A, double* Bout, const double* P0,
                                                                  const double* __restrict__ U, const double* __restrict__ V,
                                                                  const double* __restrict__ W, const double* __restrict__ F,
                                                                  const int* __restrict__ L, int nL, int nx, int ny, int nz, double dx, double dt,
                                                                  double c_old, double c_new, double bcurv, double two_dx, double dx2,
                                                                  double four_dx2, double lim, unsigned long long* __restrict__ partials,
                                                                  const int* __restrict__ done)
{
    if (done[CTL_STOP]) return;
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long acc = 0ull;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
        const double* c = A + p;
        const double phic = c[0];
        const bool blend = P0 != nullptr;
        const double old = blend ? P0[p] : phic;
        // the term: an interior point, so every offset in {-1, 0, 1}^3 lies inside the field
        double C;
        {
#pragma clang fp contract(off)
            bool deg;
            double g2, g;
            const CurvD d = curv_derivs(c, rs, ps, two_dx, dx2, four_dx2);
            double H = curv_mean(d, g2, g, deg);
            if (H > lim) H = lim;
            if (H < -lim) H = -lim;
            C = bcurv * (H * g);
        }
        double R = 0.0;
        if constexpr (HASV || HASF) {
            int i, j, k;
            band_decode(p, nx, ny, i, j, k);
            const bool weno_ok = i > 3 && i < nx - 4 && j > 3 && j < ny - 4 && k > 3 && k < nz - 4;
            double qx[7], qy[7], qz[7];
            band_stencil7(c, rs, ps, weno_ok, qx, qy, qz);
            double u = 0.0, v = 0.0, w = 0.0, f = 0.0;
            if constexpr (HASV) u = U[p], v = V[p], w = W[p];
            if constexpr (HASF) f = F[p];
            const double inv_dx = 1.0 / dx, floor2 = 1.E-99 * dx * dx / 13.0;
            double ax, bx, ay, by, az, bz;
            axis_pair<STRICT>(qx, weno_ok, false, dx, floor2, ax, bx);
            axis_pair<STRICT>(qy, weno_ok, false, dx, floor2, ay, by);
            axis_pair<STRICT>(qz, weno_ok, false, dx, floor2, az, bz);
            R = advect_rhs<STRICT, HASV, HASF>(ax, bx, ay, by, az, bz, u, v, w, f, inv_dx);
        }
        const double out = stage_blend<STRICT, HASV || HASF, true>(phic, dt, R, blend, c_old, old, c_new, C);
        Bout[p] = out;
        acc = (unsigned long long)__double_as_longlong(__builtin_fabs(out - old));
    }
    if (partials) {
        acc = block_umax<MB_CH / 64>(wave_umax_x(acc), threadIdx.x);
        if (threadIdx.x == 0) partials[blockIdx.x] = acc;
    }
}

} // namespace lsf
