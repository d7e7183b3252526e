// lsf_redistance_band.hpp -- closest-point redistancing of a cell list: the cells next to the surface take the length of the segment
// to their foot on the interpolant's zero level set, the rest of the list is filled from them by Jacobi passes of lsf_distance_fill's
// visit: lsf_redistance_band (include/lsf_redistance.h; account: DESIGN.md section 4.27; driver: lsf_host_redistance_band.hpp).
//
// The list is lsf_reinit_band's,
//     LIST = { interior points with mask == 1 on entry },
// built by the same machinery (band_list_count<true> / band_list_sort: brick-sorted 32-bit point indices).  Every kernel is a plain
// launch, one lane per list entry, MB_CH consecutive entries -- a few neighbouring bricks -- per block; no kernel waits for another
// block, and the only loop is pt_foot's, bounded by `iters`.
//   k_rdb_foot     once per call, read-only on the caller's arrays.  The cell as a point ((double)i dx, (double)j dx, (double)k dx) of
//                  the grid with xLo = 0 is sampled and projected by the rules of lsf_sample_points, word for word (sp_sample and
//                  pt_foot of lsf_point_stencil.hpp: cubic with the linear fallback of the joint rule, the mask as the band, iso 0).
//                  Per entry: the value on entry, its sign, dist = |x - foot| where the cell is FROZEN (status OK and dist <
//                  near dx) and +inf elsewhere, the frozen flag, and which of the six axis neighbours are in the list.  Per block
//                  the counts the host decides the errors on and fills info[] from.
//   k_rdb_seed     the magnitudes u into the field at list cells: dist at frozen cells, +inf at the others.  After the host has
//                  decided the errors: the first write of the call.
//   k_rdb_compute  one pass, first half: the smaller neighbour magnitude per axis (a neighbour that is not in the list counts as
//                  +inf), df_solve of lsf_distance_fill.hpp, new = min(old, t); the new value and a store flag go to per-entry
//                  arrays.  The field is only read.  The second half is k_extb_commit of lsf_extend_band.hpp, unchanged: the stores
//                  at the lanes' own points and one integer add per block into cnt[pass].  Two launches per pass: all reads of a
//                  pass come before its writes (Jacobi).
//   k_rdb_finish   the result rule: frozen cells take s dist (dist == 0.0: the value on entry), reached cells s u, cells still at
//                  +inf the value on entry.  Per block the filled and unreached counts and the largest |new - old| as a bit pattern.
// The stop test is lsf_extend_band.hpp's: cnt[] holds one count per pass of a batch and is zeroed before the batch is enqueued; the
// kernels of pass p > 0 of a batch return at once when cnt[p - 1] == 0.
//
// Bounds: "Bounds" of lsf_point_stencil.hpp for every sample; lsf_band_cell.hpp for the six neighbours (a list entry is an interior
// point, so p - 1, p + 1 and the points one row and one plane away exist).  A neighbour that is not in the list is not loaded: the
// lane loads its own point instead, so u is read at list cells only.  Per-entry arrays are indexed by e < nL only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf_redistance.h"
#include "lsf_block_reduce.hpp"
#include "lsf_distance_fill.hpp"
#include "lsf_extend_band.hpp"
#include "lsf_point_stencil.hpp"

namespace lsf {

// partials per block of k_rdb_foot: frozen cells, feet OFFBAND, OUTSIDE, FLAT, NOT_CONVERGED, OK but dist >= near dx (info[1], [4..8]
// in that order), and list cells with a non-finite phi at themselves
constexpr int RDB_NPART = 7;
constexpr int RDB_NFIN = 3; // ... of k_rdb_finish: filled, unreached, the largest |new - old| as a bit pattern
// flag bytes per entry, one array each: frozen, phi < 0 on entry, the six in-list bits (bit 2 x + side), the store flag of a pass
constexpr int RDB_NFLAG = 4;

// G: the field, the mask, the grid with xLo = 0.  tol_dx = tol * dx and near_dx = near * dx, computed once on the host.
__global__ __launch_bounds__(MB_CH) void k_rdb_foot(SpGrid G, const int* __restrict__ L, int nL, int iters, double tol_dx, double near_dx,
                                                    double* __restrict__ dist, double* __restrict__ old, unsigned char* __restrict__ fz,
                                                    unsigned char* __restrict__ neg, unsigned char* __restrict__ nbits,
                                                    unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    int st = -1; // no entry
    bool frozen = false, bad = false;
    if (e < nL) {
        const int p = L[e];
        const int rs = G.nx + 1, ps = (G.nx + 1) * (G.ny + 1);
        const int k = p / ps, r = p - k * ps, j = r / rs, i = r - j * rs;
        const int c[3] = {i, j, k}, n1[3] = {G.nx, G.ny, G.nz}, sd[3] = {1, rs, ps};
        unsigned in = 0;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            // p - sd and p + sd exist; a wall point is not in the list whatever its mask word holds
            in |= (c[x] - 1 >= 1 && G.mask[p - sd[x]] == 1) ? 1u << (2 * x) : 0u;
            in |= (c[x] + 1 <= n1[x] - 1 && G.mask[p + sd[x]] == 1) ? 2u << (2 * x) : 0u;
        }
        const double a = G.phi[p];
        bad = !__builtin_isfinite(a);
        const double x0 = (double)i * G.dx, x1 = (double)j * G.dx, x2 = (double)k * G.dx;
        double y0 = x0, y1 = x1, y2 = x2, d = HUGE_VAL;
        SpSample s;
        st = sp_sample<true, false, true>(G, nullptr, x0, x1, x2, s);
        if (st == LSF_SAMPLE_OK) st = pt_foot<true, true>(G, 0.0, iters, tol_dx, s, y0, y1, y2);
        if (st == LSF_SAMPLE_OK) {
            const double d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
            const double len = __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            frozen = len < near_dx;
            d = frozen ? len : HUGE_VAL;
        }
        dist[e] = d;
        old[e] = a;
        fz[e] = frozen ? 1 : 0;
        neg[e] = a < 0.0 ? 1 : 0;
        nbits[e] = (unsigned char)in;
    }
    unsigned long long cnt[RDB_NPART] = {wave_count(frozen),
                                         wave_count(st == LSF_SAMPLE_OFFBAND),
                                         wave_count(st == LSF_SAMPLE_OUTSIDE),
                                         wave_count(st == LSF_SAMPLE_FLAT),
                                         wave_count(st == LSF_SAMPLE_NOT_CONVERGED),
                                         wave_count(st == LSF_SAMPLE_OK && !frozen),
                                         wave_count(bad)};
    block_usum_out<MB_CH / 64, true>(cnt, (int)threadIdx.x, part + (size_t)blockIdx.x * RDB_NPART);
}

__global__ __launch_bounds__(MB_CH) void k_rdb_seed(double* __restrict__ u, const int* __restrict__ L, const double* __restrict__ dist, int nL)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    if (e < nL) u[L[e]] = dist[e];
}

// Pass `pass` of a batch, first half.  u is read at list cells only and never written here.
__global__ __launch_bounds__(MB_CH) void k_rdb_compute(const double* __restrict__ u, const int* __restrict__ L, const unsigned char* __restrict__ fz,
                                                       const unsigned char* __restrict__ nbits, int nL, int nx, int ny, double dx,
                                                       double* __restrict__ nv, unsigned char* __restrict__ chg,
                                                       const unsigned long long* __restrict__ cnt, int pass)
{
#pragma clang fp contract(off)
    if (pass > 0 && cnt[pass - 1] == 0ull) return; // the pass before lowered nothing: the call is over
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    if (e >= nL) return;
    if (fz[e]) {
        chg[e] = 0;
        return;
    }
    const int p = L[e];
    const int sd[3] = {1, nx + 1, (nx + 1) * (ny + 1)};
    const unsigned in = nbits[e];
    const double old = u[p];
    double m[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const bool has_lo = (in >> (2 * x)) & 1u, has_hi = (in >> (2 * x + 1)) & 1u;
        const double lo = u[has_lo ? p - sd[x] : p], hi = u[has_hi ? p + sd[x] : p]; // both loads go out before either is used
        m[x] = fmin(has_lo ? lo : HUGE_VAL, has_hi ? hi : HUGE_VAL);
    }
    bool low = false;
    if (fmin(fmin(m[0], m[1]), m[2]) < HUGE_VAL) {
        const double t = df_solve(m[0], m[1], m[2], dx);
        low = t < old;
        nv[e] = t;
    }
    chg[e] = low ? 1 : 0;
}

// part: RDB_NFIN words per block
__global__ __launch_bounds__(MB_CH) void k_rdb_finish(double* __restrict__ phi, const int* __restrict__ L, const double* __restrict__ dist,
                                                      const double* __restrict__ old, const unsigned char* __restrict__ fz,
                                                      const unsigned char* __restrict__ neg, int nL, unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long red[MB_CH / 64][RDB_NFIN];
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    bool filled = false, unreached = false;
    unsigned long long diff = 0ull; // the bit pattern of 0.0
    if (e < nL) {
        const int p = L[e];
        const double a = old[e];
        const bool frozen = fz[e] != 0;
        const double m = frozen ? dist[e] : phi[p];
        filled = !frozen && m < HUGE_VAL;
        unreached = !frozen && !filled;
        const bool keep = unreached || (frozen && m == 0.0);
        const double v = keep ? a : (neg[e] ? -m : m);
        phi[p] = v;
        diff = (unsigned long long)__double_as_longlong(__builtin_fabs(v - a));
    }
    const unsigned long long w[RDB_NFIN] = {wave_count(filled), wave_count(unreached), wave_umax_x(diff)};
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < RDB_NFIN; ++q) red[threadIdx.x >> 6][q] = w[q];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[RDB_NFIN] = {red[0][0], red[0][1], red[0][2]};
        for (int q = 1; q < MB_CH / 64; ++q) {
            t[0] += red[q][0], t[1] += red[q][1];
            t[2] = red[q][2] > t[2] ? red[q][2] : t[2];
        }
        for (int q = 0; q < RDB_NFIN; ++q) part[(size_t)blockIdx.x * RDB_NFIN + q] = t[q];
    }
}

} // namespace lsf
