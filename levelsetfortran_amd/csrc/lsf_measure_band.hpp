// lsf_measure_band.hpp -- surface and volume integrals of the level set phi = iso over the cells of a caller's mask: lsf_measure_band
// (include/lsf.h).
//
// The list is lsf_reinit_band's,
//     LIST = { interior points with mask == 1 on entry },
// built by the same machinery (band_list_count<true> / band_list_sort: brick-sorted 32-bit point indices).  A list point names the
// cell whose lower corner it is (a MEASURED cell).  Two launches over the list, one lane per list cell, MB_CH consecutive entries per
// block, modelled on k_curvature_band:
//   k_measure_check  gathers the 8 corners (16 with q) through L1/L2, forms the corner byte and, for a crossed cell, counts the
//                    crossed edges among the 19 of its six tetrahedra that have a non-finite phi - iso (or q) on an endpoint.  The
//                    two counts go to ctl with one integer atomic per wave that has any.
//   k_measure_band   returns at once when ctl holds a count (nothing is written then: the host refuses the call).  Otherwise a lane
//                    gathers its 8 corners, leaves with 0.0 when the corner byte is 0 or 255, and walks the triangles of its cell
//                    with xs_cell_emit of lsf_extract_surface.hpp -- the rule that emits them, used unchanged.  A node is computed
//                    where it is used: its two endpoints are read again (L1 hits: the lane has just gathered them), so no corner
//                    array is indexed by a run-time value and nothing spills.  Per triangle the nine terms of the header, evaluated
//                    as written without contraction; a cell adds its triangles to 0.0 in emission order.
// Reduction: the nine sums of a lane's cell are added over the wave by an xor butterfly (every lane of a pair forms the same sum, so
// the pattern is fixed), the four wave sums in wave order through LDS, one set of partials per block; the host adds the blocks in
// block order.  Counts are integers.  Plain launches, no floating-point atomic, no block waits for another: the totals are a
// function of field, mask and list order alone.
//
// Bounds: lsf_band_cell.hpp.  What is this file's own: a list entry is an interior point, so i + 1 <= nx, j + 1 <= ny, k + 1 <= nz
// and the eight corners p + {0,1} + {0,1}*row + {0,1}*plane exist; the OPEN test is band_listed6.  The one store is at the lane's
// own point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_advect_band.hpp"
#include "lsf_extract_surface.hpp"

namespace lsf {

constexpr int MS_NQ = 9;   // area, volume, x dV, y dV, z dV, x dS, y dS, z dS, q dS
constexpr int MS_NCNT = 4; // integer partials per block: crossed cells, triangles, open cells, triangles of area 0.0
enum { MS_BAD_F = 0, MS_BAD_Q = 1, MS_CTL_LEN = 2 };

struct MsNode {
    double x, y, z, q;
};

// the node on the edge between the corner offsets u < v (x + 2y + 4z) of the cell whose lower corner is the point at `phi`
template <bool HASQ>
__device__ __forceinline__ MsNode ms_node(const double* __restrict__ phi, const double* __restrict__ q, long rs, long ps, int i, int j, int k,
                                          unsigned u, unsigned v, double iso, double dx, double x0, double y0, double z0)
{
#pragma clang fp contract(off)
    const long oa = (long)(u & 1u) + rs * (long)((u >> 1) & 1u) + ps * (long)((u >> 2) & 1u);
    const long ob = (long)(v & 1u) + rs * (long)((v >> 1) & 1u) + ps * (long)((v >> 2) & 1u);
    const double fa = phi[oa] - iso, fb = phi[ob] - iso;
    const double t = fa / (fa - fb);
    const unsigned d = u ^ v;
    MsNode n;
    n.x = xs_coord(x0, i + (int)(u & 1u), d & 1u, t, dx);
    n.y = xs_coord(y0, j + (int)((u >> 1) & 1u), d & 2u, t, dx);
    n.z = xs_coord(z0, k + (int)((u >> 2) & 1u), d & 4u, t, dx);
    n.q = 0.0;
    if constexpr (HASQ) {
        const double qa = q[oa], qb = q[ob];
        n.q = qa + t * (qb - qa);
    }
    return n;
}

// the nine terms of one triangle added to a cell's sums, as the header writes them
template <bool HASQ>
__device__ __forceinline__ void ms_triangle(const MsNode& P0, const MsNode& P1, const MsNode& P2, double (&acc)[MS_NQ], unsigned& ndeg)
{
#pragma clang fp contract(off)
    const double e1x = P1.x - P0.x, e1y = P1.y - P0.y, e1z = P1.z - P0.z;
    const double e2x = P2.x - P0.x, e2y = P2.y - P0.y, e2z = P2.z - P0.z;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double a = 0.5 * __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
    const double cx = P1.y * P2.z - P1.z * P2.y, cy = P1.z * P2.x - P1.x * P2.z, cz = P1.x * P2.y - P1.y * P2.x;
    const double v = ((P0.x * cx + P0.y * cy) + P0.z * cz) / 6.0;
    auto moment = [](double n, double a0, double a1, double a2) {
#pragma clang fp contract(off)
        const double s01 = a0 + a1, s12 = a1 + a2, s20 = a2 + a0;
        return (n * ((s01 * s01 + s12 * s12) + s20 * s20)) / 48.0;
    };
    auto mean = [](double a0, double a1, double a2) {
#pragma clang fp contract(off)
        return ((a0 + a1) + a2) / 3.0;
    };
    acc[0] = acc[0] + a;
    acc[1] = acc[1] + v;
    acc[2] = acc[2] + moment(nx, P0.x, P1.x, P2.x);
    acc[3] = acc[3] + moment(ny, P0.y, P1.y, P2.y);
    acc[4] = acc[4] + moment(nz, P0.z, P1.z, P2.z);
    acc[5] = acc[5] + a * mean(P0.x, P1.x, P2.x);
    acc[6] = acc[6] + a * mean(P0.y, P1.y, P2.y);
    acc[7] = acc[7] + a * mean(P0.z, P1.z, P2.z);
    if constexpr (HASQ) acc[8] = acc[8] + a * mean(P0.q, P1.q, P2.q);
    ndeg += a == 0.0 ? 1u : 0u;
}

// corner byte of the cell at `phi` (bit x + 2y + 4z: that corner is inside, f < 0) and the corners whose f is not finite
__device__ __forceinline__ void ms_corners(const double* __restrict__ phi, long rs, long ps, double iso, unsigned& byte, unsigned& nonf)
{
#pragma clang fp contract(off)
    byte = nonf = 0u;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const double f = phi[(o & 1) + rs * ((o >> 1) & 1) + ps * ((o >> 2) & 1)] - iso;
        byte |= (f < 0.0 ? 1u : 0u) << o;
        nonf |= (__builtin_isfinite(f) ? 0u : 1u) << o;
    }
}

// Validation: crossed edges of measured cells with a non-finite endpoint, counted once per measured cell that holds them.
template <bool HASQ>
__global__ __launch_bounds__(MB_CH) void k_measure_check(const double* __restrict__ phi, const double* __restrict__ q, const int* __restrict__ L,
                                                         int nL, int nx, int ny, double iso, unsigned long long* __restrict__ ctl)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long badf = 0ull, badq = 0ull;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
        unsigned byte, nonf;
        ms_corners(phi + p, rs, ps, iso, byte, nonf);
        if (byte != 0u && byte != 255u) {
            unsigned nonq = 0u;
            if constexpr (HASQ) {
#pragma unroll
                for (int o = 0; o < 8; ++o)
                    nonq |= (__builtin_isfinite(q[p + (o & 1) + rs * ((o >> 1) & 1) + ps * ((o >> 2) & 1)]) ? 0u : 1u) << o;
            }
            // the 19 edges of the six tetrahedra: corner offsets u < v with the bits of u among those of v
#pragma unroll
            for (unsigned v = 1u; v < 8u; ++v)
#pragma unroll
                for (unsigned u = 0u; u < v; ++u) {
                    if ((u & v) != u) continue;
                    const unsigned crossed = ((byte >> u) ^ (byte >> v)) & 1u;
                    badf += crossed & ((nonf >> u) | (nonf >> v));
                    badq += crossed & ((nonq >> u) | (nonq >> v));
                }
        }
    }
    badf = wave_usum(badf);
    badq = wave_usum(badq);
    if ((threadIdx.x & 63) == 0) {
        if (badf) atomicAdd(&ctl[MS_BAD_F], badf);
        if (badq) atomicAdd(&ctl[MS_BAD_Q], badq);
    }
}

// List cell e of chunk blockIdx.x.  part: MS_NQ doubles per block; cnt: MS_NCNT words per block.
template <bool HASQ, bool HASCELL>
__global__ __launch_bounds__(MB_CH) void k_measure_band(const double* __restrict__ phi, const int32_t* __restrict__ mask,
                                                        const double* __restrict__ q, double* __restrict__ cell_area,
                                                        const int* __restrict__ L, int nL, int nx, int ny, int nz, double dx, double x0, double y0,
                                                        double z0, double iso, const unsigned long long* __restrict__ ctl,
                                                        double* __restrict__ part, unsigned long long* __restrict__ cnt)
{
#pragma clang fp contract(off)
    __shared__ double red[MB_CH / 64][MS_NQ];
    __shared__ unsigned long long redc[MB_CH / 64][MS_NCNT];
    if (ctl[MS_BAD_F] | ctl[MS_BAD_Q]) return; // refused by the validation pass: nothing is written
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    double acc[MS_NQ];
#pragma unroll
    for (int m = 0; m < MS_NQ; ++m) acc[m] = 0.0;
    unsigned long long ncross = 0ull, ntri = 0ull, nopen = 0ull, ndeg = 0ull;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
        const double* c = phi + p;
        unsigned byte, nonf;
        ms_corners(c, rs, ps, iso, byte, nonf);
        if (byte != 0u && byte != 255u) {
            int i, j, k;
            band_decode(p, nx, ny, i, j, k);
            const double* cq = HASQ ? q + p : nullptr;
            unsigned tris = 0u, deg = 0u;
            xs_cell_emit(
                byte, [&](unsigned u, unsigned v) { return ms_node<HASQ>(c, cq, rs, ps, i, j, k, u, v, iso, dx, x0, y0, z0); },
                [&](const MsNode& A, const MsNode& B, const MsNode& C) {
                    ms_triangle<HASQ>(A, B, C, acc, deg);
                    ++tris;
                });
            // OPEN: a face-neighbour cell whose lower corner is not in LIST
            const bool in = band_listed6(mask + p, i, j, k, nx, ny, nz, rs, ps);
            ncross = 1ull, ntri = tris, nopen = in ? 0ull : 1ull, ndeg = deg;
        }
        if constexpr (HASCELL) cell_area[p] = acc[0];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int m = 0; m < (HASQ ? MS_NQ : MS_NQ - 1); ++m) acc[m] = acc[m] + __shfl_xor(acc[m], o, 64);
    wave_usum_each(ncross, ntri, nopen, ndeg); // (lsf_block_reduce.hpp; the block level shares the barrier of the sums)
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int m = 0; m < MS_NQ; ++m) red[w][m] = acc[m];
        redc[w][0] = ncross, redc[w][1] = ntri, redc[w][2] = nopen, redc[w][3] = ndeg;
    }
    __syncthreads();
    if (threadIdx.x < MS_NQ) {
        double t = red[0][threadIdx.x];
        for (int w = 1; w < MB_CH / 64; ++w) t = t + red[w][threadIdx.x];
        part[(size_t)blockIdx.x * MS_NQ + threadIdx.x] = t;
    } else if (threadIdx.x < MS_NQ + MS_NCNT) {
        const int m = threadIdx.x - MS_NQ;
        unsigned long long t = redc[0][m];
        for (int w = 1; w < MB_CH / 64; ++w) t += redc[w][m];
        cnt[(size_t)blockIdx.x * MS_NCNT + m] = t;
    }
}

} // namespace lsf
