// lsf_cut_cells_band.hpp -- what an embedded-boundary solver needs of every cell of a caller's mask: the volume fraction inside the
// body phi < iso, the apertures of its lower faces and the surface's area vector: lsf_cut_cells_band (include/lsf.h).
//
// The list is lsf_reinit_band's, built by the same machinery (band_list_count<true> / band_list_sort); a list point names the cell
// whose lower corner it is.  After k_measure_check<false> of lsf_measure_band.hpp, launched unchanged (the five edges of every face
// triangle are among the 19 it looks at), ONE plain launch over the list, one lane per list cell, MB_CH consecutive entries per
// block, modelled on k_measure_band:
//   k_cut_cells_band  returns at once when ctl holds a count (nothing is written then: the host refuses the call).  Otherwise a lane
//                     gathers its 8 corners with ms_corners and leaves with the constants of the header when the corner byte is 0
//                     or 255.  A cut cell walks its triangles with xs_cell_emit of lsf_extract_surface.hpp, used unchanged, with
//                     nodes in CELL UNITS (ms_node with the lower corner at the origin and dx = 1), adds 0.5 n and P0 . (P1 x P2) / 6
//                     per triangle in emission order, and evaluates the six face formulas.  An edge fraction is computed where it
//                     is used: its two endpoints are read again (L1 hits: the lane has just gathered them), so no array is indexed
//                     by a run-time value and nothing spills.  Which outputs are given is a template flag per group.
// Reduction (lsf_block_reduce.hpp): the stored fraction of a lane's cell is added over the wave by an xor butterfly (every lane of
// a pair forms the same sum, so the pattern is fixed), the four wave sums in wave order through LDS; the smallest stored fraction of
// the cut cells is a minimum of bit patterns (the fractions are >= +0.0: order-free); four integer counts.  Per block one fp64
// partial, one 64-bit key and four counts; the host adds the blocks in block order.  Plain launches, no floating-point atomic, no
// block waits for another: the totals are a function of field, mask and list order alone.
//
// Bounds: lsf_band_cell.hpp.  What is this file's own: a list entry is an interior point, so i + 1 <= nx, j + 1 <= ny, k + 1 <= nz
// and the eight corners p + {0,1} + {0,1}*row + {0,1}*plane exist -- every read of phi here is at one of them, with a corner offset
// 0..7 (a vertex of a Kuhn tetrahedron or of a face triangle); the OPEN test is band_listed6.  The stores, at most seven, are at
// the lane's own point; the block's partials go to index blockIdx.x of arrays the host sized by the grid of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_measure_band.hpp"

namespace lsf {

constexpr int CC_NCNT = 4; // integer partials per block: cut cells, full cells, open cut cells, clamped cut cells

// s(m, j): the fraction of the edge from corner m to the zero crossing on the edge {m, j} of the cell at `phi` -- the node's own
// t = fa / (fa - fb) from the lower endpoint when m is that endpoint, 1.0 - t otherwise
__device__ __forceinline__ double cc_edge(const double* __restrict__ phi, long rs, long ps, double iso, unsigned m, unsigned j)
{
#pragma clang fp contract(off)
    const unsigned u = m < j ? m : j, v = m < j ? j : m;
    const double fa = phi[(long)(u & 1u) + rs * (long)((u >> 1) & 1u) + ps * (long)((u >> 2) & 1u)] - iso;
    const double fb = phi[(long)(v & 1u) + rs * (long)((v >> 1) & 1u) + ps * (long)((v >> 2) & 1u)] - iso;
    const double t = fa / (fa - fb);
    return m == u ? t : 1.0 - t;
}

// the inside fraction of the face triangle with the corner offsets a, b, c and linear f
__device__ __forceinline__ double cc_tri(const double* __restrict__ phi, long rs, long ps, double iso, unsigned byte, unsigned a, unsigned b,
                                         unsigned c)
{
#pragma clang fp contract(off)
    const unsigned ia = (byte >> a) & 1u, ib = (byte >> b) & 1u, ic = (byte >> c) & 1u, nin = ia + ib + ic;
    if (nin == 0u) return 0.0;
    if (nin == 3u) return 1.0;
    // the vertex alone on its side, and the two others in the triangle's order
    const unsigned lone = nin == 1u ? 1u : 0u;
    const unsigned m = ia == lone ? a : (ib == lone ? b : c);
    const unsigned o1 = ia == lone ? b : a, o2 = ic == lone ? b : c;
    const double r = cc_edge(phi, rs, ps, iso, m, o1) * cc_edge(phi, rs, ps, iso, m, o2);
    return nin == 1u ? r : 1.0 - r;
}

// the aperture of the face normal to axis A at base in {0, 1 << A}, cut along the Kuhn diagonal base - base|b|c (B < C the other axes)
template <int A>
__device__ __forceinline__ double cc_face(const double* __restrict__ phi, long rs, long ps, double iso, unsigned byte, unsigned base)
{
#pragma clang fp contract(off)
    constexpr unsigned b = A == 0 ? 2u : 1u, c = A == 2 ? 2u : 4u;
    return 0.5 * (cc_tri(phi, rs, ps, iso, byte, base, base | b, base | b | c) + cc_tri(phi, rs, ps, iso, byte, base, base | c, base | b | c));
}

// List cell e of chunk blockIdx.x.  part: one double per block; key: one word per block; cnt: CC_NCNT words per block.
template <bool HASVOF, bool HASA, bool HASB>
__global__ __launch_bounds__(MB_CH) void k_cut_cells_band(const double* __restrict__ phi, const int32_t* __restrict__ mask, double* __restrict__ vof,
                                                          double* __restrict__ ax, double* __restrict__ ay, double* __restrict__ az,
                                                          double* __restrict__ bx, double* __restrict__ by, double* __restrict__ bz,
                                                          const int* __restrict__ L, int nL, int nx, int ny, int nz, double iso,
                                                          const unsigned long long* __restrict__ ctl, double* __restrict__ part,
                                                          unsigned long long* __restrict__ key, unsigned long long* __restrict__ cnt)
{
#pragma clang fp contract(off)
    __shared__ double red[MB_CH / 64];
    __shared__ unsigned long long redk[MB_CH / 64];
    __shared__ unsigned long long redc[MB_CH / 64][CC_NCNT];
    if (ctl[MS_BAD_F]) return; // refused by the validation pass: nothing is written
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    double sum = 0.0;
    unsigned long long kmin = 0x7ff0000000000000ull; // +inf: a lane without a cut cell
    unsigned long long ncut = 0ull, nfull = 0ull, nopen = 0ull, nclamp = 0ull;
    if (e < nL) {
        const unsigned p = (unsigned)L[e];
        const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
        const double* c = phi + p;
        unsigned byte, nonf;
        ms_corners(c, rs, ps, iso, byte, nonf);
        double v = byte == 255u ? 1.0 : 0.0, a0 = v, a1 = v, a2 = v, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        if (byte != 0u && byte != 255u) {
            double V = 0.0;
            xs_cell_emit(
                byte, [&](unsigned u, unsigned w) { return ms_node<false>(c, nullptr, rs, ps, 0, 0, 0, u, w, iso, 1.0, 0.0, 0.0, 0.0); },
                [&](const MsNode& P0, const MsNode& P1, const MsNode& P2) {
#pragma clang fp contract(off)
                    if constexpr (HASB) {
                        const double e1x = P1.x - P0.x, e1y = P1.y - P0.y, e1z = P1.z - P0.z;
                        const double e2x = P2.x - P0.x, e2y = P2.y - P0.y, e2z = P2.z - P0.z;
                        b0 = b0 + 0.5 * (e1y * e2z - e1z * e2y);
                        b1 = b1 + 0.5 * (e1z * e2x - e1x * e2z);
                        b2 = b2 + 0.5 * (e1x * e2y - e1y * e2x);
                    }
                    const double cx = P1.y * P2.z - P1.z * P2.y, cy = P1.z * P2.x - P1.x * P2.z, cz = P1.x * P2.y - P1.y * P2.x;
                    V = V + ((P0.x * cx + P0.y * cy) + P0.z * cz) / 6.0;
                });
            // the divergence theorem about c0: the lower faces contribute nothing
            const double ux = cc_face<0>(c, rs, ps, iso, byte, 1u), uy = cc_face<1>(c, rs, ps, iso, byte, 2u), uz = cc_face<2>(c, rs, ps, iso, byte, 4u);
            const double raw = ((ux + uy) + uz) / 3.0 + V;
            v = raw < 0.0 ? 0.0 : (raw > 1.0 ? 1.0 : raw);
            if constexpr (HASA) a0 = cc_face<0>(c, rs, ps, iso, byte, 0u), a1 = cc_face<1>(c, rs, ps, iso, byte, 0u), a2 = cc_face<2>(c, rs, ps, iso, byte, 0u);
            int i, j, k;
            band_decode(p, nx, ny, i, j, k);
            // OPEN: a face-neighbour cell whose lower corner is not in LIST
            const bool in = band_listed6(mask + p, i, j, k, nx, ny, nz, rs, ps);
            ncut = 1ull, nopen = in ? 0ull : 1ull, nclamp = (raw < 0.0 || raw > 1.0) ? 1ull : 0ull;
            kmin = (unsigned long long)__double_as_longlong(v);
        }
        nfull = byte == 255u ? 1ull : 0ull;
        sum = v;
        if constexpr (HASVOF) vof[p] = v;
        if constexpr (HASA) ax[p] = a0, ay[p] = a1, az[p] = a2;
        if constexpr (HASB) bx[p] = b0, by[p] = b1, bz[p] = b2;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum = sum + __shfl_xor(sum, o, 64);
    kmin = wave_umin(kmin);
    wave_usum_each(ncut, nfull, nopen, nclamp); // (lsf_block_reduce.hpp; the block level shares the barrier of the sum)
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[w] = sum, redk[w] = kmin;
        redc[w][0] = ncut, redc[w][1] = nfull, redc[w][2] = nopen, redc[w][3] = nclamp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        unsigned long long q = redk[0];
        for (int w = 1; w < MB_CH / 64; ++w) t = t + red[w], q = redk[w] < q ? redk[w] : q;
        part[blockIdx.x] = t, key[blockIdx.x] = q;
    } else if (threadIdx.x <= CC_NCNT) {
        const int m = threadIdx.x - 1;
        unsigned long long t = redc[0][m];
        for (int w = 1; w < MB_CH / 64; ++w) t += redc[w][m];
        cnt[(size_t)blockIdx.x * CC_NCNT + m] = t;
    }
}

} // namespace lsf
