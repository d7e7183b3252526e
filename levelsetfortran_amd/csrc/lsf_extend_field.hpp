// lsf_extend_field.hpp -- a quantity q carried off the frozen set constant along the normals of phi (grad q . grad phi = 0, first-order
// upwind in |phi|, fast sweeping): lsf_extend_field.  No reference counterpart.  Contract: include/lsf.h; account: DESIGN.md section
// 4.14; driver: lsf_host_extend_field.hpp.  The schedule, the frozen words and the LDS layout are those of lsf_distance_fill.hpp
// (DfGrid and the DF_ constants are shared by inclusion); the kernels are new.
//   k_ext_check       read-only: builds the frozen words (bit set = FROZEN or outside the grid), counts frozen points, non-finite
//                     frozen q and non-finite phi.  The host decides the errors before anything is written.
//   k_ext_init        every other point of q becomes NaN: UNKNOWN.
//   k_ext_tile_plane  one raster sweep, tile plane by tile plane, one wave per tile, exactly as k_df_tile_plane: a visit reads the
//                     six axis neighbours only, so the tiles of one plane share no operand and the in-tile hyperplane march gives
//                     every cell the operands of the serial raster order.  Two LDS images with face halos: f = |phi| (+inf outside the
//                     grid; never written) and q (NaN outside).  A tile without a live cell returns before it loads; a tile that
//                     changed nothing stores nothing.
//   k_ext_count       the non-frozen points that hold a value / are still NaN.
// LDS: 2 images x 361 x 10 doubles = 57 760 B + 256 B of row words: under the 64 KB static limit, two tiles per CU.  A step issues 7
// ds_read_b64 on f and 7 on q; both images have the pitches of lsf_distance_fill.hpp, so each read is conflict-free by its argument.
#pragma once
#include "lsf_distance_fill.hpp"

namespace lsf {

constexpr int EXT_IMG = DF_PXY * (DF_TZ + 2); // doubles of one LDS image

// counters of one call (64-bit words)
enum { EXT_N_FROZEN, EXT_N_BADQ, EXT_N_BADPHI, EXT_N_CHANGED, EXT_N_REACHED, EXT_N_UNREACHED, EXT_N_COUNTERS };

// One axis of a visit: the neighbour with the smaller f, the one at the lower index on a tie; its weight and weighted value, both 0
// when the axis is not used.
__device__ __forceinline__ void ext_axis(double fp, double f_lo, double f_hi, double q_lo, double q_hi, double* s, double* t)
{
#pragma clang fp contract(off)
    const bool hi = f_hi < f_lo;
    const double fn = hi ? f_hi : f_lo, qn = hi ? q_hi : q_lo;
    const double w = fp - fn;
    const bool used = w > 0.0 && qn == qn;
    *s = used ? w : 0.0;
    *t = used ? w * qn : 0.0;
}

// A 32-lane half of a wave per word.  mask == nullptr: frozen = |phi| < far.
__global__ __launch_bounds__(256) void k_ext_check(const double* __restrict__ q, const double* __restrict__ phi, const int32_t* __restrict__ mask,
                                                   DfGrid g, double far, long long nwords, uint32_t* __restrict__ words,
                                                   unsigned long long* __restrict__ counters)
{
    const long long w = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    unsigned nfz = 0, nbq = 0, nbp = 0;
    bool bit = true;
    if (w < nwords) {
        const int tA = (int)(w % g.nTA);
        const long long row = w / g.nTA;
        const int i = tA * DF_TX + (threadIdx.x & 31);
        if (i < g.NX) {
            const size_t p = (size_t)i + (size_t)g.NX * (size_t)row;
            const double v = phi[p];
            const bool fz = mask ? mask[p] == 1 : fabs(v) < far;
            bit = fz;
            nfz = fz;
            nbp = !isfinite(v);
            nbq = fz && !isfinite(q[p]);
        }
    }
    const unsigned long long bal = __ballot(bit);
    if (w < nwords && (threadIdx.x & 31) == 0) words[w] = (uint32_t)(bal >> (threadIdx.x & 32));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nfz += __shfl_down(nfz, off);
        nbq += __shfl_down(nbq, off);
        nbp += __shfl_down(nbp, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nfz) atomicAdd(counters + EXT_N_FROZEN, (unsigned long long)nfz);
        if (nbq) atomicAdd(counters + EXT_N_BADQ, (unsigned long long)nbq);
        if (nbp) atomicAdd(counters + EXT_N_BADPHI, (unsigned long long)nbp);
    }
}

__global__ __launch_bounds__(256) void k_ext_init(double* __restrict__ q, DfGrid g, long long nwords, const uint32_t* __restrict__ words)
{
    const long long w = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (w >= nwords) return;
    const int l = threadIdx.x & 31;
    if ((words[w] >> l) & 1u) return; // frozen, or past the end of the row
    const int tA = (int)(w % g.nTA);
    const long long row = w / g.nTA;
    q[(size_t)(tA * DF_TX + l) + (size_t)g.NX * (size_t)row] = __builtin_nan("");
}

__global__ __launch_bounds__(256) void k_ext_count(const double* __restrict__ q, DfGrid g, long long nwords, const uint32_t* __restrict__ words,
                                                   unsigned long long* __restrict__ counters)
{
    const long long w = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    unsigned nval = 0, nnan = 0;
    if (w < nwords) {
        const int l = threadIdx.x & 31;
        if (!((words[w] >> l) & 1u)) { // live: inside the grid and not frozen
            const int tA = (int)(w % g.nTA);
            const long long row = w / g.nTA;
            const double v = q[(size_t)(tA * DF_TX + l) + (size_t)g.NX * (size_t)row];
            nval = v == v;
            nnan = !(v == v);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nval += __shfl_down(nval, off);
        nnan += __shfl_down(nnan, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nval) atomicAdd(counters + EXT_N_REACHED, (unsigned long long)nval);
        if (nnan) atomicAdd(counters + EXT_N_UNREACHED, (unsigned long long)nnan);
    }
}

// The tile at (x0, y0, z0) and its six face halos into the two LDS images, by the whole wave: f = |phi| (+inf outside the grid) and
// q (NaN outside).  The loads themselves are unconditional -- an outside point loads the tile's own first point, which lies inside
// the grid; its own offset is formed but never used as an address -- so the 2 x 8 loads of a group go out together and the two
// fields share their latencies.
__device__ __forceinline__ void ext_load_images(const double* __restrict__ phi, const double* q, double* s_f, double* s_q, const DfGrid& g, int x0,
                                                int y0, int z0, int lane)
{
    const size_t py = (size_t)g.NX, pz = py * (size_t)g.NY;
    const size_t p0 = (size_t)x0 + py * (size_t)y0 + pz * (size_t)z0;
    auto val = [&](int i, int j, int k, double* f, double* v) {
        const bool in = i >= 0 && i < g.NX && j >= 0 && j < g.NY && k >= 0 && k < g.NZ;
        const size_t p = in ? (size_t)i + py * (size_t)j + pz * (size_t)k : p0;
        const double a = phi[p], b = q[p];
        *f = in ? fabs(a) : HUGE_VAL;
        *v = in ? b : __builtin_nan("");
    };
    const int half = lane >> 5, i = lane & 31;
    constexpr int G = 8; // points in flight per lane: a group is loaded into registers first, then stored to LDS
    double f[G], v[G];
    // the tile, two rows per step
#pragma unroll 1
    for (int it0 = 0; it0 < DF_ROWS / 2; it0 += G) {
#pragma unroll
        for (int m = 0; m < G; ++m) {
            const int r = 2 * (it0 + m) + half;
            val(x0 + i, y0 + (r & 7), z0 + (r >> 3), &f[m], &v[m]);
        }
#pragma unroll
        for (int m = 0; m < G; ++m) {
            const int r = 2 * (it0 + m) + half, o = ((r >> 3) + 1) * DF_PXY + ((r & 7) + 1) * DF_PX + i + 1;
            s_f[o] = f[m], s_q[o] = v[m];
        }
    }
    // the y and z face halos, 2 x 8 rows each (side 0: below, 1: above), and the x face halos, one point per row and side
    double wf[2 * G + 2], wv[2 * G + 2];
    const int rj = lane & 7, rk = lane >> 3;
#pragma unroll
    for (int it = 0; it < G; ++it) {
        const int r = 2 * it + half, m = r & 7, side = r >> 3;
        val(x0 + i, side ? y0 + DF_TY : y0 - 1, z0 + m, &wf[2 * it], &wv[2 * it]);
        val(x0 + i, y0 + m, side ? z0 + DF_TZ : z0 - 1, &wf[2 * it + 1], &wv[2 * it + 1]);
    }
    val(x0 - 1, y0 + rj, z0 + rk, &wf[2 * G], &wv[2 * G]);
    val(x0 + DF_TX, y0 + rj, z0 + rk, &wf[2 * G + 1], &wv[2 * G + 1]);
#pragma unroll
    for (int it = 0; it < G; ++it) {
        const int r = 2 * it + half, m = r & 7, side = r >> 3;
        const int oy = (m + 1) * DF_PXY + (side ? DF_TY + 1 : 0) * DF_PX + i + 1, oz = (side ? DF_TZ + 1 : 0) * DF_PXY + (m + 1) * DF_PX + i + 1;
        s_f[oy] = wf[2 * it], s_q[oy] = wv[2 * it];
        s_f[oz] = wf[2 * it + 1], s_q[oz] = wv[2 * it + 1];
    }
    const int ox = (rk + 1) * DF_PXY + (rj + 1) * DF_PX;
    s_f[ox] = wf[2 * G], s_q[ox] = wv[2 * G];
    s_f[ox + DF_TX + 1] = wf[2 * G + 1], s_q[ox + DF_TX + 1] = wv[2 * G + 1];
}

// One wave per tile of the plane A + B + C = P of the frame reflected by (sx, sy, sz); block x = B + nTB * C.
__global__ __launch_bounds__(DF_ROWS) void k_ext_tile_plane(double* q, const double* __restrict__ phi, const uint32_t* __restrict__ words, DfGrid g,
                                                            int P, int sx, int sy, int sz, unsigned long long* __restrict__ counters)
{
    __shared__ double s_f[EXT_IMG], s_q[EXT_IMG];
    __shared__ uint32_t s_fz[DF_ROWS];
    const int B = (int)(blockIdx.x % (unsigned)g.nTB), C = (int)(blockIdx.x / (unsigned)g.nTB);
    const int A = P - B - C;
    if (A < 0 || A >= g.nTA) return;
    const int tA = sx > 0 ? A : g.nTA - 1 - A, tB = sy > 0 ? B : g.nTB - 1 - B, tC = sz > 0 ? C : g.nTC - 1 - C;
    const int x0 = tA * DF_TX, y0 = tB * DF_TY, z0 = tC * DF_TZ;
    const int lane = threadIdx.x;

    // the row this lane marches: (b, c) in the frame, (jj, kk) in the tile
    const int b = lane & 7, c = lane >> 3;
    const int jj = sy > 0 ? b : DF_TY - 1 - b, kk = sz > 0 ? c : DF_TZ - 1 - c;
    uint32_t fw = ~0u;
    if (y0 + jj < g.NY && z0 + kk < g.NZ) fw = words[(size_t)tA + (size_t)g.nTA * ((size_t)(y0 + jj) + (size_t)g.NY * (size_t)(z0 + kk))];
    if (__ballot(fw != ~0u) == 0ull) return; // no live cell in this tile
    s_fz[jj + DF_TY * kk] = fw;
    ext_load_images(phi, q, s_f, s_q, g, x0, y0, z0, lane);
    __syncthreads();

    unsigned cnt = 0;
    const int ro = (kk + 1) * DF_PXY + (jj + 1) * DF_PX + 1;
    const double* rf = s_f + ro;
    double* rq = s_q + ro;
#pragma unroll 1
    for (int p = 0; p < DF_STEPS; ++p) {
        const int a = p - b - c;
        if (a >= 0 && a < DF_TX) {
            const int ii = sx > 0 ? a : DF_TX - 1 - a;
            if (!((fw >> ii) & 1u)) {
#pragma clang fp contract(off)
                const double* f = rf + ii;
                double* v = rq + ii;
                const double fp = f[0], old = v[0];
                double s0, s1, s2, t0, t1, t2;
                ext_axis(fp, f[-1], f[1], v[-1], v[1], &s0, &t0);
                ext_axis(fp, f[-DF_PX], f[DF_PX], v[-DF_PX], v[DF_PX], &s1, &t1);
                ext_axis(fp, f[-DF_PXY], f[DF_PXY], v[-DF_PXY], v[DF_PXY], &s2, &t2);
                const double den = (s0 + s1) + s2;
                if (den != 0.0) {
                    const double nw = ((t0 + t1) + t2) / den;
                    if (!(nw == old)) {
                        v[0] = nw;
                        ++cnt;
                    }
                }
            }
        }
        __syncthreads(); // one wave: orders this step's LDS stores before the next step's loads
    }

    if (__ballot(cnt != 0) == 0ull) return; // nothing changed: the tile in memory is already what LDS holds
    {
        const size_t py = (size_t)g.NX, pz = py * (size_t)g.NY;
        const int half = lane >> 5, i = lane & 31;
#pragma unroll 8
        for (int it = 0; it < DF_ROWS / 2; ++it) {
            const int r = 2 * it + half, rj = r & 7, rk = r >> 3;
            if (!((s_fz[r] >> i) & 1u)) // live: inside the grid and not frozen
                q[(size_t)(x0 + i) + py * (size_t)(y0 + rj) + pz * (size_t)(z0 + rk)] = s_q[(rk + 1) * DF_PXY + (rj + 1) * DF_PX + i + 1];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane == 0) atomicAdd(counters + EXT_N_CHANGED, (unsigned long long)cnt);
}

} // namespace lsf
