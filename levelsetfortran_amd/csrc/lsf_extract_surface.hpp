// lsf_extract_surface.hpp -- the iso-surface of a field as an indexed triangle mesh: lsf_extract_surface (include/lsf.h).
//
// Marching tetrahedra on the six Kuhn tetrahedra of every cell (no reference counterpart, no 256-entry table, no ambiguous case).
// Every tetrahedron edge runs from a grid point a to a + d, d in {0,1}^3 \ {0}: seven edge types per point, one node per crossed
// edge, numbered by 7 * p + type.  Three steps, plain launches only -- no block waits for another, no look-back, no spin:
//   k_extract_count    one lane per grid point, 64 consecutive lanes along x, 4 rows per block, a march of XS_KC planes along z
//                      that carries the previous plane's four sign bits (four loads per point instead of eight): the corner byte
//                      of the cell whose lower corner the point is, and the point's 7-bit crossed-edge mask.  Both are stored
//                      (2 bytes per point); crossed cells and crossed edges with a non-finite endpoint are counted.
//   k_extract_sums     per tile of XS_TILE consecutive points (linear order) the nodes and triangles it owns;
//   k_extract_scan     ONE block walks the tile sums XS_SCAN_T at a time with a running carry: exclusive tile offsets and the totals;
//   k_extract_scatter  per point the exclusive offsets of its nodes and of its cell's triangles (2 x 4 bytes per point).
//   k_extract_emit     one lane per point: its nodes go to their slots; its cell's triangles look a node up as
//                      offset[base point] + popcount(mask[base point] & lower types).  Cells with corner byte 0 or 255 leave at once.
// Counts are integers and every slot is a function of the field alone: nodes, connectivity and counts are the same from run to
// run and on any stream.
//
// Bounds: a lane exists only for i <= nx, j <= ny; it forms the offsets +1, +row, +plane only where
// i < nx, j < ny, k < nz respectively, and a mask bit is set only where the far endpoint exists, so whatever follows a mask bit or a
// non-zero corner byte addresses existing points only.  The linear kernels guard p < n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_block_reduce.hpp"

namespace lsf {

constexpr int XS_BX = 64, XS_BY = 4; // a block of k_extract_count: 64 points along x by 4 rows
constexpr int XS_KC = 32;            // planes it marches (tests/test_gpu_extract_surface.py has a grid longer than two of these)
constexpr int XS_T = 256, XS_PER = 4, XS_TILE = XS_T * XS_PER; // linear kernels: 1024 consecutive points per block
constexpr int XS_SCAN_T = 1024;      // tile sums one pass of k_extract_scan takes: beyond 1024 * 1024 points it walks more than one
// ctl words (unsigned long long): totals and counters of one call
enum { XS_NODES = 0, XS_TRIS = 1, XS_CELLS = 2, XS_BAD = 3, XS_T1 = 4, XS_CTL_LEN = 8 };

// corners of tetrahedron 0..5 (axis orders xyz, xzy, yxz, yzx, zxy, zyx) as offsets x + 2y + 4z: v0 = 0, v1, v2, v3 = 7
__host__ __device__ __forceinline__ unsigned xs_tet_v1(int t) { return (0x442211u >> (4 * t)) & 0xfu; }
__host__ __device__ __forceinline__ unsigned xs_tet_v2(int t) { return (0x656353u >> (4 * t)) & 0xfu; }
// parity of the axis order: tetrahedra 1, 2, 5 are the odd permutations
__host__ __device__ __forceinline__ bool xs_tet_negative(int t) { return (0x26u >> t) & 1u; }

// triangles of a cell from its corner byte (bit x + 2y + 4z set: that corner is inside)
__host__ __device__ __forceinline__ unsigned xs_cell_triangles(unsigned byte)
{
    if (byte == 0u || byte == 255u) return 0u;
    unsigned n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned in = __builtin_popcount(byte & (0x81u | (1u << xs_tet_v1(t)) | (1u << xs_tet_v2(t))));
        n += in == 2u ? 2u : (in == 1u || in == 3u ? 1u : 0u);
    }
    return n;
}

// The triangles of one crossed cell, in the order (tetrahedron 0..5, triangle 0..1).  node(u, v): the node on the edge between the
// corner offsets u < v (x + 2y + 4z); put(a, b, c): the next triangle.  The rule of include/lsf.h, for a tetrahedron with vertices
// v0..v3 and parity `neg`:
//   one vertex m alone on its side (1 or 3 inside), the others a < b < c: (ma, mb, mc), the last two swapped when
//       neg xor (m odd) xor (3 inside);
//   two inside p < q, two outside r < s: (pr, ps, qs) and (pr, qs, qr), the last two of each swapped when neg xor (p + q even).
template <class NodeFn, class PutFn>
__host__ __device__ __forceinline__ void xs_cell_emit(unsigned byte, NodeFn node, PutFn put)
{
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned v1 = xs_tet_v1(t), v2 = xs_tet_v2(t);
        const unsigned code = (byte & 1u) | (((byte >> v1) & 1u) << 1) | (((byte >> v2) & 1u) << 2) | (((byte >> 7) & 1u) << 3);
        const unsigned nin = __builtin_popcount(code);
        if (nin == 0u || nin == 4u) continue;
        const bool neg = xs_tet_negative(t);
        auto off = [&](unsigned m) { return m == 0u ? 0u : (m == 1u ? v1 : (m == 2u ? v2 : 7u)); };
        auto E = [&](unsigned u, unsigned v) { return u < v ? node(off(u), off(v)) : node(off(v), off(u)); };
        if (nin == 2u) {
            const unsigned P = __builtin_ctz(code), Q = 31u - __builtin_clz(code);
            const unsigned nc = ~code & 0xfu, R = __builtin_ctz(nc), S = 31u - __builtin_clz(nc);
            const bool flip = neg != (((P + Q) & 1u) == 0u);
            const auto pr = E(P, R), ps = E(P, S), qs = E(Q, S), qr = E(Q, R);
            if (flip) put(pr, qs, ps), put(pr, qr, qs);
            else put(pr, ps, qs), put(pr, qs, qr);
        } else {
            const unsigned m = __builtin_ctz(nin == 1u ? code : (~code & 0xfu));
            const unsigned a = m == 0u ? 1u : 0u, b = m <= 1u ? 2u : 1u, c = m == 3u ? 2u : 3u;
            const bool flip = (neg != ((m & 1u) != 0u)) != (nin == 3u);
            if (flip) put(E(m, a), E(m, c), E(m, b));
            else put(E(m, a), E(m, b), E(m, c));
        }
    }
}

// coordinate A of a node: xLo[A] + ((double)i_A + t) * dx along the edge, xLo[A] + (double)i_A * dx across it; as written
__host__ __device__ __forceinline__ double xs_coord(double lo, int iA, bool along, double t, double dx)
{
#pragma clang fp contract(off)
    return along ? lo + ((double)iA + t) * dx : lo + (double)iA * dx;
}

// One point from the bits of its two planes (bits 0..3: f < 0 at (i,j), (i+1,j), (i,j+1), (i+1,j+1); bits 4..7: f not finite there;
// an absent point contributes 0) and the neighbours that exist (ex: i < nx, ey: j < ny, ez: k < nz): the corner byte of its cell
// (0 for a point that owns none), its crossed-edge mask, and the crossed edges with a non-finite endpoint.
__host__ __device__ __forceinline__ void xs_classify(unsigned lowp, unsigned upp, bool ex, bool ey, bool ez, unsigned& mask, unsigned& cellByte,
                                                      unsigned& bad)
{
    const unsigned byte = (lowp & 0xfu) | ((upp & 0xfu) << 4);
    const unsigned nonf = (lowp >> 4) | (upp & 0xf0u);
    // edge types whose far endpoint exists: x is in types 0, 2, 4, 6; y in 1, 2, 5, 6; z in 3..6
    const unsigned exists = (ex ? 0x7fu : 0x2au) & (ey ? 0x7fu : 0x19u) & (ez ? 0x7fu : 0x07u);
    mask = ((byte >> 1) ^ ((byte & 1u) ? 0x7fu : 0u)) & exists;
    cellByte = (ex && ey && ez) ? byte : 0u;
    bad = (unsigned)__builtin_popcount(mask & ((nonf & 1u) ? 0x7fu : (nonf >> 1)));
}

// ---- classify and count ------------------------------------------------------------------------------------------------
// The launch is one-dimensional: block L = x block fastest, then y, then the chunks along z.
static __global__ __launch_bounds__(XS_BX* XS_BY) void k_extract_count(const double* __restrict__ phi, int nx, int ny, int nz, double iso,
                                                                        unsigned char* __restrict__ maskOut, unsigned char* __restrict__ byteOut,
                                                                        unsigned long long* __restrict__ ctl, int nbx, int nby)
{
    const unsigned L = blockIdx.x;
    const int bxi = (int)(L % (unsigned)nbx), byi = (int)((L / (unsigned)nbx) % (unsigned)nby), bzi = (int)(L / ((unsigned)nbx * (unsigned)nby));
    const int i = bxi * XS_BX + (int)threadIdx.x, j = byi * XS_BY + (int)threadIdx.y;
    const int k0 = bzi * XS_KC, k1 = min(k0 + XS_KC, nz + 1); // planes k0 .. k1-1 of the points 0 .. nz
    const long sx = nx + 1, sxy = (long)(nx + 1) * (ny + 1);
    unsigned long long cells = 0ull, bad = 0ull;
    if (i <= nx && j <= ny) {
        const bool ex = i < nx, ey = j < ny; // the neighbours +x, +y exist
        const long col = i + sx * j;
        // sign and non-finite bits of (i,j), (i+1,j), (i,j+1), (i+1,j+1) in plane q: bits 0..3 and 4..7; an absent point gives 0
        auto plane4 = [&](int q) -> unsigned {
            const double* P = phi + sxy * q + col;
            unsigned r = 0u;
            auto put = [&](double v, int b) {
                const double f = v - iso;
                r |= (f < 0.0 ? 1u : 0u) << b;
                r |= (__builtin_isfinite(f) ? 0u : 1u) << (b + 4);
            };
            put(P[0], 0);
            if (ex) put(P[1], 1);
            if (ey) put(P[sx], 2);
            if (ex && ey) put(P[sx + 1], 3);
            return r;
        };
        unsigned lowp = plane4(k0);
        for (int k = k0; k < k1; ++k) {
            const bool ez = k < nz;
            const unsigned upp = ez ? plane4(k + 1) : 0u;
            unsigned mask, byte, nbad;
            xs_classify(lowp, upp, ex, ey, ez, mask, byte, nbad);
            const long p = sxy * k + col;
            maskOut[p] = (unsigned char)mask;
            byteOut[p] = (unsigned char)byte;
            cells += (byte != 0u && byte != 255u) ? 1ull : 0ull;
            bad += nbad;
            lowp = upp;
        }
    }
    cells = wave_usum(cells);
    bad = wave_usum(bad);
    if (((threadIdx.x + XS_BX * threadIdx.y) & 63u) == 0u) {
        if (cells) atomicAdd(&ctl[XS_CELLS], cells);
        if (bad) atomicAdd(&ctl[XS_BAD], bad);
    }
}

// ---- exclusive prefix sums in linear order ---------------------------------------------------------------------------------
// exclusive scan of (a, b) over the threads of a block of NT threads; the block totals come back in ta, tb
template <int NT>
__device__ __forceinline__ void xs_block_scan(unsigned& a, unsigned& b, unsigned& ta, unsigned& tb, unsigned (*red)[2])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned ia = a, ib = b; // inclusive within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
        if (lane >= o) ia += ua, ib += ub;
    }
    if (lane == 63) red[w][0] = ia, red[w][1] = ib;
    __syncthreads();
    unsigned wa = 0u, wb = 0u;
    ta = tb = 0u;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) {
        if (q < w) wa += red[q][0], wb += red[q][1];
        ta += red[q][0], tb += red[q][1];
    }
    __syncthreads(); // red may be used again
    a = wa + ia - a;
    b = wb + ib - b;
}

static __global__ __launch_bounds__(XS_T) void k_extract_sums(const unsigned char* __restrict__ maskIn, const unsigned char* __restrict__ byteIn,
                                                              long n, uint2* __restrict__ sums)
{
    __shared__ unsigned red[XS_T / 64][2];
    const long p0 = (long)blockIdx.x * XS_TILE + (long)threadIdx.x * XS_PER;
    unsigned a = 0u, b = 0u;
#pragma unroll
    for (int q = 0; q < XS_PER; ++q)
        if (p0 + q < n) a += __builtin_popcount((unsigned)maskIn[p0 + q]), b += xs_cell_triangles(byteIn[p0 + q]);
    unsigned ta, tb;
    xs_block_scan<XS_T>(a, b, ta, tb, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(ta, tb);
}

// one block: the tile sums XS_SCAN_T at a time, the carry in registers (a pass holds at most 1024 * 12 * 1024 < 2^32)
static __global__ __launch_bounds__(XS_SCAN_T) void k_extract_scan(const uint2* __restrict__ sums, long nTiles, ulonglong2* __restrict__ tileOff,
                                                                   unsigned long long* __restrict__ ctl)
{
    __shared__ unsigned red[XS_SCAN_T / 64][2];
    unsigned long long ca = 0ull, cb = 0ull;
    for (long base = 0; base < nTiles; base += XS_SCAN_T) {
        const long q = base + threadIdx.x;
        unsigned a = 0u, b = 0u;
        if (q < nTiles) a = sums[q].x, b = sums[q].y;
        unsigned ta, tb;
        xs_block_scan<XS_SCAN_T>(a, b, ta, tb, red);
        if (q < nTiles) tileOff[q] = make_ulonglong2(ca + a, cb + b);
        ca += ta, cb += tb;
    }
    if (threadIdx.x == 0) ctl[XS_NODES] = ca, ctl[XS_TRIS] = cb;
}

// offsets are stored as 32-bit words: the host refuses totals above 2^31 - 1 before anything reads them
static __global__ __launch_bounds__(XS_T) void k_extract_scatter(const unsigned char* __restrict__ maskIn, const unsigned char* __restrict__ byteIn,
                                                                 long n, const ulonglong2* __restrict__ tileOff, uint32_t* __restrict__ nodeOff,
                                                                 uint32_t* __restrict__ triOff)
{
    __shared__ unsigned red[XS_T / 64][2];
    const long p0 = (long)blockIdx.x * XS_TILE + (long)threadIdx.x * XS_PER;
    unsigned ca[XS_PER], cb[XS_PER], a = 0u, b = 0u;
#pragma unroll
    for (int q = 0; q < XS_PER; ++q) {
        ca[q] = cb[q] = 0u;
        if (p0 + q < n) ca[q] = __builtin_popcount((unsigned)maskIn[p0 + q]), cb[q] = xs_cell_triangles(byteIn[p0 + q]);
        a += ca[q], b += cb[q];
    }
    unsigned ta, tb;
    xs_block_scan<XS_T>(a, b, ta, tb, red);
    const ulonglong2 base = tileOff[blockIdx.x];
    unsigned long long ra = base.x + a, rb = base.y + b;
#pragma unroll
    for (int q = 0; q < XS_PER; ++q) {
        if (p0 + q < n) nodeOff[p0 + q] = (uint32_t)ra, triOff[p0 + q] = (uint32_t)rb;
        ra += ca[q], rb += cb[q];
    }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------
// surfX(nn,3) and surfElem(nt,3) are Fortran-ordered; node and triangle numbers are 1-based in the output.
static __global__ __launch_bounds__(XS_T) void k_extract_emit(const double* __restrict__ phi, int nx, int ny, int nz, double dx, double x0, double y0,
                                                              double z0, double iso, const unsigned char* __restrict__ maskIn,
                                                              const unsigned char* __restrict__ byteIn, const uint32_t* __restrict__ nodeOff,
                                                              const uint32_t* __restrict__ triOff, double* __restrict__ surfX, long nn,
                                                              int32_t* __restrict__ surfElem, long nt, unsigned long long* __restrict__ ctl)
{
#pragma clang fp contract(off)
    const long n = (long)(nx + 1) * (ny + 1) * (nz + 1);
    const long p = (long)blockIdx.x * XS_T + threadIdx.x;
    const unsigned sx = (unsigned)(nx + 1), sy = (unsigned)(ny + 1);
    const long sxy = (long)sx * sy;
    unsigned long long t1 = 0ull;
    if (p < n) {
        const unsigned mask = maskIn[p], byte = byteIn[p];
        if (mask) { // the nodes this point owns: the far endpoint of a set bit exists (k_extract_count)
            const unsigned up = (unsigned)p;
            const int i = (int)(up % sx), j = (int)((up / sx) % sy), k = (int)(up / (sx * sy));
            const double fa = phi[p] - iso;
            long slot = nodeOff[p];
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                if (!((mask >> e) & 1u)) continue;
                const int d = e + 1;
                const double fb = phi[p + (d & 1) + (long)sx * ((d >> 1) & 1) + sxy * ((d >> 2) & 1)] - iso;
                const double t = fa / (fa - fb);
                t1 += t == 1.0 ? 1ull : 0ull;
                surfX[slot] = xs_coord(x0, i, d & 1, t, dx);
                surfX[slot + nn] = xs_coord(y0, j, d & 2, t, dx);
                surfX[slot + 2 * nn] = xs_coord(z0, k, d & 4, t, dx);
                ++slot;
            }
        }
        if (byte != 0u && byte != 255u) { // a crossed cell (wall points carry byte 0): all eight corners exist
            long ts = triOff[p];
            // the node on the edge between the corner offsets u < v of this cell, 1-based
            auto node = [&](unsigned u, unsigned v) -> int32_t {
                const long b = p + (long)(u & 1u) + (long)sx * ((u >> 1) & 1u) + sxy * ((u >> 2) & 1u);
                const unsigned e = (u ^ v) - 1u;
                return (int32_t)(nodeOff[b] + (uint32_t)__builtin_popcount((unsigned)maskIn[b] & ((1u << e) - 1u)) + 1u);
            };
            xs_cell_emit(byte, node, [&](int32_t a, int32_t b, int32_t c) {
                surfElem[ts] = a, surfElem[ts + nt] = b, surfElem[ts + 2 * nt] = c;
                ++ts;
            });
        }
    }
    t1 = wave_usum(t1);
    if ((threadIdx.x & 63u) == 0u && t1) atomicAdd(&ctl[XS_T1], t1);
}

} // namespace lsf
