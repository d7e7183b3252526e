// lsf_distance_fill.hpp -- first-order Godunov fast sweeping of |grad phi| = 1 outwards from a frozen set: lsf_distance_fill.  No
// reference counterpart.  Contract: include/lsf.h; account: DESIGN.md section 4.11; driver: lsf_host_distance_fill.hpp.
//
// The only grid-sized storage besides the caller's field is one bit per point: a 32-bit word per run of DF_TX points of a row
// (rows start a new word, so a word is exactly one row of a tile).  Bit set = the point is FROZEN or lies outside the grid.
//   k_df_check       read-only on the field: builds the words, counts frozen points, non-finite frozen values and pairs of axis
//                    neighbours of opposite sign that are not both frozen.  The host decides the errors before anything is written.
//   k_df_init        every other point becomes +-inf with the sign it has (phi < 0 is negative).
//   k_df_tile_plane  one raster sweep, tile plane by tile plane.  Tiles of DF_TX x DF_TY x DF_TZ points; the tiles with A + B + C = P
//                    in the sweep's reflected frame form one plain launch, planes in stream order.  A radius-1 star stencil reads
//                    from a face neighbour only: the upstream ones ran in the launch before (this sweep's values), the downstream
//                    ones run in the launch after (old values), and two tiles of one plane share no face -- the Gauss-Seidel
//                    condition of SURVEY.md appendix B with radius 1, so the result is the serial raster sweep bit for bit.
//                    One wave per tile: the magnitudes of the tile and its six face halos sit in LDS; lane (b, c) of the 8 x 8 rows
//                    marches along its row one step behind its two upstream rows (cell a at step a + b + c: the in-tile hyperplane),
//                    reads the six neighbours, solves, and lowers its cell.  The direction of the sweep only reflects which row and
//                    which end a lane starts from.  Signs and frozen bits are one word per row.  A tile without a live cell returns
//                    before it loads; a tile that lowered nothing stores nothing.
// LDS layout: row pitch 34 doubles (32 + 2 halo), plane pitch 361 (>= 340, = 9 mod 32).  At one step the lanes of a 32-lane half
// (b = 0..7, c = 0..3) address p + 33 b + 360 c = p + b + 8 c (mod 32) doubles: 32 distinct 8-byte slots of the 64-bank row, so
// the six ds_read_b64 of a step are conflict-free in every direction (a reflection negates b or c).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsf {

constexpr int DF_TX = 32, DF_TY = 8, DF_TZ = 8;
constexpr int DF_PX = DF_TX + 2;
constexpr int DF_PXY = 361;
constexpr int DF_STEPS = DF_TX + DF_TY + DF_TZ - 2;
constexpr int DF_ROWS = DF_TY * DF_TZ; // = lanes of the wave
static_assert(DF_TX == 32 && DF_ROWS == 64, "a frozen word is one tile row, a wave holds one lane per row");
static_assert(DF_PXY >= DF_PX * (DF_TY + 2), "plane pitch");

// counters of one call (64-bit words): frozen points, non-finite frozen values, sign jumps, visits that lowered a value
enum { DF_N_FROZEN, DF_N_NONFINITE, DF_N_JUMP, DF_N_CHANGED, DF_N_COUNTERS };

struct DfGrid {
    int NX, NY, NZ;    // points per axis
    int nTA, nTB, nTC; // tiles per axis
};

// The update of one point from the smaller neighbour magnitude of each axis; every operation as the contract writes it.
__device__ __forceinline__ double df_solve(double x, double y, double z, double dx)
{
#pragma clang fp contract(off)
    const double a = fmin(fmin(x, y), z);
    const double c = fmax(fmax(x, y), z);
    const double b = fmax(fmin(x, y), fmin(fmax(x, y), z));
    double t = a + dx;
    if (t > b) {
        const double d = a - b;
        t = ((a + b) + __builtin_sqrt(2.0 * (dx * dx) - d * d)) * 0.5;
        if (t > c) {
            const double s = ((a - b) * (a - b) + (a - c) * (a - c)) + (b - c) * (b - c);
            t = (((a + b) + c) + __builtin_sqrt(fmax(3.0 * (dx * dx) - s, 0.0))) / 3.0;
        }
    }
    return t;
}

// A 32-lane half of a wave per word.  mask == nullptr: frozen = |phi| < far.
__global__ __launch_bounds__(256) void k_df_check(const double* __restrict__ phi, const int32_t* __restrict__ mask, DfGrid g, double far,
                                                  long long nwords, uint32_t* __restrict__ words, unsigned long long* __restrict__ counters)
{
    const long long w = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    unsigned nfz = 0, nnf = 0, njump = 0;
    bool bit = true;
    if (w < nwords) {
        const int tA = (int)(w % g.nTA);
        const long long row = w / g.nTA;
        const int j = (int)(row % g.NY), k = (int)(row / g.NY);
        const int i = tA * DF_TX + (threadIdx.x & 31);
        if (i < g.NX) {
            const size_t sy = (size_t)g.NX, sz = sy * (size_t)g.NY;
            const size_t p = (size_t)i + sy * (size_t)j + sz * (size_t)k;
            const double v = phi[p];
            const bool fz = mask ? mask[p] == 1 : fabs(v) < far;
            const bool neg = v < 0.0;
            bit = fz;
            nfz = fz;
            nnf = fz && !isfinite(v);
            const size_t step[3] = {1, sy, sz};
            const bool has[3] = {i + 1 < g.NX, j + 1 < g.NY, k + 1 < g.NZ};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
                if (has[ax]) {
                    const size_t q = p + step[ax];
                    const double v2 = phi[q];
                    const bool fz2 = mask ? mask[q] == 1 : fabs(v2) < far;
                    njump += ((v2 < 0.0) != neg) && !(fz && fz2);
                }
        }
    }
    const unsigned long long bal = __ballot(bit);
    if (w < nwords && (threadIdx.x & 31) == 0) words[w] = (uint32_t)(bal >> (threadIdx.x & 32));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nfz += __shfl_down(nfz, off);
        nnf += __shfl_down(nnf, off);
        njump += __shfl_down(njump, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nfz) atomicAdd(counters + DF_N_FROZEN, (unsigned long long)nfz);
        if (nnf) atomicAdd(counters + DF_N_NONFINITE, (unsigned long long)nnf);
        if (njump) atomicAdd(counters + DF_N_JUMP, (unsigned long long)njump);
    }
}

__global__ __launch_bounds__(256) void k_df_init(double* __restrict__ phi, DfGrid g, long long nwords, const uint32_t* __restrict__ words)
{
    const long long w = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (w >= nwords) return;
    const int l = threadIdx.x & 31;
    if ((words[w] >> l) & 1u) return; // frozen, or past the end of the row
    const int tA = (int)(w % g.nTA);
    const long long row = w / g.nTA;
    const size_t p = (size_t)(tA * DF_TX + l) + (size_t)g.NX * (size_t)row;
    phi[p] = phi[p] < 0.0 ? -HUGE_VAL : HUGE_VAL;
}

// One wave per tile of the plane A + B + C = P of the frame reflected by (sx, sy, sz); block x = B + nTB * C.
__global__ __launch_bounds__(DF_ROWS) void k_df_tile_plane(double* phi, const uint32_t* __restrict__ words, DfGrid g, int P, int sx, int sy, int sz,
                                                           double dx, unsigned long long* __restrict__ counters)
{
    __shared__ double u[DF_PXY * (DF_TZ + 2)];
    __shared__ uint32_t s_neg[DF_ROWS], s_fz[DF_ROWS];
    const int B = (int)(blockIdx.x % (unsigned)g.nTB), C = (int)(blockIdx.x / (unsigned)g.nTB);
    const int A = P - B - C;
    if (A < 0 || A >= g.nTA) return;
    const int tA = sx > 0 ? A : g.nTA - 1 - A, tB = sy > 0 ? B : g.nTB - 1 - B, tC = sz > 0 ? C : g.nTC - 1 - C;
    const int x0 = tA * DF_TX, y0 = tB * DF_TY, z0 = tC * DF_TZ;
    const int lane = threadIdx.x;
    const size_t py = (size_t)g.NX, pz = py * (size_t)g.NY;

    // the row this lane marches: (b, c) in the frame, (jj, kk) in the tile
    const int b = lane & 7, c = lane >> 3;
    const int jj = sy > 0 ? b : DF_TY - 1 - b, kk = sz > 0 ? c : DF_TZ - 1 - c;
    uint32_t fw = ~0u;
    if (y0 + jj < g.NY && z0 + kk < g.NZ) fw = words[(size_t)tA + (size_t)g.nTA * ((size_t)(y0 + jj) + (size_t)g.NY * (size_t)(z0 + kk))];
    if (__ballot(fw != ~0u) == 0ull) return; // no live cell in this tile
    s_fz[jj + DF_TY * kk] = fw;

    // magnitude of a point, +inf outside the grid.  The load itself is unconditional (an outside point loads the tile's own first
    // point, which no other tile writes), so the loads of an unrolled loop go out together instead of one per branch
    const size_t p0 = (size_t)x0 + py * (size_t)y0 + pz * (size_t)z0;
    auto mag = [&](int i, int j, int k, bool* neg) -> double {
        const bool in = i >= 0 && i < g.NX && j >= 0 && j < g.NY && k >= 0 && k < g.NZ;
        const double v = phi[in ? (size_t)i + py * (size_t)j + pz * (size_t)k : p0];
        *neg = in && v < 0.0;
        return in ? fabs(v) : HUGE_VAL;
    };
    {
        const int half = lane >> 5, i = lane & 31;
        constexpr int G = 8; // loads in flight per lane: a group is loaded into registers first, then stored to LDS
        double v[G];
        bool ng[G];
        // the tile, two rows per step; a row's signs are one word
#pragma unroll 1
        for (int it0 = 0; it0 < DF_ROWS / 2; it0 += G) {
#pragma unroll
            for (int m = 0; m < G; ++m) {
                const int r = 2 * (it0 + m) + half;
                v[m] = mag(x0 + i, y0 + (r & 7), z0 + (r >> 3), &ng[m]);
            }
#pragma unroll
            for (int m = 0; m < G; ++m) {
                const int r = 2 * (it0 + m) + half;
                u[((r >> 3) + 1) * DF_PXY + ((r & 7) + 1) * DF_PX + i + 1] = v[m];
                const unsigned long long bal = __ballot(ng[m]);
                if (i == 0) s_neg[r] = (uint32_t)(bal >> (lane & 32));
            }
        }
        // the y and z face halos, 2 x 8 rows each (side 0: below, 1: above), and the x face halos, one point per row and side
        double w[2 * G + 2];
        const int rj = lane & 7, rk = lane >> 3;
#pragma unroll
        for (int it = 0; it < G; ++it) {
            const int r = 2 * it + half, m = r & 7, side = r >> 3;
            w[2 * it] = mag(x0 + i, side ? y0 + DF_TY : y0 - 1, z0 + m, &ng[0]);
            w[2 * it + 1] = mag(x0 + i, y0 + m, side ? z0 + DF_TZ : z0 - 1, &ng[0]);
        }
        w[2 * G] = mag(x0 - 1, y0 + rj, z0 + rk, &ng[0]);
        w[2 * G + 1] = mag(x0 + DF_TX, y0 + rj, z0 + rk, &ng[0]);
#pragma unroll
        for (int it = 0; it < G; ++it) {
            const int r = 2 * it + half, m = r & 7, side = r >> 3;
            u[(m + 1) * DF_PXY + (side ? DF_TY + 1 : 0) * DF_PX + i + 1] = w[2 * it];
            u[(side ? DF_TZ + 1 : 0) * DF_PXY + (m + 1) * DF_PX + i + 1] = w[2 * it + 1];
        }
        u[(rk + 1) * DF_PXY + (rj + 1) * DF_PX] = w[2 * G];
        u[(rk + 1) * DF_PXY + (rj + 1) * DF_PX + DF_TX + 1] = w[2 * G + 1];
    }
    __syncthreads();

    unsigned cnt = 0;
    double* row = u + (kk + 1) * DF_PXY + (jj + 1) * DF_PX + 1;
#pragma unroll 1
    for (int p = 0; p < DF_STEPS; ++p) {
        const int a = p - b - c;
        if (a >= 0 && a < DF_TX) {
            const int ii = sx > 0 ? a : DF_TX - 1 - a;
            if (!((fw >> ii) & 1u)) {
                double* q = row + ii;
                const double x = fmin(q[-1], q[1]), y = fmin(q[-DF_PX], q[DF_PX]), z = fmin(q[-DF_PXY], q[DF_PXY]);
                if (fmin(fmin(x, y), z) < HUGE_VAL) {
                    const double t = df_solve(x, y, z, dx);
                    if (t < q[0]) {
                        q[0] = t;
                        ++cnt;
                    }
                }
            }
        }
        __syncthreads(); // one wave: orders this step's LDS stores before the next step's loads
    }

    if (__ballot(cnt != 0) == 0ull) return; // nothing lowered: the tile in memory is already what LDS holds
    {
        const int half = lane >> 5, i = lane & 31;
#pragma unroll 8
        for (int it = 0; it < DF_ROWS / 2; ++it) {
            const int r = 2 * it + half, rj = r & 7, rk = r >> 3;
            if (!((s_fz[r] >> i) & 1u)) { // live: inside the grid and not frozen
                const double m = u[(rk + 1) * DF_PXY + (rj + 1) * DF_PX + i + 1];
                phi[(size_t)(x0 + i) + py * (size_t)(y0 + rj) + pz * (size_t)(z0 + rk)] = ((s_neg[r] >> i) & 1u) ? -m : m;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane == 0) atomicAdd(counters + DF_N_CHANGED, (unsigned long long)cnt);
}

} // namespace lsf
