// lsf_reseed_points.hpp -- the maintenance of the marker population of the particle level set on the device: keep, drop and re-radius
// the old markers, count them per cell, top every under-populated cell next to the surface up with new markers attracted to a random
// target level, and return one compacted set: lsf_reseed_points (include/lsf.h).
//
// Plain launches in stream order, no block waits for another:
//   k_rs_classify    one lane per old marker, in the caller's order: radius, pt_locate, the band rule on the 8 corners of its cell
//                    (pt_in_band), the LINEAR value (sp_stencil; all of lsf_point_stencil.hpp).  Writes status, the refreshed
//                    radius, the keep flag
//                    with the marker's exclusive rank inside its block (xs_block_scan of lsf_extract_surface.hpp, reused), the
//                    block's kept total, and adds 1 to the int32 count of the marker's cell: integer atomics, order-free.
//   k_rs_cells       one lane per cell in memory order -- the points of the grid or, under a mask, the entries of the BandList in
//                    memory order, each taken as the lower corner of its cell: eligibility by seedParticles' rule, need =
//                    max(per_cell - count, 0), its exclusive rank inside the tile of RS_BLOCK cells and the tile's total.
//   k_extract_scan   (lsf_extract_surface.hpp, as it is) one block: exclusive tile offsets and the total, for the kept flags, the
//                    needs and, later, the accept flags.
//   k_rs_candidates  one lane per candidate g = (cell, j) in ascending (p, j).  The cell is found by a two-level binary search of the
//                    exclusive offsets (tiles, then the RS_BLOCK ranks of the tile): at most 32 + 8 dependent 4- or 16-byte loads
//                    beside the 64 to 448 gathers of the samples that follow.  The alternative, one block per tile of cells, leaves
//                    most blocks of a maskless grid without a candidate and the others with anything from 1 to 256 * per_cell;
//                    the search keeps every wave full of candidates whatever the shape of the band.  Then the four draws
//                    (splitmix64, exact integer arithmetic), the first sample in the caller's order (sp_sample), the attraction --
//                    the foot iteration of lsf_sample_points (pt_foot) with the candidate's goal as iso, at most `iters` moves -- the
//                    LINEAR
//                    sample at the end and the acceptance.  Stores position, radius (0 for a rejected candidate) and the accept
//                    flag with its rank.
//   k_rs_emit_kept, k_rs_emit_new   the kept markers in the caller's order with src = 1-based input position, then the accepted
//                    candidates in ascending (p, j) with src = 0.
// Everything is evaluated as the header writes it, left to right, without contraction, so the result is the numpy statement's
// (tests/reseed_ref.py) bit for bit; the counts are integers and no order of execution reaches them.
//
// Bounds.  An old marker reaches loads only behind pt_locate ("Bounds" of lsf_point_stencil.hpp); behind it the 8 corners exist
// and the cell's lower corner p = i0 + ... is below the number of points, the size of count.  k_rs_cells forms a cell only where
// i < nx, j < ny, k < nz, so its 8 corners exist; a list entry is an interior point.
// A candidate exists only for g < ncand, the total of the needs, so both searches end on a cell with need > 0 (below); its position
// and every moved position pass sp_sample's locate before anything is loaded for them.  Slots: a kept marker writes slot
// offK + rank < nkept, a new one nkept + offA + rank < nout, each into arrays of nout and 3 nout entries.  Lanes beyond npts, the
// cells or ncand touch no memory.  Every loop is bounded: the searches by 32 and 8 trips, the attraction by iters <= 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsf.h"
#include "lsf_block_reduce.hpp"
#include "lsf_extract_surface.hpp"
#include "lsf_point_stencil.hpp"

namespace lsf {

constexpr int RS_BLOCK = 256;                  // markers, cells or candidates per block; a tile of the scans
constexpr int RS_NPART = 7;                    // the six status counts and the kept markers on the wrong side
constexpr uint32_t RS_FLAG = 0x80000000u;      // bit 31 of a rank word: kept (markers), accepted (candidates)
// ctl words (unsigned long long) of one call
enum { RS_NCAND = 0, RS_NKEPT = 2, RS_NACC = 4, RS_ELIG = 6, RS_OVER = 7, RS_MAXC = 8, RS_REJ_EARLY = 9, RS_REJ_LATE = 10, RS_CTL_LEN = 12 };

struct RsParams {
    int per_cell, iters;
    double rmin, band; // as given
    double rmin_dx, rmax_dx, band_dx, tol_dx; // rmin*dx, rmax*dx, band*dx, tol*dx: one product each, formed once on the host
    unsigned long long seed;
};

// u_d of candidate (p, j): the splitmix64 finaliser of the counter (p*4096 + j)*4 + d, all mod 2^64
__device__ __forceinline__ double rs_draw(unsigned long long seed, unsigned long long p, unsigned j, unsigned d)
{
    const unsigned long long ctr = (p * 4096ull + j) * 4ull + d;
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (ctr + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * 0x1.0p-53; // both factors exact: no rounding
}

// Old marker t of block blockIdx.x.  pts: (npts, 3) in Fortran order.  status may be NULL.  count: int32 per grid point (the cell's
// lower corner), zero before the launch.  rank[t]: RS_FLAG if kept | exclusive rank among the block's kept; sums[block].x their
// number (.y = 0).  part: RS_NPART counts per block.
template <bool HAS_MASK>
__global__ __launch_bounds__(RS_BLOCK) void k_rs_classify(SpGrid G, RsParams P, const double* __restrict__ pts, const double* __restrict__ rad,
                                                          int npts, int32_t* __restrict__ status, double* __restrict__ radn,
                                                          uint32_t* __restrict__ rank, uint2* __restrict__ sums, int* count,
                                                          unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ unsigned red[RS_BLOCK / 64][2];
    const size_t t = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, N = (size_t)npts;
    int st = -1; // no marker
    bool wrong = false;
    double rn = 0.0;
    if (t < N) {
        const double ra = rad[t];
        int i0[3];
        double tt[3];
        if (!__builtin_isfinite(ra) || ra == 0.0)
            st = LSF_RESEED_BADRADIUS;
        // The INSIDE test comes first: nothing below may run for a marker that fails it (see "Bounds" above).
        else if (!pt_locate<false>(pts[t], G.x0, G.dx, G.nx, i0[0], tt[0]) || !pt_locate<false>(pts[t + N], G.y0, G.dx, G.ny, i0[1], tt[1]) ||
                 !pt_locate<false>(pts[t + 2 * N], G.z0, G.dx, G.nz, i0[2], tt[2]))
            st = LSF_RESEED_OUTSIDE;
        else if (HAS_MASK && !pt_in_band<2>(G, i0))
            st = LSF_RESEED_OFFBAND;
        else {
            SpSample o;
            sp_stencil<false, false>(G, nullptr, i0, tt, o);
            if (!__builtin_isfinite(o.v))
                st = LSF_RESEED_NONFINITE;
            else if (__builtin_fabs(o.v) > P.band_dx)
                st = LSF_RESEED_FAR;
            else {
                st = LSF_RESEED_KEPT;
                const double s = ra < 0.0 ? -1. : 1.;
                const double sv = s * o.v;
                wrong = sv < 0.0;
                rn = s * __builtin_fmin(__builtin_fmax(sv, P.rmin_dx), P.rmax_dx);
                const size_t rs = (size_t)G.nx + 1, ps = rs * ((size_t)G.ny + 1);
                atomicAdd(count + ((size_t)i0[0] + rs * (size_t)i0[1] + ps * (size_t)i0[2]), 1);
            }
        }
        if (status) status[t] = st;
        radn[t] = rn;
    }
    unsigned a = st == LSF_RESEED_KEPT ? 1u : 0u, b = 0u, ta, tb;
    const unsigned keep = a;
    xs_block_scan<RS_BLOCK>(a, b, ta, tb, red);
    if (t < N) rank[t] = a | (keep ? RS_FLAG : 0u);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(ta, 0u);
    unsigned long long cnt[RS_NPART];
#pragma unroll
    for (int m = 0; m < 6; ++m) cnt[m] = st == m;
    cnt[6] = wrong;
    block_usum_out<RS_BLOCK / 64>(cnt, (int)threadIdx.x, part + (size_t)blockIdx.x * RS_NPART);
}

// Entry e of the list L (LIST) or point e of the grid, taken as the lower corner of its cell; n: entries or points.  rank[e]: the
// exclusive rank of the cell's first candidate inside its tile; sums[tile].x the tile's candidates.  ctl: RS_ELIG, RS_OVER, RS_MAXC.
template <bool LIST>
__global__ __launch_bounds__(RS_BLOCK) void k_rs_cells(SpGrid G, RsParams P, const int* __restrict__ L, size_t n, const int* __restrict__ count,
                                                       uint32_t* __restrict__ rank, uint2* __restrict__ sums, unsigned long long* __restrict__ ctl)
{
    __shared__ unsigned red[RS_BLOCK / 64][2];
    const size_t e = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    unsigned need = 0u, elig = 0u, over = 0u, cmax = 0u;
    if (e < n) {
        const size_t p = LIST ? (size_t)(unsigned)L[e] : e;
        const size_t rs = (size_t)G.nx + 1, ps = rs * ((size_t)G.ny + 1);
        const int i = (int)(p % rs), j = (int)((p / rs) % ((size_t)G.ny + 1)), k = (int)(p / ps);
        const int cnt = count[p];
        cmax = (unsigned)cnt;
        over = cnt > P.per_cell ? 1u : 0u;
        if (i < G.nx && j < G.ny && k < G.nz) { // the point owns a cell: its 8 corners exist
            bool ok = true;
            if constexpr (LIST) {
                const int lo[3] = {i, j, k};
                ok = pt_in_band<2>(G, lo);
            }
            if (ok) {
                const double* __restrict__ f = G.phi + p;
#pragma unroll
                for (int c = 0; c < 8; ++c) ok = ok && __builtin_fabs(f[(size_t)(c & 1) + rs * (size_t)((c >> 1) & 1) + ps * (size_t)(c >> 2)]) < P.band_dx;
            }
            if (ok) {
                elig = 1u;
                need = cnt < P.per_cell ? (unsigned)(P.per_cell - cnt) : 0u;
            }
        }
    }
    unsigned a = need, b = elig, ta, tb;
    xs_block_scan<RS_BLOCK>(a, b, ta, tb, red);
    if (e < n) rank[e] = a;
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = make_uint2(ta, 0u);
        if (tb) atomicAdd(&ctl[RS_ELIG], (unsigned long long)tb);
    }
    over = wave_usum(over);
    const unsigned long long mx = wave_umax_x((unsigned long long)cmax);
    if ((threadIdx.x & 63u) == 0u) {
        if (over) atomicAdd(&ctl[RS_OVER], (unsigned long long)over);
        if (mx) atomicMax(&ctl[RS_MAXC], mx);
    }
}

// Candidate g of block blockIdx.x; ncand > 0 candidates over the n cells whose ranks and tile offsets k_rs_cells and k_extract_scan
// left.  cpts: (ncand, 3) in Fortran order; crad[g] == 0 for a rejected candidate; arank[g]: RS_FLAG if accepted | its exclusive
// rank among the block's accepted; asums[block].x their number.  ctl: RS_REJ_EARLY, RS_REJ_LATE.
template <bool CUBIC, bool HAS_MASK>
__global__ __launch_bounds__(RS_BLOCK) void k_rs_candidates(SpGrid G, RsParams P, const int* __restrict__ L, size_t n,
                                                            const uint32_t* __restrict__ rank, const ulonglong2* __restrict__ tileOff,
                                                            unsigned long long ncand, double* __restrict__ cpts, double* __restrict__ crad,
                                                            uint32_t* __restrict__ arank, uint2* __restrict__ asums,
                                                            unsigned long long* __restrict__ ctl)
{
#pragma clang fp contract(off)
    __shared__ unsigned red[RS_BLOCK / 64][2];
    const unsigned long long g = (unsigned long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    unsigned acc = 0u, early = 0u, late = 0u;
    if (g < ncand) {
        // the last tile whose offset is <= g, then the last cell of it whose rank is <= g - offset: g lies below that cell's offset
        // plus its need, so the need is positive (cells without candidates share their offset with the next one and are passed over)
        const size_t nTiles = (n + RS_BLOCK - 1) / RS_BLOCK;
        size_t lo = 0, hi = nTiles; // tileOff[lo].x <= g; tileOff[hi].x > g or hi == nTiles
        while (hi - lo > 1) {
            const size_t mid = lo + (hi - lo) / 2;
            if (tileOff[mid].x <= g) lo = mid;
            else hi = mid;
        }
        const unsigned r = (unsigned)(g - tileOff[lo].x);
        const size_t e0 = lo * RS_BLOCK;
        size_t a = 0, b = n - e0 < (size_t)RS_BLOCK ? n - e0 : (size_t)RS_BLOCK;
        while (b - a > 1) {
            const size_t mid = a + (b - a) / 2;
            if (rank[e0 + mid] <= r) a = mid;
            else b = mid;
        }
        const size_t e = e0 + a;
        const unsigned j = r - rank[e];
        const unsigned long long p = HAS_MASK ? (unsigned long long)(unsigned)L[e] : (unsigned long long)e;
        const unsigned long long rs = (unsigned long long)G.nx + 1, ny1 = (unsigned long long)G.ny + 1;
        const int ci = (int)(p % rs), cj = (int)((p / rs) % ny1), ck = (int)(p / (rs * ny1));
        const double u0 = rs_draw(P.seed, p, j, 0u), u1 = rs_draw(P.seed, p, j, 1u), u2 = rs_draw(P.seed, p, j, 2u), u3 = rs_draw(P.seed, p, j, 3u);
        const double x0 = G.x0 + ((double)ci + u0) * G.dx, x1 = G.y0 + ((double)cj + u1) * G.dx, x2 = G.z0 + ((double)ck + u2) * G.dx;
        double y0 = x0, y1 = x1, y2 = x2, rd = 0.0;
        SpSample s;
        int st = sp_sample<CUBIC, false, HAS_MASK>(G, nullptr, x0, x1, x2, s);
        if (st == LSF_SAMPLE_OK && !__builtin_isfinite(s.v)) st = -1;
        if (st == LSF_SAMPLE_OK) {
            const double sg = s.v < 0.0 ? -1. : 1.;
            const double goal = sg * ((P.rmin + (P.band - P.rmin) * u3) * G.dx);
            st = pt_foot<CUBIC, HAS_MASK>(G, goal, P.iters, P.tol_dx, s, y0, y1, y2);
            if (st == LSF_SAMPLE_OK) {
                SpSample l;
                const int s3 = sp_sample<false, false, HAS_MASK>(G, nullptr, y0, y1, y2, l);
                if (s3 == LSF_SAMPLE_OK) {
                    const double av = __builtin_fabs(l.v);
                    if (av >= P.rmin_dx && av <= P.band_dx && (l.v < 0.0 ? -1. : 1.) == sg) {
                        acc = 1u;
                        rd = sg * __builtin_fmin(__builtin_fmax(av, P.rmin_dx), P.rmax_dx);
                    }
                }
                late = acc ? 0u : 1u;
            } else
                early = 1u;
        } else
            early = 1u;
        cpts[g] = y0, cpts[g + ncand] = y1, cpts[g + 2 * ncand] = y2;
        crad[g] = rd;
    }
    unsigned a = acc, b = 0u, ta, tb;
    xs_block_scan<RS_BLOCK>(a, b, ta, tb, red);
    if (g < ncand) arank[g] = a | (acc ? RS_FLAG : 0u);
    if (threadIdx.x == 0) asums[blockIdx.x] = make_uint2(ta, 0u);
    wave_usum_each(early, late);
    if ((threadIdx.x & 63u) == 0u) {
        if (early) atomicAdd(&ctl[RS_REJ_EARLY], (unsigned long long)early);
        if (late) atomicAdd(&ctl[RS_REJ_LATE], (unsigned long long)late);
    }
}

// the kept old markers, in the caller's order: slot = tileOff[block].x + rank.  src may be NULL.
static __global__ __launch_bounds__(RS_BLOCK) void k_rs_emit_kept(const double* __restrict__ pts, const double* __restrict__ radn, int npts,
                                                                   const uint32_t* __restrict__ rank, const ulonglong2* __restrict__ tileOff,
                                                                   double* __restrict__ pout, double* __restrict__ rout, int32_t* __restrict__ src,
                                                                   size_t nout)
{
    const size_t t = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, N = (size_t)npts;
    if (t >= N) return;
    const uint32_t w = rank[t];
    if (!(w & RS_FLAG)) return;
    const size_t slot = (size_t)tileOff[blockIdx.x].x + (w & ~RS_FLAG);
    pout[slot] = pts[t], pout[slot + nout] = pts[t + N], pout[slot + 2 * nout] = pts[t + 2 * N];
    rout[slot] = radn[t];
    if (src) src[slot] = (int32_t)(t + 1);
}

// the accepted candidates behind the nkept kept markers, in ascending (p, j)
static __global__ __launch_bounds__(RS_BLOCK) void k_rs_emit_new(const double* __restrict__ cpts, const double* __restrict__ crad,
                                                                  unsigned long long ncand, const uint32_t* __restrict__ arank,
                                                                  const ulonglong2* __restrict__ tileOff, size_t nkept, double* __restrict__ pout,
                                                                  double* __restrict__ rout, int32_t* __restrict__ src, size_t nout)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (g >= ncand) return;
    const uint32_t w = arank[g];
    if (!(w & RS_FLAG)) return;
    const size_t slot = nkept + (size_t)tileOff[blockIdx.x].x + (w & ~RS_FLAG);
    pout[slot] = cpts[g], pout[slot + nout] = cpts[g + ncand], pout[slot + 2 * nout] = cpts[g + 2 * ncand];
    rout[slot] = crad[g];
    if (src) src[slot] = 0;
}

} // namespace lsf
