// lsf_evolve_band.hpp -- the band time loop: lsf_evolve_band (include/lsf.h) moves the surface and its cell list together.
//
// A step is the stages of lsf_advect_field_band (k_advect_band_stage, k_advect_finish) followed by sweeps of lsf_reinit_band
// (k_rb_gather for phiS, k_reinit_band), all on ONE list that stays on the device from step to step: nothing of a step is
// proportional to the grid.  What is new here are the four passes that let the list follow the surface (Peng et al.'s local level
// set method: dilate the trusted core, give entering cells a placeholder the sweeps then correct):
//
//   k_evb_check      over the list: open-edge cells, sign flips among them against the last build, the smallest |phi| there, and
//                    the wall-adjacent cells with |phi| < core dx.  One quadruple of partials per block, finished IN BLOCK ORDER by
//                    k_evb_check_finish into one 64-byte record: all the host reads per check.
//   k_evb_dilate     core mark and dilation: a list cell with |phi| < core dx stores 1 at every interior point within Chebyshev
//                    distance `ring` into the (zeroed) scratch mask.  Lanes that cover the same point store the same value.
//   k_evb_leave      over the OLD list: its cells are copied from phi into every stage buffer (a stage buffer must equal phi
//                    off-list at all times, and a leaving cell is about to be off-list), and a cell the scratch mask does not hold
//                    leaves the caller's mask.
//   k_evb_enter      over the NEW list: a cell the caller's mask does not hold yet enters with phi < 0 ? -far : +far, written into phi
//                    AND every stage buffer, and into the caller's mask; one count per block, added up by k_evb_enter_finish.
//   k_evb_edge       over the new list, after k_evb_enter has completed the mask: the open-edge flag, the sign of phi (the reference
//                    of the flips until the next build) and the wall-adjacent flag, one byte per list entry.
//
// Bounds: lsf_band_cell.hpp.  What is this file's own: every list after the first comes from k_mb_collect<true> run on the scratch
// mask, which k_evb_dilate writes at interior points only, so its entries are interior points too.  k_evb_dilate clips its cube to
// 1..n-1 on each axis BEFORE it forms an address: i0 = max(i - ring, 1), i1 = min(i + ring, nx - 1), likewise j and k, and
// 1 <= i0 <= i <= i1 <= nx - 1 because the cell itself is interior.  k_evb_edge reads the mask at the six neighbours of an interior
// point: distance 1, inside the field.  Every other access is at the lane's own point or its own list entry.
//
// Plain launches only: no atomics, no block waits for another; every reduction is a bit-pattern minimum or an integer count, so the
// order of the list reaches no result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_advect_band.hpp"

namespace lsf {

constexpr int EVB_OPEN = 1, EVB_NEG = 2, EVB_WALL = 4; // the byte of k_evb_edge
constexpr int EVB_CHECK_BLOCKS = 1024;                  // most blocks of k_evb_check
// the record of a check (unsigned 64-bit words): what the host reads
enum EvbRec { EVB_R_MARGIN = 0, EVB_R_OPEN = 1, EVB_R_FLIPS = 2, EVB_R_WALL = 3, EVB_R_ENTERED = 4, EVB_R_STOP = 5, EVB_R_COUNT = 6, EVB_R_NAN = 7, EVB_R_WORDS = 8 };

// the caller's mask after the first list build: 1 on the list cells (the mask has been zeroed)
static __global__ __launch_bounds__(256) void k_evb_set(const int* __restrict__ L, int nL, int32_t* __restrict__ mask)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nL) mask[L[e]] = 1;
}

// end of a step whose last pass wrote the second buffer: its list cells into phi -- unless the call has stopped (a NaN step: the
// sweeps behind it left at once and the buffer does not hold what the host's bookkeeping says)
static __global__ __launch_bounds__(256) void k_evb_scatter(const int* __restrict__ L, const double* __restrict__ G, int nL, double* __restrict__ F,
                                                            const int* __restrict__ done)
{
    if (done[CTL_STOP]) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nL) {
        const int p = L[e];
        F[p] = G[p];
    }
}

static __global__ __launch_bounds__(256) void k_evb_check(const double* __restrict__ phi, const int* __restrict__ L,
                                                          const unsigned char* __restrict__ flag, int nL, double core_dx,
                                                          unsigned long long* __restrict__ part, int nb)
{
    __shared__ unsigned long long rmn[4], re[4], rf[4], rw[4];
    unsigned long long mn = ADV_INF_BITS, ne = 0ull, nf = 0ull, nw = 0ull;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < nL; e += 256L * gridDim.x) {
        const int fl = flag[e];
        if (fl & (EVB_OPEN | EVB_WALL)) {
            const double x = phi[L[e]];
            if (fl & EVB_OPEN) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(__builtin_fabs(x));
                mn = b < mn ? b : mn;
                ne += 1ull;
                nf += (unsigned long long)((x < 0.0) != ((fl & EVB_NEG) != 0));
            }
            if (fl & EVB_WALL) nw += (unsigned long long)(__builtin_fabs(x) < core_dx);
        }
    }
    // counts and a minimum: the wave-level pieces of lsf_block_reduce.hpp, one barrier
    mn = wave_umin(mn);
    wave_usum_each(ne, nf, nw);
    if ((threadIdx.x & 63) == 0) rmn[threadIdx.x >> 6] = mn, re[threadIdx.x >> 6] = ne, rf[threadIdx.x >> 6] = nf, rw[threadIdx.x >> 6] = nw;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = rmn[0];
        for (int q = 1; q < 4; ++q) t = rmn[q] < t ? rmn[q] : t;
        part[blockIdx.x] = t;
        part[nb + blockIdx.x] = (re[0] + re[1]) + (re[2] + re[3]);
        part[2 * nb + blockIdx.x] = (rf[0] + rf[1]) + (rf[2] + rf[3]);
        part[3 * nb + blockIdx.x] = (rw[0] + rw[1]) + (rw[2] + rw[3]);
    }
}

// the partials of k_evb_check in block order (thread t takes blocks t, t + 256, ...: at most four quadruples; a minimum and three
// integer sums, the same in any order), and the control words beside them: the record of the check.  One block.
static __global__ __launch_bounds__(256) void k_evb_check_finish(const unsigned long long* __restrict__ part, int nb, const int* __restrict__ ctl,
                                                                 unsigned long long* __restrict__ rec)
{
    __shared__ unsigned long long rmn[4], re[4], rf[4], rw[4];
    unsigned long long mn = ADV_INF_BITS, ne = 0ull, nf = 0ull, nw = 0ull;
    for (int b = threadIdx.x; b < nb; b += 256) {
        const unsigned long long x = part[b];
        mn = x < mn ? x : mn;
        ne += part[nb + b], nf += part[2 * nb + b], nw += part[3 * nb + b];
    }
    mn = wave_umin(mn);
    wave_usum_each(ne, nf, nw);
    if ((threadIdx.x & 63) == 0) rmn[threadIdx.x >> 6] = mn, re[threadIdx.x >> 6] = ne, rf[threadIdx.x >> 6] = nf, rw[threadIdx.x >> 6] = nw;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = rmn[0];
        for (int q = 1; q < 4; ++q) t = rmn[q] < t ? rmn[q] : t;
        rec[EVB_R_MARGIN] = t;
        rec[EVB_R_OPEN] = (re[0] + re[1]) + (re[2] + re[3]);
        rec[EVB_R_FLIPS] = (rf[0] + rf[1]) + (rf[2] + rf[3]);
        rec[EVB_R_WALL] = (rw[0] + rw[1]) + (rw[2] + rw[3]);
        rec[EVB_R_STOP] = (unsigned long long)ctl[CTL_STOP];
        rec[EVB_R_COUNT] = (unsigned long long)ctl[CTL_COUNT];
        rec[EVB_R_NAN] = (unsigned long long)ctl[CTL_NAN];
    }
}

// core mark and dilation (see the head of the file for the bounds)
static __global__ __launch_bounds__(256) void k_evb_dilate(const double* __restrict__ phi, const int* __restrict__ L, int nL, int nx, int ny, int nz,
                                                           double core_dx, int ring, int32_t* __restrict__ scratch)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nL) return;
    const unsigned p = (unsigned)L[e];
    if (!(__builtin_fabs(phi[p]) < core_dx)) return;
    int i, j, k;
    band_decode(p, nx, ny, i, j, k);
    const int i0 = max(i - ring, 1), i1 = min(i + ring, nx - 1);
    const int j0 = max(j - ring, 1), j1 = min(j + ring, ny - 1);
    const int k0 = max(k - ring, 1), k1 = min(k + ring, nz - 1);
    const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
    for (int kk = k0; kk <= k1; ++kk)
        for (int jj = j0; jj <= j1; ++jj) {
            int32_t* row = scratch + kk * ps + jj * rs;
            for (int ii = i0; ii <= i1; ++ii) row[ii] = 1;
        }
}

// over the OLD list, before the new one is built.  W2 may be nullptr (Euler has one stage buffer).
static __global__ __launch_bounds__(256) void k_evb_leave(const int* __restrict__ L, int nL, const double* __restrict__ phi, double* __restrict__ W1,
                                                          double* __restrict__ W2, const int32_t* __restrict__ scratch, int32_t* __restrict__ mask)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nL) return;
    const int p = L[e];
    const double x = phi[p];
    W1[p] = x;
    if (W2) W2[p] = x;
    if (scratch[p] != 1) mask[p] = 0;
}

// over the NEW list.  A lane reads and writes its own point only.
static __global__ __launch_bounds__(256) void k_evb_enter(const int* __restrict__ L, int nL, double far, double* __restrict__ phi,
                                                          double* __restrict__ W1, double* __restrict__ W2, int32_t* __restrict__ mask,
                                                          unsigned long long* __restrict__ counts)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    unsigned long long c = 0ull;
    if (e < nL) {
        const int p = L[e];
        if (mask[p] != 1) {
            const double x = phi[p] < 0.0 ? -far : far;
            phi[p] = x;
            W1[p] = x;
            if (W2) W2[p] = x;
            mask[p] = 1;
            c = 1ull;
        }
    }
    c = block_usum<4>(c, threadIdx.x);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// the entering cells of a rebuild, added to the record's running sum (one block)
static __global__ __launch_bounds__(256) void k_evb_enter_finish(const unsigned long long* __restrict__ counts, int n, unsigned long long* __restrict__ rec)
{
    unsigned long long c = 0ull;
    for (int b = threadIdx.x; b < n; b += 256) c += counts[b];
    c = block_usum<4>(c, threadIdx.x);
    if (threadIdx.x == 0) rec[EVB_R_ENTERED] += c;
}

// the open-edge/sign pass: one byte per list entry, from the caller's mask (1 on the list, 0 elsewhere) and the field as they are.
// EVB_OPEN: an axis neighbour is an interior point outside the list (a wall neighbour opens nothing: the list cannot grow there);
// EVB_NEG: phi < 0 now; EVB_WALL: an axis neighbour is a wall point.
static __global__ __launch_bounds__(256) void k_evb_edge(const int32_t* __restrict__ mask, const double* __restrict__ phi, const int* __restrict__ L,
                                                         int nL, int nx, int ny, int nz, unsigned char* __restrict__ flag)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nL) return;
    const unsigned p = (unsigned)L[e];
    int i, j, k;
    band_decode(p, nx, ny, i, j, k);
    const long rs = nx + 1, ps = (long)(nx + 1) * (ny + 1);
    const int32_t* m = mask + p;
    const bool open = (i > 1 && m[-1] != 1) || (i < nx - 1 && m[1] != 1) || (j > 1 && m[-rs] != 1) || (j < ny - 1 && m[rs] != 1) ||
                      (k > 1 && m[-ps] != 1) || (k < nz - 1 && m[ps] != 1);
    const bool wall = i == 1 || i == nx - 1 || j == 1 || j == ny - 1 || k == 1 || k == nz - 1;
    flag[e] = (unsigned char)((open ? EVB_OPEN : 0) | (phi[p] < 0.0 ? EVB_NEG : 0) | (wall ? EVB_WALL : 0));
}

} // namespace lsf
