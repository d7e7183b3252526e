// lsf_extend_band.hpp -- a quantity q carried off the frozen cells of a cell list constant along the normals of phi, by Jacobi passes
// of lsf_extend_field's visit over the list: lsf_extend_field_band (include/lsf.h; account: DESIGN.md section 4.18; driver:
// lsf_host_extend_band.hpp).
//
// The list is lsf_reinit_band's,
//     LIST = { interior points with mask == 1 on entry },
// built by the same machinery (band_list_count<true> / band_list_sort: brick-sorted 32-bit point indices).  Every kernel runs one
// lane per list entry, MB_CH consecutive entries -- a few neighbouring bricks -- per block.
//   k_extb_plan     once per call, read-only on the caller's arrays.  |phi| never changes during a call, so what an axis of a visit
//                   takes is fixed: per entry and axis the point index of the chosen neighbour and its weight w = f(p) - f(n), stored
//                   as 0.0 where the axis can never be used (w <= 0 -- which covers a NaN --, or the neighbour is not in the list:
//                   not interior, or its mask word is not 1).  An unused axis keeps the entry's OWN point as its index, so that no
//                   later gather of q leaves the list.  Also the frozen flag, and per block the counts the host decides the errors on.
//   k_extb_init     NaN into the non-frozen list cells, after the host has decided the errors.
//   k_extb_compute  one pass, first half: streams the plan, gathers q at the three neighbours and at the cell, evaluates the visit
//                   without contraction and writes the new value and a store flag to per-entry arrays.  q is only read.
//   k_extb_commit   second half: stores the flagged values at the lanes' own points and adds the block's count into cnt[p].  Two
//                   launches per pass: all reads of a pass come before its writes (Jacobi), with no block waiting for another.
//   k_extb_count    the non-frozen list cells that hold a value / are still NaN, per block.
// The stop test: cnt[] holds one 64-bit count per pass of a batch and is zeroed before the batch is enqueued.  The kernels of pass
// p > 0 of a batch return at once when cnt[p - 1] == 0: their own cnt[p] stays 0 and the rest of the batch drains empty.  The only
// atomic is that integer add, one per block and pass: no arrival order reaches a result.
//
// Bounds: lsf_band_cell.hpp (a list entry is an interior point, so p - 1, p + 1 and the points one row and one plane away exist).
// What is this file's own: the plan's indices are such neighbours or p itself, and per-entry arrays are indexed by e < nL only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_advect_band.hpp"

namespace lsf {

constexpr int EXTB_NPART = 3; // partials per block of k_extb_plan: frozen cells, frozen cells with a non-finite q, cells that see a non-finite phi

// nb: 3 x nL point indices, wt: 3 x nL weights (axis-major), fz: nL flags, part: EXTB_NPART words per block.
// known == nullptr: frozen = |phi| < far.
__global__ __launch_bounds__(MB_CH) void k_extb_plan(const double* __restrict__ q, const double* __restrict__ phi, const int32_t* __restrict__ mask,
                                                     const int32_t* __restrict__ known, const int* __restrict__ L, int nL, int nx, int ny, int nz,
                                                     double far, int* __restrict__ nb, double* __restrict__ wt, unsigned char* __restrict__ fz,
                                                     unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long v[EXTB_NPART] = {0ull, 0ull, 0ull};
    if (e < nL) {
        const int p = L[e];
        const int rs = nx + 1, ps = (nx + 1) * (ny + 1);
        const int k = p / ps, r = p - k * ps, j = r / rs, i = r - j * rs;
        const int c[3] = {i, j, k}, n1[3] = {nx, ny, nz}, st[3] = {1, rs, ps};
        const double a = phi[p], f = __builtin_fabs(a);
        bool badphi = !__builtin_isfinite(a);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double a_lo = phi[p - st[x]], a_hi = phi[p + st[x]];
            badphi = badphi || !__builtin_isfinite(a_lo) || !__builtin_isfinite(a_hi);
            const double f_lo = __builtin_fabs(a_lo), f_hi = __builtin_fabs(a_hi);
            const bool hi = f_hi < f_lo; // a tie takes the lower index
            const double fn = hi ? f_hi : f_lo;
            const int cn = hi ? c[x] + 1 : c[x] - 1, n = hi ? p + st[x] : p - st[x];
            const double w = f - fn;
            const bool usable = w > 0.0 && cn >= 1 && cn <= n1[x] - 1 && mask[n] == 1;
            nb[(size_t)x * nL + e] = usable ? n : p;
            wt[(size_t)x * nL + e] = usable ? w : 0.0;
        }
        const bool frozen = known ? known[p] == 1 : f < far;
        fz[e] = frozen ? 1 : 0;
        v[0] = frozen ? 1ull : 0ull;
        v[1] = frozen && !__builtin_isfinite(q[p]) ? 1ull : 0ull;
        v[2] = badphi ? 1ull : 0ull;
    }
    block_usum_out<MB_CH / 64>(v, threadIdx.x, part + (size_t)blockIdx.x * EXTB_NPART);
}

__global__ __launch_bounds__(MB_CH) void k_extb_init(double* __restrict__ q, const int* __restrict__ L, const unsigned char* __restrict__ fz, int nL)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    if (e < nL && !fz[e]) q[L[e]] = __builtin_nan("");
}

// Pass `pass` of a batch, first half.  q is read at list cells only and never written here.
__global__ __launch_bounds__(MB_CH) void k_extb_compute(const double* __restrict__ q, const int* __restrict__ L, const int* __restrict__ nb,
                                                        const double* __restrict__ wt, const unsigned char* __restrict__ fz, int nL,
                                                        double* __restrict__ nv, unsigned char* __restrict__ chg,
                                                        const unsigned long long* __restrict__ cnt, int pass)
{
#pragma clang fp contract(off)
    if (pass > 0 && cnt[pass - 1] == 0ull) return; // the pass before changed nothing: the call is over
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    if (e >= nL) return;
    if (fz[e]) {
        chg[e] = 0;
        return;
    }
    const double old = q[L[e]];
    double s[3], t[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double w = wt[(size_t)x * nL + e], qn = q[nb[(size_t)x * nL + e]];
        const bool used = w > 0.0 && qn == qn;
        s[x] = used ? w : 0.0;
        t[x] = used ? w * qn : 0.0;
    }
    const double den = (s[0] + s[1]) + s[2];
    const double nw = ((t[0] + t[1]) + t[2]) / den;
    nv[e] = nw;
    chg[e] = (den != 0.0 && !(nw == old)) ? 1 : 0;
}

// ... second half: the stores, at the lanes' own points, and the count of the pass
__global__ __launch_bounds__(MB_CH) void k_extb_commit(double* __restrict__ q, const int* __restrict__ L, const double* __restrict__ nv,
                                                       const unsigned char* __restrict__ chg, int nL, unsigned long long* __restrict__ cnt, int pass)
{
    if (pass > 0 && cnt[pass - 1] == 0ull) return;
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    const bool store = e < nL && chg[e] != 0;
    if (store) q[L[e]] = nv[e];
    const unsigned long long bal = __ballot(store);
    __shared__ unsigned red[MB_CH / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (unsigned)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = red[0];
        for (int w = 1; w < MB_CH / 64; ++w) t += red[w];
        if (t) atomicAdd(cnt + pass, (unsigned long long)t);
    }
}

// part: 2 words per block: the non-frozen list cells that hold a value, and those that are still NaN
__global__ __launch_bounds__(MB_CH) void k_extb_count(const double* __restrict__ q, const int* __restrict__ L, const unsigned char* __restrict__ fz,
                                                      int nL, unsigned long long* __restrict__ part)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long v[2] = {0ull, 0ull};
    if (e < nL && !fz[e]) {
        const double x = q[L[e]];
        v[0] = x == x ? 1ull : 0ull;
        v[1] = x == x ? 0ull : 1ull;
    }
    block_usum_out<MB_CH / 64>(v, threadIdx.x, part + (size_t)blockIdx.x * 2);
}

} // namespace lsf
