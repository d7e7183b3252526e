// lsf_block_reduce.hpp -- the order-free reductions of the band and point kernels: integer sums, and maxima and minima of bit patterns.
//
// Whatever order the operands meet in, the result is the same, so none of these reaches a statement: a kernel may use them for a
// count, or for the largest or smallest of non-negative doubles taken as their bit patterns (as unsigned integers these order like
// the numbers, +inf is the largest of them and every NaN, sign cleared, lies above +inf).  Floating-point SUMS do not belong here:
// their order is part of the statement of the call that forms them (wave_sum of lsf_kernels.hpp and the kernels that use it).
//
// Wave level: wave_usum, wave_usum_each, wave_umax_x, wave_umin over the 64 lanes, every lane gets the result.  Block level, over
// the NW waves of the block through an LDS array that the function owns: block_usum (one counter, the total comes back IN THREAD 0
// ONLY), block_usum_out (N counters, thread 0 writes the totals to memory) and block_umax (combines the NW wave maxima: its
// argument is a wave's result, the caller applies wave_umax_x first; valid in thread 0 only).  `tid` is the thread's linear index
// in the block, and every thread of the block must make the call: it holds a barrier.  A kernel calls at most one block-level
// function, once: each holds ONE barrier, so a second call could write an array that thread 0 still reads.  A kernel that
// reduces more than one kind of thing -- counts AND a maximum or minimum (k_curvature_band, k_evb_check, k_evb_check_finish,
// k_advect_band_close), counts beside floating-point values (the two scans, k_measure_band) -- uses the wave-level pieces with LDS
// arrays and one barrier of its own.
#pragma once
#include <hip/hip_runtime.h>

namespace lsf {

template <typename T>
__device__ __forceinline__ T wave_usum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the number of lanes of the wave whose flag is set, in every lane: one ballot and one population count, both scalar
__device__ __forceinline__ unsigned long long wave_count(bool f) { return (unsigned long long)__popcll(__ballot(f)); }

// butterfly maximum over the 64 lanes, the lane exchanges of wave_sum_x (lsf_kernels.hpp): no LDS round trips
__device__ __forceinline__ unsigned long long wave_umax_x(unsigned long long v)
{
    auto lo = [](unsigned long long x) { return (int)(unsigned)(x & 0xffffffffull); };
    auto hi = [](unsigned long long x) { return (int)(unsigned)(x >> 32); };
    auto join = [](int l, int h) { return ((unsigned long long)(unsigned)h << 32) | (unsigned long long)(unsigned)l; };
    auto mx = [](unsigned long long a, unsigned long long b) { return a > b ? a : b; };
    {   // partner 32 lanes away
        const auto l = __builtin_amdgcn_permlane32_swap(lo(v), lo(v), false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi(v), hi(v), false, false);
        v = mx(join(l[0], h[0]), join(l[1], h[1]));
    }
    {   // 16 lanes away
        const auto l = __builtin_amdgcn_permlane16_swap(lo(v), lo(v), false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi(v), hi(v), false, false);
        v = mx(join(l[0], h[0]), join(l[1], h[1]));
    }
    // 8 lanes away: row_ror:8
    v = mx(v, join(__builtin_amdgcn_update_dpp(0, lo(v), 0x128, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, hi(v), 0x128, 0xf, 0xf, false)));
    {   // 4 lanes away: row_ror:12 for banks 0 and 2, row_ror:4 for banks 1 and 3
        int l = __builtin_amdgcn_update_dpp(0, lo(v), 0x12c, 0xf, 0x5, false);
        l = __builtin_amdgcn_update_dpp(l, lo(v), 0x124, 0xf, 0xa, false);
        int h = __builtin_amdgcn_update_dpp(0, hi(v), 0x12c, 0xf, 0x5, false);
        h = __builtin_amdgcn_update_dpp(h, hi(v), 0x124, 0xf, 0xa, false);
        v = mx(v, join(l, h));
    }
    // 2 and 1 lanes away: quad_perm [2,3,0,1] and [1,0,3,2]
    v = mx(v, join(__builtin_amdgcn_update_dpp(0, lo(v), 0x4e, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, hi(v), 0x4e, 0xf, 0xf, false)));
    v = mx(v, join(__builtin_amdgcn_update_dpp(0, lo(v), 0xb1, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, hi(v), 0xb1, 0xf, 0xf, false)));
    return v;
}

__device__ __forceinline__ unsigned long long wave_umin(unsigned long long v) { return ~wave_umax_x(~v); }

// several counters at once, in place: the exchanges of one distance are issued together
template <typename... T>
__device__ __forceinline__ void wave_usum_each(T&... v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ((v += __shfl_xor(v, o, 64)), ...);
}

// r[0] + ... + r[N-1] of per-wave results in LDS, pairwise: (r0 + r1) + (r2 + r3) for four waves
template <int N, typename T>
__device__ __forceinline__ T lds_usum(const T* r, int stride)
{
    if constexpr (N == 1) return r[0];
    else return lds_usum<N / 2>(r, stride) + lds_usum<N - N / 2>(r + (N / 2) * stride, stride);
}

template <int NW, typename T>
__device__ __forceinline__ T block_usum(T v, int tid)
{
    __shared__ T red[NW];
    v = wave_usum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) v = lds_usum<NW>(red, 1);
    return v;
}

// the block's sums of N per-lane counters, written by thread 0 to out[0 .. N).  PER_WAVE: v already holds the wave's totals
// (wave_count, wave_usum) and only the waves are added.
template <int NW, bool PER_WAVE = false, typename T, int N>
__device__ __forceinline__ void block_usum_out(T (&v)[N], int tid, T* out)
{
    __shared__ T red[NW][N];
    if constexpr (!PER_WAVE)
#pragma unroll
        for (int m = 0; m < N; ++m) v[m] = wave_usum(v[m]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int m = 0; m < N; ++m) red[tid >> 6][m] = v[m];
    __syncthreads();
    if (tid == 0)
#pragma unroll
        for (int m = 0; m < N; ++m) out[m] = lds_usum<NW>(&red[0][m], N);
}

// the largest of the NW wave maxima w (each the result of wave_umax_x)
template <int NW>
__device__ __forceinline__ unsigned long long block_umax(unsigned long long w, int tid)
{
    __shared__ unsigned long long red[NW];
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        w = red[0];
        for (int q = 1; q < NW; ++q) w = red[q] > w ? red[q] : w;
    }
    return w;
}

} // namespace lsf
