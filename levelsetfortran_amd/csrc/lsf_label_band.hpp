// lsf_label_band.hpp -- the 6-connected components of the cells of a list on either side of phi = iso: lsf_label_band
// (include/lsf.h; account: DESIGN.md section 4.22; driver: lsf_host_label_band.hpp).
//
// The list is lsf_reinit_band's,
//     LIST = { interior points with mask == 1 on entry },
// built by the same machinery (band_list_count<true> / band_list_sort: brick-sorted 32-bit point indices).  Every kernel is a plain
// launch, one lane per list entry, MB_CH consecutive entries -- a few neighbouring bricks -- per block.
//
// THE FOREST LIVES IN label ITSELF.  A labelled cell's word is the point index of another cell of its component and never larger than
// its own index; a cell whose word is its own index is a ROOT; a list cell of a class `side` leaves out holds -1 for the whole call.
// Nothing proportional to the grid is cleared or allocated.
//   k_label_check    read-only: per block the list cells with a non-finite d = phi - iso, the INSIDE cells (d < 0) and the OUTSIDE
//                    cells.  The host decides the errors on these counts before anything is written.
//   k_label_init     label[c] = c at labelled cells, -1 at the other list cells.
//   k_label_link     one pass, first half.  For a labelled cell and each of its +x, +y, +z neighbours that is a list cell (interior,
//                    mask == 1) of the same class (from phi at the neighbour): both cells are chased to their roots, and where the
//                    roots differ the smaller root goes to the larger root's word by a 32-bit atomicMin.  Every such edge adds one
//                    to the pass's counter (one atomic add per block).
//   k_label_flatten  second half: every labelled cell's word becomes its root.  No root changes here, so the forest is flat after it.
//   k_label_roots    per block the roots of each class.
//   k_label_collect  the roots, in any order, into a compact array (sorted afterwards by rocprim::radix_sort_keys).
//   k_label_slots    root t of the sorted array gets slot t < rows, or -1, at its point of the list build's staging buffer -- free after
//                    band_list_sort, written and read at root points only -- and row t of the table is initialised.
//   k_label_table    one launch over the list: each labelled cell goes into its root's row with 64-bit integer atomics (add, min,
//                    max), the lanes of a wave that share a slot reduced first.  Integer results carry no order.
//
// WHY PASSES AND NO RETRY.  No loop in these kernels depends on another lane's or block's progress.  A chase ends by its own data: it
// follows a word only while the word is smaller than the index it was read at, so the indices strictly decrease and a cycle is
// impossible whatever the memory holds; a word that is larger than its index or negative, or a chase beyond `cap` (= list cells)
// steps, sets *flag, which the host turns into LSF_ERR_HIP.  Two blocks may hang two different roots below one root at the same time:
// atomicMin keeps the smaller and the other link is LOST.  That costs a pass, never correctness: every word ever stored is the index
// of a cell of the same true component (the two ends of a link are face neighbours of one class, or roots of such), so the forest is
// at every moment a refinement of the truth; the lane that lost still counted its edge, so a further pass runs and finds the edge
// again.  A pass whose link launch counts nothing performed no atomic at all: it read a forest nobody was writing, flat since the
// launch before, and saw equal roots across every edge -- each true component is one tree, and its root, never larger than any
// member, is the component's smallest index.  The kernels enqueued behind such a pass return at once.
//
// The words of the forest are read and written with relaxed agent-scope atomics while other blocks may write them (link, flatten):
// a stale value is an older ancestor, still a cell of the component with a larger index, and only lengthens a chase.
//
// Bounds, by construction and not by a range check (the argument of lsf_advect_band.hpp): a list entry is an interior point, so its six
// face neighbours exist; a +1 neighbour is used only when it is interior itself and its mask word is 1, i.e. a list cell; a chase
// visits words it read from list cells' slots, checked to lie in [0, index); slot numbers are read at root points only, which
// k_label_slots wrote.  Lanes with e >= nL touch no memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsf_extend_band.hpp"

namespace lsf {

constexpr int LB_ROW = 10;    // LSF_LABEL_COMP_LEN: int64 words per row of the table
constexpr int LB_NCHECK = 3;  // partials per block of k_label_check: non-finite, INSIDE, OUTSIDE cells
constexpr int LB_NROOTS = 2;  // ... of k_label_roots: INSIDE roots, OUTSIDE roots
constexpr int LB_SIDE_INSIDE = 0, LB_SIDE_OUTSIDE = 1, LB_SIDE_BOTH = 2; // LSF_LABEL_INSIDE / OUTSIDE / BOTH

__device__ __forceinline__ int lb_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lb_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above cell c: follows the words while they decrease.  Ends by its own data (see above); `cap` is the hard limit.
__device__ __forceinline__ int lb_chase(const int* label, int c, int cap, int* flag)
{
    for (int it = 0;; ++it) {
        const int up = lb_load(label + c);
        if (up == c) return c;
        if (up > c || up < 0 || it >= cap) { // not a forest word, or longer than any chain of list cells
            atomicOr(flag, 1);
            return c;
        }
        c = up;
    }
}

__global__ __launch_bounds__(MB_CH) void k_label_check(const double* __restrict__ phi, const int* __restrict__ L, int nL, double iso,
                                                       unsigned long long* __restrict__ part)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long v[LB_NCHECK] = {0ull, 0ull, 0ull};
    if (e < nL) {
        const double d = phi[L[e]] - iso;
        const bool bad = !__builtin_isfinite(d);
        v[0] = bad ? 1ull : 0ull;
        v[1] = !bad && d < 0.0 ? 1ull : 0ull;
        v[2] = !bad && !(d < 0.0) ? 1ull : 0ull;
    }
    block_usum_out<MB_CH / 64>(v, threadIdx.x, part + (size_t)blockIdx.x * LB_NCHECK);
}

__global__ __launch_bounds__(MB_CH) void k_label_init(const double* __restrict__ phi, const int* __restrict__ L, int nL, double iso, int side,
                                                      int* __restrict__ label)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    if (e >= nL) return;
    const int p = L[e];
    const bool inside = phi[p] - iso < 0.0;
    const bool labelled = side == LB_SIDE_BOTH || (side == LB_SIDE_INSIDE) == inside;
    label[p] = labelled ? p : -1;
}

// Pass `pass` of a batch, first half.  cnt[pass] receives the edges found between two trees.
__global__ __launch_bounds__(MB_CH) void k_label_link(const double* __restrict__ phi, const int32_t* __restrict__ mask, const int* __restrict__ L,
                                                      int nL, int nx, int ny, int nz, double iso, int* label, unsigned long long* cnt, int pass,
                                                      int* flag)
{
    if (pass > 0 && cnt[pass - 1] == 0ull) return; // the pass before linked nothing: the labels are final
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned found = 0;
    if (e < nL) {
        const int p = L[e];
        if (lb_load(label + p) >= 0) { // (-1 stays -1 for the whole call)
            const int rs = nx + 1, ps = (nx + 1) * (ny + 1);
            const int k = p / ps, r = p - k * ps, j = r / rs, i = r - j * rs;
            const int c[3] = {i, j, k}, n1[3] = {nx, ny, nz}, st[3] = {1, rs, ps};
            const bool inside = phi[p] - iso < 0.0;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                if (c[x] + 1 > n1[x] - 1) continue; // a wall point is no list cell
                const int n = p + st[x];
                if (mask[n] != 1 || (phi[n] - iso < 0.0) != inside) continue;
                const int ra = lb_chase(label, p, nL, flag), rb = lb_chase(label, n, nL, flag);
                if (ra == rb) continue;
                atomicMin(label + (ra > rb ? ra : rb), ra > rb ? rb : ra);
                ++found;
            }
        }
    }
    found = block_usum<MB_CH / 64>(found, threadIdx.x);
    if (threadIdx.x == 0 && found) atomicAdd(cnt + pass, (unsigned long long)found);
}

// ... second half: every labelled cell's word becomes its root
__global__ __launch_bounds__(MB_CH) void k_label_flatten(const int* __restrict__ L, int nL, int* label, const unsigned long long* __restrict__ cnt,
                                                         int pass, int* flag)
{
    if (cnt[pass] == 0ull) return; // nothing was linked: the forest is as flat as the launch before left it
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    if (e >= nL) return;
    const int p = L[e], up = lb_load(label + p);
    if (up < 0 || up == p) return;
    const int r = lb_chase(label, p, nL, flag);
    if (r != up) lb_store(label + p, r);
}

__global__ __launch_bounds__(MB_CH) void k_label_roots(const double* __restrict__ phi, const int* __restrict__ L, int nL, double iso,
                                                       const int* __restrict__ label, unsigned long long* __restrict__ part)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    unsigned long long v[LB_NROOTS] = {0ull, 0ull};
    if (e < nL) {
        const int p = L[e];
        if (label[p] == p) {
            const bool inside = phi[p] - iso < 0.0;
            v[0] = inside ? 1ull : 0ull;
            v[1] = inside ? 0ull : 1ull;
        }
    }
    block_usum_out<MB_CH / 64>(v, threadIdx.x, part + (size_t)blockIdx.x * LB_NROOTS);
}

// roots[0 .. *head): the roots in any order; one returning atomic add per block that holds a root
__global__ __launch_bounds__(MB_CH) void k_label_collect(const int* __restrict__ L, int nL, const int* __restrict__ label, int* __restrict__ roots,
                                                         unsigned* head)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    const int p = e < nL ? L[e] : -1;
    const bool root = p >= 0 && label[p] == p;
    const unsigned long long bal = __ballot(root);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ unsigned red[MB_CH / 64 + 1];
    if (lane == 0) red[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < MB_CH / 64; ++w) t += red[w];
        red[MB_CH / 64] = t ? atomicAdd(head, t) : 0u;
    }
    __syncthreads();
    if (root) {
        unsigned at = red[MB_CH / 64];
        for (int w = 0; w < wave; ++w) at += red[w];
        roots[at + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = p;
    }
}

// sorted: the ncomp roots ascending.  The first `rows` get their slot number and an empty row, the others -1.
__global__ __launch_bounds__(MB_CH) void k_label_slots(const int* __restrict__ sorted, int ncomp, int rows, const double* __restrict__ phi,
                                                       double iso, int* __restrict__ slot, long long* __restrict__ table)
{
    const int t = blockIdx.x * MB_CH + threadIdx.x;
    if (t >= ncomp) return;
    const int r = sorted[t];
    slot[r] = t < rows ? t : -1;
    if (t >= rows) return;
    long long* row = table + (size_t)t * LB_ROW;
    row[0] = r, row[1] = 0, row[2] = phi[r] - iso < 0.0 ? -1 : 1;
    row[3] = row[5] = row[7] = 0x7fffffffffffffffll;
    row[4] = row[6] = row[8] = -1;
    row[9] = 0;
}

__device__ __forceinline__ int lb_wave_min(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// each labelled cell into its root's row.  The lanes of a wave that share a slot are reduced first: the loop below runs once per
// distinct slot of the wave (at most 64 times), on the wave's own data only.
__global__ __launch_bounds__(MB_CH) void k_label_table(const int32_t* __restrict__ mask, const int* __restrict__ L, int nL, int nx, int ny, int nz,
                                                       const int* __restrict__ label, const int* __restrict__ slot, int rows, long long* table)
{
    const int e = blockIdx.x * MB_CH + threadIdx.x;
    int s = -1, i = 0, j = 0, k = 0;
    bool edge = false;
    if (e < nL) {
        const int p = L[e], r = label[p];
        if (r >= 0 && r <= p && label[r] == r) { // (the forest is flat: always.  slot[] holds a number at root points only)
            s = slot[r];
            s = s < rows ? s : -1;
            const int rs = nx + 1, ps = (nx + 1) * (ny + 1);
            k = p / ps;
            const int q = p - k * ps;
            j = q / rs, i = q - j * rs;
            // a face neighbour that is no list cell: a wall point, or an interior point whose mask word is not 1
            edge = i == 1 || i == nx - 1 || j == 1 || j == ny - 1 || k == 1 || k == nz - 1 || mask[p - 1] != 1 || mask[p + 1] != 1 ||
                   mask[p - rs] != 1 || mask[p + rs] != 1 || mask[p - ps] != 1 || mask[p + ps] != 1;
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(s >= 0);
    while (pending) { // wave-uniform
        const int lead = __ffsll((long long)pending) - 1;
        const int sref = __shfl(s, lead, 64);
        const bool mine = s == sref;
        const unsigned long long set = __ballot(mine);
        const long long cells = __popcll(set), edges = __popcll(__ballot(mine && edge));
        const int big = 0x7fffffff;
        const int ilo = lb_wave_min(mine ? i : big), ihi = -lb_wave_min(mine ? -i : big);
        const int jlo = lb_wave_min(mine ? j : big), jhi = -lb_wave_min(mine ? -j : big);
        const int klo = lb_wave_min(mine ? k : big), khi = -lb_wave_min(mine ? -k : big);
        if (lane == lead) {
            long long* row = table + (size_t)sref * LB_ROW;
            __hip_atomic_fetch_add(row + 1, cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(row + 3, (long long)ilo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(row + 4, (long long)ihi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(row + 5, (long long)jlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(row + 6, (long long)jhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(row + 7, (long long)klo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(row + 8, (long long)khi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (edges) __hip_atomic_fetch_add(row + 9, edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        pending &= ~set;
    }
}

} // namespace lsf
