// lsf_host_band.hpp -- what the host sides of the calls that work on a list of cells or on points share: the list itself (BandList, its
// two phases and band_list_build, the masked list in one call), the runtime flags as template arguments (with_flags), the finish of the
// per-block words (block_counts_finish), and the driver of the passes that are enqueued CHECK_EVERY at a time (band_passes).  Included by
// lsf_api.hip inside its anonymous namespace, before every host that uses them.
#pragma once

// The list of cells a band call works on (the min/max flow of lsf_host_minmax.hpp, lsf_reinit_band and every call after it), built once per
// call in two phases; the min/max flow decides between them, every other call goes through band_list_build.  Staging: the first n ints of
// S_PONG -- asked for at n doubles, the size at which the dense min/max executors and the reinit on the band want their second field, so
// that no call frees and allocates the buffer a second time.
struct BandList {
    int nL = 0, nchunks = 0;       // cells (after band_list_count), chunks of MB_CH cells
    int* L = nullptr;              // S_MB_L: point indices, sorted by brick key or in memory order (after band_list_sort)
    const unsigned* key = nullptr; // S_MB_KEY: the sorted brick keys; NULL for a list in memory order
    size_t n = 0;                  // points of the grid
    long nblk = 0;                 // blocks of the scan
    int nx = 0, ny = 0, nz = 0, nbx = 0, nby = 0; // ... bricks along x, y
    int *staging = nullptr, *counts = nullptr, *offsets = nullptr;
    // brick keys are 32-bit: beyond that a list can only stay in memory order
    bool keys_fit() const { return (double)nbx * nby * cdiv(nz + 1, 4) * 256.0 <= 4.0e9; }
};
// phase 1: the cells per scan block and their number.  MASK_ONLY: the cells of the caller's mask; otherwise the cells that can ever be
// in the band of phi (k_mb_collect).  Waits for the device.
template <bool MASK_ONLY>
int band_list_count(BandList& bl, const double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    bl.n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    bl.nx = nx, bl.ny = ny, bl.nz = nz, bl.nbx = cdiv(nx + 1, 8), bl.nby = cdiv(ny + 1, 8);
    bl.nblk = (long)((bl.n + MB_SCAN - 1) / MB_SCAN);
    if ((rc = ws(c.slot[S_PONG], bl.n * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_MB_CNT], (size_t)(2 * bl.nblk + 8) * sizeof(int)))) return rc;
    bl.staging = (int*)c.slot[S_PONG].p, bl.counts = (int*)c.slot[S_MB_CNT].p;
    bl.offsets = bl.counts + ((bl.nblk + 3) & ~3L); // 16-byte aligned like counts (k_mb_offsets moves vectors)
    hipLaunchKernelGGL(k_mb_collect<MASK_ONLY>, dim3((unsigned)bl.nblk), dim3(256), 0, st, MASK_ONLY ? nullptr : d_phi, d_mask, nx, ny, nz, dx,
                       bl.staging, bl.counts);
    hipLaunchKernelGGL(k_mb_offsets, dim3(1), dim3(1024), 0, st, (const int*)bl.counts, bl.nblk, bl.offsets);
    HIPCHK(hipMemcpyAsync(&bl.nL, bl.offsets + bl.nblk, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bl.nchunks = (bl.nL + MB_CH - 1) / MB_CH;
    return LSF_OK;
}
// phase 2 (nL > 0): the list in memory order and its brick keys, then -- `sort`, which needs keys_fit() -- sorted by key.  Both pairs of
// arrays live in S_MB_KEY and S_MB_L; the sort's temporary storage is the staging buffer, free again once its segments have been
// gathered (in stream order).
int band_list_sort(BandList& bl, bool sort, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const size_t nL = (size_t)bl.nL;
    if ((rc = ws(c.slot[S_MB_L], nL * sizeof(int)))) return rc;
    if ((rc = ws(c.slot[S_MB_KEY], nL * 3 * sizeof(int)))) return rc;
    bl.L = (int*)c.slot[S_MB_L].p;
    unsigned* key_in = (unsigned*)c.slot[S_MB_KEY].p;
    unsigned* key = key_in + nL;
    int* L_in = (int*)(key + nL);
    hipLaunchKernelGGL(k_mb_gather, dim3((unsigned)((bl.nblk + 3) / 4)), dim3(256), 0, st, (const int*)bl.staging, (const int*)bl.counts,
                       (const int*)bl.offsets, bl.nblk, bl.nx + 1, bl.ny + 1, bl.nbx, bl.nby, sort ? L_in : bl.L, key_in);
    if (!sort) return LSF_OK;
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_in, key, L_in, bl.L, nL, 0, 32, st));
    void* tmp = bl.staging;
    if (tmp_bytes > bl.n * sizeof(int)) { // tiny grids
        if ((rc = ws(c.slot[S_MB_TMP], tmp_bytes))) return rc;
        tmp = c.slot[S_MB_TMP].p;
    }
    HIPCHK(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key, L_in, bl.L, nL, 0, 32, st));
    bl.key = key;
    return LSF_OK;
}
// The list of the caller's mask in one call: both phases, the second where the list holds a cell.  An empty list (bl.nL == 0, nothing
// sorted) is LSF_OK: what it means is the caller's.  The band calls ask for the brick order (sort), which they get where keys_fit() -- a
// grid whose brick keys do not fit 32 bits keeps the memory order: no result depends on the order of the list beyond the order of a sum,
// which is then that one and still a function of the mask alone; only the locality of a chunk does -- and the calls on points keep the
// memory order.
int band_list_build(BandList& bl, const int32_t* d_mask, int nx, int ny, int nz, double dx, bool sort, hipStream_t st)
{
    if (int rc = band_list_count<true>(bl, nullptr, d_mask, nx, ny, nz, dx, st)) return rc;
    return bl.nL > 0 ? band_list_sort(bl, sort && bl.keys_fit(), st) : LSF_OK;
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for the runtime values b0, b1, ...: the one place where flags become
// template arguments.  Every combination of the flags is instantiated; an f that has no kernel for one says so with if constexpr.
template <class F>
void with_flags(F&& f)
{
    f();
}
template <class F, class... B>
void with_flags(F&& f, bool b, B... rest)
{
    if (b)
        with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else
        with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// The finish of a launch whose blocks each left npart words in part: copies them home, synchronises the stream and combines them in
// block order into tot[0..npart) -- sums, and with last_is_max the last word as a maximum of bit patterns (integers: no order in the
// result).  Fills info, where one is given, with the sums.
int block_counts_finish(const unsigned long long* part, int nblocks, int npart, unsigned long long* tot, int64_t* info, hipStream_t st,
                        bool last_is_max = false)
{
    std::vector<unsigned long long> h((size_t)nblocks * npart);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int nsum = npart - (last_is_max ? 1 : 0);
    for (int m = 0; m < npart; ++m) tot[m] = 0;
    for (int b = 0; b < nblocks; ++b) {
        for (int m = 0; m < nsum; ++m) tot[m] += h[(size_t)b * npart + m];
        if (last_is_max) tot[nsum] = std::max(tot[nsum], h[(size_t)b * npart + nsum]);
    }
    if (info)
        for (int m = 0; m < nsum; ++m) info[m] = (int64_t)tot[m];
    return LSF_OK;
}

// Up to max_passes passes, a batch of at most CHECK_EVERY enqueued ahead of the device.  enqueue(p) puts pass p of a batch on the
// stream; it adds what it changed to d_cnt[p], and the kernels behind a pass that changed nothing return at once.  Per batch: the counts
// of the batch cleared, the launches, one copy home and one wait.  The copy is nread words of d_cnt (at most BAND_PASS_WORDS; 0: the
// counts of the batch alone).  seen(words), where given, looks at the words of a batch before they are absorbed and may refuse.  The
// counts up to and including the first zero are the trace: that pass is counted.
constexpr int BAND_PASS_WORDS = CHECK_EVERY + 1;
template <class Enqueue, class Seen>
int band_passes(std::vector<int64_t>& trace, unsigned long long* d_cnt, int max_passes, int nread, hipStream_t st, Enqueue&& enqueue, Seen&& seen)
{
    unsigned long long hc[BAND_PASS_WORDS];
    if (nread > BAND_PASS_WORDS) return fail(LSF_ERR_INVALID, "band_passes: more words per batch than its buffer holds");
    bool stopped = false;
    while (!stopped && (int)trace.size() < max_passes) {
        const int batch = std::min(CHECK_EVERY, max_passes - (int)trace.size());
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)batch * sizeof(unsigned long long), st));
        for (int p = 0; p < batch; ++p) enqueue(p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hc, d_cnt, (size_t)(nread ? nread : batch) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = seen((const unsigned long long*)hc)) return rc;
        for (int p = 0; p < batch && !stopped; ++p) {
            trace.push_back((int64_t)hc[p]);
            stopped = hc[p] == 0;
        }
    }
    return LSF_OK;
}
template <class Enqueue>
int band_passes(std::vector<int64_t>& trace, unsigned long long* d_cnt, int max_passes, int nread, hipStream_t st, Enqueue&& enqueue)
{
    return band_passes(trace, d_cnt, max_passes, nread, st, enqueue, [](const unsigned long long*) { return LSF_OK; });
}
// the report of the passes: their number, and as much of the trace as the caller has room for
void passes_report(const std::vector<int64_t>& trace, int* passes_done, int64_t* changed_trace, int trace_cap)
{
    if (passes_done) *passes_done = (int)trace.size();
    if (changed_trace)
        for (int p = 0; p < (int)trace.size() && p < trace_cap; ++p) changed_trace[p] = trace[p];
}
