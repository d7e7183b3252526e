// lsf_host_label_band.hpp -- host side of lsf_label_band (kernels and design: lsf_label_band.hpp; argument checks: lsf_host_args.hpp): the list, the check
// launch with its error counts, the link / flatten passes enqueued CHECK_EVERY at a time, and the table of components (the list, the
// pass driver and the finish of the counts: lsf_host_band.hpp).  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed label_band_args_ok.  comp, ncomp and info are host arrays and are written on LSF_OK only, d_label after every
// error has been decided.  Returns after the stream is synchronised.
int label_band_core(const double* d_phi, const int32_t* d_mask, int32_t* d_label, int nx, int ny, int nz, double iso, int side, int max_passes,
                    int64_t* comp, int comp_cap, int64_t* ncomp, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, 1.0, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) { // empty list: nothing to do, nothing written
        if (info)
            for (int q = 0; q < LSF_LABEL_INFO_LEN; ++q) info[q] = 0;
        if (ncomp) *ncomp = 0;
        return LSF_OK;
    }
    const int* L = bl.L;
    int* label = (int*)d_label;
    constexpr int NPART = LB_NCHECK > LB_NROOTS ? LB_NCHECK : LB_NROOTS;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * NPART * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_LB_CNT], (CHECK_EVERY + 2) * sizeof(unsigned long long)))) return rc;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    unsigned long long* d_cnt = (unsigned long long*)c.slot[S_LB_CNT].p; // one count per pass of a batch | the chase flag | the head of the roots
    int* d_flag = (int*)(d_cnt + CHECK_EVERY);
    unsigned* d_head = (unsigned*)(d_cnt + CHECK_EVERY + 1);
    const dim3 grid((unsigned)nchunks), blk(MB_CH);

    // the check: read-only on the caller's arrays; its counts decide the errors
    hipLaunchKernelGGL(k_label_check, grid, blk, 0, st, d_phi, L, nL, iso, part);
    HIPCHK(hipGetLastError());
    unsigned long long chk[LB_NCHECK];
    if ((rc = block_counts_finish(part, nchunks, LB_NCHECK, chk, nullptr, st))) return rc;
    const unsigned long long nbad = chk[0], nin = chk[1], nout = chk[2];
    if (nbad) return fail(LSF_ERR_INVALID, "lsf_label_band: " + std::to_string(nbad) + " list cell(s) hold a non-finite phi - iso");
    const unsigned long long nlabelled = side == LSF_LABEL_BOTH ? nin + nout : side == LSF_LABEL_INSIDE ? nin : nout;

    HIPCHK(hipMemsetAsync(d_cnt + CHECK_EVERY, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_label_init, grid, blk, 0, st, d_phi, L, nL, iso, side, label);
    // the passes, a batch enqueued ahead of the device; the kernels behind a pass that linked nothing return at once, and the host
    // reads the counts of the batch and the chase flag once
    std::vector<int64_t> trace;
    rc = band_passes(
        trace, d_cnt, max_passes, CHECK_EVERY + 1, st,
        [&](int p) {
            hipLaunchKernelGGL(k_label_link, grid, blk, 0, st, d_phi, d_mask, L, nL, nx, ny, nz, iso, label, d_cnt, p, d_flag);
            hipLaunchKernelGGL(k_label_flatten, grid, blk, 0, st, L, nL, label, (const unsigned long long*)d_cnt, p, d_flag);
        },
        [](const unsigned long long* hc) {
            if ((int)hc[CHECK_EVERY] == 0) return (int)LSF_OK;
            return fail(LSF_ERR_HIP, "lsf_label_band: a chase met a word that is no forest word, or ran beyond the number of list cells "
                                     "(label was written by someone else during the call?)");
        });
    if (rc) return rc;
    const int passes = (int)trace.size();
    const unsigned long long last = (unsigned long long)trace.back(); // (max_passes >= 1: there is one)

    // the roots of each class
    hipLaunchKernelGGL(k_label_roots, grid, blk, 0, st, d_phi, L, nL, iso, (const int*)label, part);
    HIPCHK(hipGetLastError());
    unsigned long long roots_of[LB_NROOTS];
    if ((rc = block_counts_finish(part, nchunks, LB_NROOTS, roots_of, nullptr, st))) return rc;
    const unsigned long long rin = roots_of[0], rout = roots_of[1];
    const size_t nc = (size_t)(rin + rout);
    const int rows = (int)std::min(nc, (size_t)comp_cap);
    std::vector<int64_t> table((size_t)rows * LB_ROW);
    if (rows > 0) {
        // the roots, sorted ascending; the first `rows` get a slot number at their point of the staging buffer of the list build
        // (free since band_list_sort, written and read at root points only) and a row
        size_t tmp_bytes = 0;
        HIPCHK(rocprim::radix_sort_keys(nullptr, tmp_bytes, (unsigned*)nullptr, (unsigned*)nullptr, nc, 0, 32, st));
        const size_t keys_bytes = (nc * sizeof(int) + 255) & ~(size_t)255;
        if ((rc = ws(c.slot[S_LB_ROOTS], 2 * keys_bytes + tmp_bytes))) return rc;
        if ((rc = ws(c.slot[S_LB_ROWS], (size_t)rows * LB_ROW * sizeof(long long)))) return rc;
        int* roots = (int*)c.slot[S_LB_ROOTS].p;
        int* sorted = (int*)((char*)c.slot[S_LB_ROOTS].p + keys_bytes);
        void* tmp = (char*)c.slot[S_LB_ROOTS].p + 2 * keys_bytes;
        long long* d_rows = (long long*)c.slot[S_LB_ROWS].p;
        hipLaunchKernelGGL(k_label_collect, grid, blk, 0, st, L, nL, (const int*)label, roots, d_head);
        HIPCHK(rocprim::radix_sort_keys(tmp, tmp_bytes, (unsigned*)roots, (unsigned*)sorted, nc, 0, 32, st));
        hipLaunchKernelGGL(k_label_slots, dim3((unsigned)((nc + MB_CH - 1) / MB_CH)), blk, 0, st, (const int*)sorted, (int)nc, rows, d_phi, iso,
                           bl.staging, d_rows);
        hipLaunchKernelGGL(k_label_table, grid, blk, 0, st, d_mask, L, nL, nx, ny, nz, (const int*)label, (const int*)bl.staging, rows, d_rows);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(table.data(), d_rows, table.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] components on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu labelled, %llu + %llu components, "
                        "%d pass(es), last count %llu\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, nlabelled, rin, rout, passes, last);
    if (comp)
        for (size_t q = 0; q < table.size(); ++q) comp[q] = table[q];
    if (ncomp) *ncomp = (int64_t)nc;
    if (info) {
        info[0] = nL, info[1] = (int64_t)nlabelled, info[2] = (int64_t)rin, info[3] = (int64_t)rout, info[4] = passes, info[5] = (int64_t)last;
        info[6] = (int64_t)((unsigned long long)nL - nlabelled), info[7] = 0;
    }
    return LSF_OK;
}
