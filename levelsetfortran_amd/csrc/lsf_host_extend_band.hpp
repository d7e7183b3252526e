// lsf_host_extend_band.hpp -- host side of lsf_extend_field_band (kernels and design: lsf_extend_band.hpp; argument checks: lsf_host_args.hpp): the list, the
// plan pass with its error counts, the Jacobi passes enqueued CHECK_EVERY at a time, and the final count.  Included by lsf_api.hip
// inside its anonymous namespace.
#pragma once

// the arguments have passed extend_band_args_ok.  passes_done, changed_trace and info are written on LSF_OK only, q after every error
// has been decided.  Returns after the stream is synchronised.
int extend_band_core(double* d_q, const double* d_phi, const int32_t* d_mask, const int32_t* d_known, int nx, int ny, int nz, double dx,
                     double band, int max_passes, int* passes_done, int64_t* changed_trace, int trace_cap, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_count<true>(bl, nullptr, d_mask, nx, ny, nz, dx, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: the list is empty (no interior point with mask == 1)");
    // (a grid whose brick keys do not fit 32 bits keeps the memory order: only the locality of a chunk depends on the order)
    if ((rc = band_list_sort(bl, bl.keys_fit(), st))) return rc;
    const int* L = bl.L;
    if ((rc = ws(c.slot[S_XB_NB], (size_t)nL * 3 * sizeof(int)))) return rc;
    if ((rc = ws(c.slot[S_XB_WT], (size_t)nL * 3 * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_XB_NV], (size_t)nL * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_XB_FLAG], (size_t)nL * 2))) return rc;
    if ((rc = ws(c.slot[S_XB_CNT], CHECK_EVERY * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * EXTB_NPART * sizeof(unsigned long long)))) return rc;
    int* nb = (int*)c.slot[S_XB_NB].p;
    double* wt = (double*)c.slot[S_XB_WT].p;
    double* nv = (double*)c.slot[S_XB_NV].p;
    unsigned char* fz = (unsigned char*)c.slot[S_XB_FLAG].p;
    unsigned char* chg = fz + nL;
    unsigned long long* d_cnt = (unsigned long long*)c.slot[S_XB_CNT].p;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const double far = d_known ? 0.0 : band * dx;
    const dim3 grid((unsigned)nchunks), blk(MB_CH);

    // the plan: read-only on the caller's arrays; its counts decide the errors
    hipLaunchKernelGGL(k_extb_plan, grid, blk, 0, st, (const double*)d_q, d_phi, d_mask, d_known, L, nL, nx, ny, nz, far, nb, wt, fz, part);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> h((size_t)nchunks * EXTB_NPART);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long nfrozen = 0, nbadq = 0, nbadphi = 0;
    for (int b = 0; b < nchunks; ++b) // integer counts: no order in the result
        nfrozen += h[(size_t)b * EXTB_NPART], nbadq += h[(size_t)b * EXTB_NPART + 1], nbadphi += h[(size_t)b * EXTB_NPART + 2];
    if (nbadphi)
        return fail(LSF_ERR_INVALID, "lsf_extend_field_band: " + std::to_string(nbadphi) +
                                         " list cell(s) see a non-finite phi at themselves or at one of their six neighbours");
    if (nfrozen == 0)
        return fail(LSF_ERR_INVALID, d_known ? "lsf_extend_field_band: no frozen cell (known holds no 1 on a list cell)"
                                             : "lsf_extend_field_band: no frozen cell (no list cell with |phi| < band*dx)");
    if (nbadq) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: " + std::to_string(nbadq) + " frozen cell(s) hold a non-finite q");

    hipLaunchKernelGGL(k_extb_init, grid, blk, 0, st, d_q, L, (const unsigned char*)fz, nL);
    // the passes, a batch enqueued ahead of the device; the kernels behind a pass that changed nothing return at once, and the host
    // reads the counts of the batch -- which are the trace -- once
    std::vector<int64_t> trace;
    unsigned long long hc[CHECK_EVERY];
    bool stopped = false;
    while (!stopped && (int)trace.size() < max_passes) {
        const int batch = std::min(CHECK_EVERY, max_passes - (int)trace.size());
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)batch * sizeof(unsigned long long), st));
        for (int p = 0; p < batch; ++p) {
            hipLaunchKernelGGL(k_extb_compute, grid, blk, 0, st, (const double*)d_q, L, (const int*)nb, (const double*)wt, (const unsigned char*)fz, nL,
                               nv, chg, (const unsigned long long*)d_cnt, p);
            hipLaunchKernelGGL(k_extb_commit, grid, blk, 0, st, d_q, L, (const double*)nv, (const unsigned char*)chg, nL, d_cnt, p);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hc, d_cnt, (size_t)batch * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int p = 0; p < batch && !stopped; ++p) {
            trace.push_back((int64_t)hc[p]);
            stopped = hc[p] == 0; // that pass is counted
        }
    }

    hipLaunchKernelGGL(k_extb_count, grid, blk, 0, st, (const double*)d_q, L, (const unsigned char*)fz, nL, part);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h.data(), part, (size_t)nchunks * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long nreached = 0, nunreached = 0;
    for (int b = 0; b < nchunks; ++b) nreached += h[(size_t)b * 2], nunreached += h[(size_t)b * 2 + 1];
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] extend on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu frozen, %d pass(es), last count %lld, "
                        "%llu unreached\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, nfrozen, (int)trace.size(), (long long)trace.back(), nunreached);
    if (passes_done) *passes_done = (int)trace.size();
    if (changed_trace)
        for (int p = 0; p < (int)trace.size() && p < trace_cap; ++p) changed_trace[p] = trace[p];
    if (info) info[0] = nL, info[1] = (int64_t)nfrozen, info[2] = (int64_t)nreached, info[3] = (int64_t)nunreached;
    return LSF_OK;
}
