// lsf_host_extend_band.hpp -- host side of lsf_extend_field_band (kernels and design: lsf_extend_band.hpp; argument checks: lsf_host_args.hpp): the list, the
// plan pass with its error counts, the Jacobi passes enqueued CHECK_EVERY at a time, and the final count (the list, the pass driver and
// the finish of the counts: lsf_host_band.hpp).  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed extend_band_args_ok.  passes_done, changed_trace and info are written on LSF_OK only, q after every error
// has been decided.  Returns after the stream is synchronised.
int extend_band_core(double* d_q, const double* d_phi, const int32_t* d_mask, const int32_t* d_known, int nx, int ny, int nz, double dx,
                     double band, int max_passes, int* passes_done, int64_t* changed_trace, int trace_cap, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) return fail(LSF_ERR_INVALID, "lsf_extend_field_band: the list is empty (no interior point with mask == 1)");
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
    unsigned long long plan[EXTB_NPART];
    if ((rc = block_counts_finish(part, nchunks, EXTB_NPART, plan, nullptr, st))) return rc;
    const unsigned long long nfrozen = plan[0], nbadq = plan[1], nbadphi = plan[2];
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
    rc = band_passes(trace, d_cnt, max_passes, 0, st, [&](int p) {
        hipLaunchKernelGGL(k_extb_compute, grid, blk, 0, st, (const double*)d_q, L, (const int*)nb, (const double*)wt, (const unsigned char*)fz, nL, nv,
                           chg, (const unsigned long long*)d_cnt, p);
        hipLaunchKernelGGL(k_extb_commit, grid, blk, 0, st, d_q, L, (const double*)nv, (const unsigned char*)chg, nL, d_cnt, p);
    });
    if (rc) return rc;

    hipLaunchKernelGGL(k_extb_count, grid, blk, 0, st, (const double*)d_q, L, (const unsigned char*)fz, nL, part);
    HIPCHK(hipGetLastError());
    unsigned long long reach[2]; // reached, unreached
    if ((rc = block_counts_finish(part, nchunks, 2, reach, nullptr, st))) return rc;
    const unsigned long long nreached = reach[0], nunreached = reach[1];
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] extend on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu frozen, %d pass(es), last count %lld, "
                        "%llu unreached\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, nfrozen, (int)trace.size(), (long long)trace.back(), nunreached);
    passes_report(trace, passes_done, changed_trace, trace_cap);
    if (info) info[0] = nL, info[1] = (int64_t)nfrozen, info[2] = (int64_t)nreached, info[3] = (int64_t)nunreached;
    return LSF_OK;
}
