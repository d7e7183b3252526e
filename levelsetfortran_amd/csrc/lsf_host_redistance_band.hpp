// lsf_host_redistance_band.hpp -- host side of lsf_redistance_band (kernels and design: lsf_redistance_band.hpp; argument checks:
// lsf_host_args_redistance.hpp): the list, the foot launch with its error counts, the seed, the Jacobi passes of the fill enqueued
// CHECK_EVERY at a time, and the finish (the list, the pass driver and the finish of the counts: lsf_host_band.hpp).  Included by
// lsf_api.hip inside its anonymous namespace.
#pragma once

// the arguments have passed redistance_band_args_ok.  passes_done, changed_trace, change and info are written on LSF_OK only, phi after
// every error has been decided.  Returns after the stream is synchronised.
int redistance_band_core(double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, double near, int iters, double tol,
                         int max_passes, int* passes_done, int64_t* changed_trace, int trace_cap, double* change, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    BandList bl;
    if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, true, st))) return rc;
    const int nL = bl.nL, nchunks = bl.nchunks;
    if (nL <= 0) return fail(LSF_ERR_INVALID, "lsf_redistance_band: the list is empty (no interior point with mask == 1)");
    const int* L = bl.L;
    if ((rc = ws(c.slot[S_RD_VAL], (size_t)nL * 3 * sizeof(double)))) return rc;
    if ((rc = ws(c.slot[S_RD_FLAG], (size_t)nL * RDB_NFLAG))) return rc;
    if ((rc = ws(c.slot[S_RD_CNT], CHECK_EVERY * sizeof(unsigned long long)))) return rc;
    if ((rc = ws(c.slot[S_PART], (size_t)nchunks * RDB_NPART * sizeof(unsigned long long)))) return rc;
    double* dist = (double*)c.slot[S_RD_VAL].p;
    double *old = dist + nL, *nv = old + nL;
    unsigned char* fz = (unsigned char*)c.slot[S_RD_FLAG].p;
    unsigned char *neg = fz + nL, *nbits = neg + nL, *chg = nbits + nL;
    unsigned long long* d_cnt = (unsigned long long*)c.slot[S_RD_CNT].p;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const double tol_dx = tol * dx, near_dx = near * dx; // computed once
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, 0.0, 0.0, 0.0};
    const dim3 grid((unsigned)nchunks), blk(MB_CH);

    // the feet: read-only on the caller's arrays; the counts decide the errors
    hipLaunchKernelGGL(k_rdb_foot, grid, blk, 0, st, G, L, nL, iters, tol_dx, near_dx, dist, old, fz, neg, nbits, part);
    HIPCHK(hipGetLastError());
    unsigned long long tot[RDB_NPART];
    if ((rc = block_counts_finish(part, nchunks, RDB_NPART, tot, nullptr, st))) return rc;
    if (tot[6]) return fail(LSF_ERR_INVALID, "lsf_redistance_band: " + std::to_string(tot[6]) + " list cell(s) hold a non-finite phi");
    if (tot[0] == 0) return fail(LSF_ERR_INVALID, "lsf_redistance_band: no frozen cell (no list cell whose foot was found closer than near*dx)");

    hipLaunchKernelGGL(k_rdb_seed, grid, blk, 0, st, d_phi, L, (const double*)dist, nL);
    // the passes, a batch enqueued ahead of the device; the kernels behind a pass that lowered nothing return at once, and the host
    // reads the counts of the batch -- which are the trace -- once
    std::vector<int64_t> trace;
    rc = band_passes(trace, d_cnt, max_passes, 0, st, [&](int p) {
        hipLaunchKernelGGL(k_rdb_compute, grid, blk, 0, st, (const double*)d_phi, L, (const unsigned char*)fz, (const unsigned char*)nbits, nL, nx, ny,
                           dx, nv, chg, (const unsigned long long*)d_cnt, p);
        hipLaunchKernelGGL(k_extb_commit, grid, blk, 0, st, d_phi, L, (const double*)nv, (const unsigned char*)chg, nL, d_cnt, p);
    });
    if (rc) return rc;

    hipLaunchKernelGGL(k_rdb_finish, grid, blk, 0, st, d_phi, L, (const double*)dist, (const double*)old, (const unsigned char*)fz,
                       (const unsigned char*)neg, nL, part);
    HIPCHK(hipGetLastError());
    unsigned long long fin[RDB_NFIN]; // filled, unreached, the largest change as a bit pattern
    if ((rc = block_counts_finish(part, nchunks, RDB_NFIN, fin, nullptr, st, true))) return rc;
    const unsigned long long nfilled = fin[0], nunreached = fin[1];
    double maxchange;
    std::memcpy(&maxchange, &fin[2], sizeof(double));
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] redistance on the band: %d list cells (%.2f %% of the grid), %d chunks, %llu frozen, %d pass(es), last count %lld, "
                        "%llu unreached, largest change %.3e\n",
                nL, 100.0 * nL / (double)bl.n, nchunks, tot[0], (int)trace.size(), (long long)trace.back(), nunreached, maxchange);
    passes_report(trace, passes_done, changed_trace, trace_cap);
    if (change) *change = maxchange;
    if (info) {
        info[0] = nL, info[1] = (int64_t)tot[0], info[2] = (int64_t)nfilled, info[3] = (int64_t)nunreached;
        for (int q = 1; q <= 5; ++q) info[3 + q] = (int64_t)tot[q];
    }
    return LSF_OK;
}
