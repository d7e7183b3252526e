// lsf_host_reseed.hpp -- host side of lsf_reseed_points (kernels and design: lsf_reseed_points.hpp; argument checks:
// lsf_host_args_points.hpp): the launches, the totals the host reads between them, and the marker set kept for the calling thread
// until lsf_reseed_get copies it out.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the marker set of the last reseed of this thread: one device allocation, owned here until a get or a new reseed
struct ReseedResult {
    bool have = false;
    int device = 0;
    int nout = 0;
    double* x = nullptr; // (nout,3) in Fortran order, then rad (nout), then src (nout, int32)
};
thread_local ReseedResult g_reseed;

void reseed_drop()
{
    if (g_reseed.x) (void)hipFree(g_reseed.x);
    g_reseed = ReseedResult{};
}

// the arguments have passed reseed_points_args_ok and every array is device memory.  d_status, nout and info are written on LSF_OK
// only.  Returns after the stream is synchronised.
int reseed_core(const double* d_phi, const int32_t* d_mask, int nx, int ny, int nz, double dx, const double xLo[3], const double* d_pts,
                const double* d_rad, int npts, int per_cell, double rmin, double rmax, double band, int order, int iters, double tol, uint64_t seed,
                int32_t* d_status, int* nout, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1), np = (size_t)npts;
    // the cells that are looked at: the list of the mask, in memory order, or the grid
    BandList bl;
    size_t nwork = n;
    const int* L = nullptr;
    if (d_mask) {
        if ((rc = band_list_build(bl, d_mask, nx, ny, nz, dx, false, st))) return rc;
        nwork = (size_t)std::max(bl.nL, 0), L = bl.L; // (an empty list: no L)
    }
    const size_t tilesK = (np + RS_BLOCK - 1) / RS_BLOCK, tilesC = (nwork + RS_BLOCK - 1) / RS_BLOCK;
    if ((rc = ws(c.slot[S_RS_COUNT], n * sizeof(int)))) return rc;
    if ((rc = ws(c.slot[S_RS_RANK], std::max(nwork, (size_t)1) * sizeof(uint32_t)))) return rc;
    if ((rc = ws(c.slot[S_RS_OLD], std::max(np, (size_t)1) * (sizeof(double) + sizeof(uint32_t) + sizeof(int32_t))))) return rc;
    if ((rc = ws(c.slot[S_RS_SCAN], (tilesK + tilesC + 2) * (sizeof(uint2) + sizeof(ulonglong2))))) return rc;
    if ((rc = ws(c.slot[S_RS_CTL], RS_CTL_LEN * sizeof(unsigned long long)))) return rc;
    PointPlan pp;
    if ((rc = point_plan(pp, np, RS_BLOCK, RS_NPART))) return rc; // (pp.nblocks == tilesK)
    int* count = (int*)c.slot[S_RS_COUNT].p;
    uint32_t* rankC = (uint32_t*)c.slot[S_RS_RANK].p;
    double* radn = (double*)c.slot[S_RS_OLD].p;
    uint32_t* rankK = (uint32_t*)(radn + std::max(np, (size_t)1));
    int32_t* statK = (int32_t*)(rankK + std::max(np, (size_t)1));
    ulonglong2* offK = (ulonglong2*)c.slot[S_RS_SCAN].p; // 16-byte entries first, then the 8-byte ones
    ulonglong2* offC = offK + tilesK + 1;
    uint2* sumsK = (uint2*)(offC + tilesC + 1);
    uint2* sumsC = sumsK + tilesK + 1;
    unsigned long long *ctl = (unsigned long long*)c.slot[S_RS_CTL].p, *part = pp.part;
    HIPCHK(hipMemsetAsync(ctl, 0, RS_CTL_LEN * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(count, 0, n * sizeof(int), st));
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const RsParams P{per_cell, iters, rmin, band, rmin * dx, rmax * dx, band * dx, tol * dx, (unsigned long long)seed};
    const dim3 blk(RS_BLOCK);
    if (np) {
        if (d_mask)
            hipLaunchKernelGGL((k_rs_classify<true>), dim3((unsigned)tilesK), blk, 0, st, G, P, d_pts, d_rad, npts, statK, radn, rankK, sumsK, count, part);
        else
            hipLaunchKernelGGL((k_rs_classify<false>), dim3((unsigned)tilesK), blk, 0, st, G, P, d_pts, d_rad, npts, statK, radn, rankK, sumsK, count, part);
    }
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(XS_SCAN_T), 0, st, (const uint2*)sumsK, (long)tilesK, offK, ctl + RS_NKEPT);
    if (nwork) {
        if (d_mask)
            hipLaunchKernelGGL((k_rs_cells<true>), dim3((unsigned)tilesC), blk, 0, st, G, P, L, nwork, (const int*)count, rankC, sumsC, ctl);
        else
            hipLaunchKernelGGL((k_rs_cells<false>), dim3((unsigned)tilesC), blk, 0, st, G, P, L, nwork, (const int*)count, rankC, sumsC, ctl);
    }
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(XS_SCAN_T), 0, st, (const uint2*)sumsC, (long)tilesC, offC, ctl + RS_NCAND);
    HIPCHK(hipGetLastError());
    unsigned long long h[RS_CTL_LEN];
    HIPCHK(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
    unsigned long long tot[RS_NPART] = {0, 0, 0, 0, 0, 0, 0};
    if (np) {
        if ((rc = block_counts_finish(part, pp.nblocks, RS_NPART, tot, nullptr, st))) return rc; // (synchronises)
    } else
        HIPCHK(hipStreamSynchronize(st));
    const unsigned long long ncand = h[RS_NCAND], nkept = h[RS_NKEPT];
    if ((unsigned long long)np + ncand > 2147483647ull)
        return fail(LSF_ERR_INVALID, "lsf_reseed_points: " + std::to_string((unsigned long long)np + ncand) + " old markers and candidates, more than 2^31 - 1");
    unsigned long long nacc = 0;
    const size_t tilesA = (size_t)((ncand + RS_BLOCK - 1) / RS_BLOCK);
    double *cpts = nullptr, *crad = nullptr;
    uint32_t* rankA = nullptr;
    ulonglong2* offA = nullptr;
    if (ncand) {
        if ((rc = ws(c.slot[S_RS_CAND], (size_t)ncand * (4 * sizeof(double) + sizeof(uint32_t)) + (tilesA + 1) * (sizeof(uint2) + sizeof(ulonglong2))))) return rc;
        offA = (ulonglong2*)c.slot[S_RS_CAND].p;
        cpts = (double*)(offA + tilesA + 1);
        crad = cpts + 3 * ncand;
        uint2* sumsA = (uint2*)(crad + ncand);
        rankA = (uint32_t*)(sumsA + tilesA + 1);
        const dim3 ga((unsigned)tilesA);
        with_flags(
            [&](auto CU, auto HM) {
                hipLaunchKernelGGL((k_rs_candidates<decltype(CU)::value, decltype(HM)::value>), ga, blk, 0, st, G, P, L, nwork, (const uint32_t*)rankC,
                                   (const ulonglong2*)offC, ncand, cpts, crad, rankA, sumsA, ctl);
            },
            order == LSF_SAMPLE_CUBIC, d_mask != nullptr);
        hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(XS_SCAN_T), 0, st, (const uint2*)sumsA, (long)tilesA, offA, ctl + RS_NACC);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        nacc = h[RS_NACC];
    }
    const size_t no = (size_t)(nkept + nacc); // <= npts + ncand <= 2^31 - 1
    ReseedResult& R = g_reseed;
    if (no) {
        if (hipMalloc((void**)&R.x, no * (4 * sizeof(double) + sizeof(int32_t))) != hipSuccess) {
            R.x = nullptr;
            return fail(LSF_ERR_HIP, "lsf_reseed_points: out of device memory for the marker set");
        }
        double* rout = R.x + 3 * no;
        int32_t* src = (int32_t*)(rout + no);
        if (nkept)
            hipLaunchKernelGGL(k_rs_emit_kept, dim3((unsigned)tilesK), blk, 0, st, d_pts, (const double*)radn, npts, (const uint32_t*)rankK,
                               (const ulonglong2*)offK, R.x, rout, src, no);
        if (nacc)
            hipLaunchKernelGGL(k_rs_emit_new, dim3((unsigned)tilesA), blk, 0, st, (const double*)cpts, (const double*)crad, ncand, (const uint32_t*)rankA,
                               (const ulonglong2*)offA, (size_t)nkept, R.x, rout, src, no);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && d_status && np) e = hipMemcpyAsync(d_status, statK, np * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            reseed_drop();
            return fail(LSF_ERR_HIP, std::string("lsf_reseed_points: ") + hipGetErrorString(e));
        }
    } else if (d_status && np) {
        HIPCHK(hipMemcpyAsync(d_status, statK, np * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    R.have = true, R.device = g_device, R.nout = (int)no;
    *nout = (int)no;
    if (info) {
        for (int m = 0; m < 6; ++m) info[m] = (int64_t)tot[m];
        info[6] = (int64_t)h[RS_ELIG], info[7] = (int64_t)ncand, info[8] = (int64_t)nacc;
        info[9] = (int64_t)h[RS_REJ_EARLY], info[10] = (int64_t)h[RS_REJ_LATE];
        info[11] = (int64_t)h[RS_OVER], info[12] = (int64_t)h[RS_MAXC], info[13] = (int64_t)tot[6];
    }
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] reseed: %d markers, %llu kept; %zu cells looked at, %llu eligible, %llu candidates, %llu accepted\n", npts, nkept, nwork,
                h[RS_ELIG], ncand, nacc);
    return LSF_OK;
}

// the kept marker set -> the caller's arrays (host: st unused; device: on st), then released.  src_out may be NULL.
int reseed_get(double* pts_out, double* rad_out, int32_t* src_out, bool to_device, hipStream_t st)
{
    ReseedResult& R = g_reseed;
    if (!R.have) return fail(LSF_ERR_INVALID, "lsf_reseed_get without a kept lsf_reseed_points result");
    if (R.nout == 0) { // an empty set: nothing to write
        reseed_drop();
        return LSF_OK;
    }
    if (!pts_out || !rad_out) return fail(LSF_ERR_INVALID, "lsf_reseed_get: NULL pts_out or rad_out");
    int rc = ensure_device();
    if (rc) return rc;
    if (R.device != g_device) return fail(LSF_ERR_INVALID, "lsf_reseed_get: the result was kept on another device (lsf_set_device)");
    const size_t no = (size_t)R.nout;
    const double* rout = R.x + 3 * no;
    const int32_t* src = (const int32_t*)(rout + no);
    if (to_device) {
        HIPCHK(hipMemcpyAsync(pts_out, R.x, 3 * no * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(rad_out, rout, no * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (src_out) HIPCHK(hipMemcpyAsync(src_out, src, no * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // the kept arrays are freed below
    } else {
        HIPCHK(hipMemcpy(pts_out, R.x, 3 * no * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(rad_out, rout, no * sizeof(double), hipMemcpyDeviceToHost));
        if (src_out) HIPCHK(hipMemcpy(src_out, src, no * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    reseed_drop();
    return LSF_OK;
}
