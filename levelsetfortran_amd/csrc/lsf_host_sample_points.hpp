// lsf_host_sample_points.hpp -- host side of lsf_sample_points (kernel and design: lsf_sample_points.hpp): validation, the one launch
// over the points and the finish of its per-block counts in block order.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// what can be decided without the device (the arrays are the caller's, host or device: only compared; xLo is a host array on both
// seams); nothing is written anywhere before this has passed
int sample_points_args_ok(const void* phi, const void* mask, const void* q, int nx, int ny, int nz, double dx, const double* xLo, const void* pts,
                          int npts, int order, double iso, int iters, double tol, const void* val, const void* grad, const void* qval,
                          const void* foot, const void* status)
{
    if (!phi) return fail(LSF_ERR_INVALID, "lsf_sample_points: phi is NULL");
    if (!pts) return fail(LSF_ERR_INVALID, "lsf_sample_points: pts is NULL");
    if (!val) return fail(LSF_ERR_INVALID, "lsf_sample_points: val is NULL");
    if (!xLo) return fail(LSF_ERR_INVALID, "lsf_sample_points: xLo is NULL");
    if (npts < 1) return fail(LSF_ERR_INVALID, "lsf_sample_points: npts must be >= 1");
    if (nx < 1 || ny < 1 || nz < 1) return fail(LSF_ERR_INVALID, "lsf_sample_points: nx, ny, nz must be >= 1");
    if ((double)((size_t)nx + 1) * (double)((size_t)ny + 1) * (double)((size_t)nz + 1) > 2147483647.0)
        return fail(LSF_ERR_INVALID, "lsf_sample_points: more than 2^31 - 1 points");
    const size_t n = ((size_t)nx + 1) * ((size_t)ny + 1) * ((size_t)nz + 1), np = (size_t)npts;
    if (!(dx > 0.0) || !std::isfinite(dx)) return fail(LSF_ERR_INVALID, "lsf_sample_points: dx must be finite and > 0");
    if (!std::isfinite(xLo[0]) || !std::isfinite(xLo[1]) || !std::isfinite(xLo[2]))
        return fail(LSF_ERR_INVALID, "lsf_sample_points: xLo must hold three finite values");
    if (!std::isfinite(iso)) return fail(LSF_ERR_INVALID, "lsf_sample_points: iso must be finite");
    if (order != LSF_SAMPLE_LINEAR && order != LSF_SAMPLE_CUBIC) return fail(LSF_ERR_INVALID, "lsf_sample_points: unknown order");
    if (iters < 0) return fail(LSF_ERR_INVALID, "lsf_sample_points: iters must be >= 0");
    if (iters >= 1 && (!(tol >= 0.0) || !std::isfinite(tol))) return fail(LSF_ERR_INVALID, "lsf_sample_points: tol must be finite and >= 0");
    if (qval && !q) return fail(LSF_ERR_INVALID, "lsf_sample_points: qval without q");
    if (foot && iters == 0) return fail(LSF_ERR_INVALID, "lsf_sample_points: foot with iters == 0");
    // an output is written while the inputs and the other outputs are still being read or written: it may share a byte with none of
    // them.  The overlap test of curvature_band_args_ok, each array with its own size.
    const void* a[9] = {phi, mask, q, pts, val, grad, qval, foot, status};
    const size_t bytes[9] = {n * sizeof(double),      n * sizeof(int32_t), n * sizeof(double),      3 * np * sizeof(double), np * sizeof(double),
                             3 * np * sizeof(double), np * sizeof(double), 3 * np * sizeof(double), np * sizeof(int32_t)};
    const char* name[9] = {"phi", "mask", "q", "pts", "val", "grad", "qval", "foot", "status"};
    for (int i = 4; i < 9; ++i) // the outputs
        for (int j = 0; j < i; ++j) {
            if (!a[i] || !a[j]) continue;
            const uintptr_t x = (uintptr_t)a[i], y = (uintptr_t)a[j];
            if (x < y ? y - x < bytes[i] : x - y < bytes[j])
                return fail(LSF_ERR_INVALID, std::string("lsf_sample_points: ") + name[i] + " overlaps " + name[j]);
        }
    return LSF_OK;
}

// the arguments have passed sample_points_args_ok and every array is device memory.  info is written on LSF_OK only.  Returns after
// the stream is synchronised.
int sample_points_core(const double* d_phi, const int32_t* d_mask, const double* d_q, int nx, int ny, int nz, double dx, const double xLo[3],
                       const double* d_pts, int npts, int order, double iso, int iters, double tol, double* d_val, double* d_grad, double* d_qval,
                       double* d_foot, int32_t* d_status, int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const int nblocks = (int)(((size_t)npts + SP_BLOCK - 1) / SP_BLOCK);
    if ((rc = ws(c.slot[S_PART], (size_t)nblocks * SP_NPART * sizeof(unsigned long long)))) return rc;
    unsigned long long* part = (unsigned long long*)c.slot[S_PART].p;
    const SpGrid G{d_phi, d_mask, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2]};
    const double tol_dx = tol * dx;
    const dim3 grid((unsigned)nblocks), blk(SP_BLOCK);
#define LSF_SP_CALL(CU, HQ, HM, PR) \
    hipLaunchKernelGGL((k_sample_points<CU, HQ, HM, PR>), grid, blk, 0, st, G, d_q, d_pts, npts, iso, iters, tol_dx, d_val, d_grad, d_qval, d_foot, \
                       d_status, part)
    switch ((order == LSF_SAMPLE_CUBIC ? 8 : 0) | (d_q ? 4 : 0) | (d_mask ? 2 : 0) | (iters >= 1 ? 1 : 0)) {
    case 0: LSF_SP_CALL(false, false, false, false); break;
    case 1: LSF_SP_CALL(false, false, false, true); break;
    case 2: LSF_SP_CALL(false, false, true, false); break;
    case 3: LSF_SP_CALL(false, false, true, true); break;
    case 4: LSF_SP_CALL(false, true, false, false); break;
    case 5: LSF_SP_CALL(false, true, false, true); break;
    case 6: LSF_SP_CALL(false, true, true, false); break;
    case 7: LSF_SP_CALL(false, true, true, true); break;
    case 8: LSF_SP_CALL(true, false, false, false); break;
    case 9: LSF_SP_CALL(true, false, false, true); break;
    case 10: LSF_SP_CALL(true, false, true, false); break;
    case 11: LSF_SP_CALL(true, false, true, true); break;
    case 12: LSF_SP_CALL(true, true, false, false); break;
    case 13: LSF_SP_CALL(true, true, false, true); break;
    case 14: LSF_SP_CALL(true, true, true, false); break;
    default: LSF_SP_CALL(true, true, true, true); break;
    }
#undef LSF_SP_CALL
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> h((size_t)nblocks * SP_NPART);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long tot[SP_NPART] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nblocks; ++b) // block order; integer counts: no order in the result
        for (int m = 0; m < SP_NPART; ++m) tot[m] += h[(size_t)b * SP_NPART + m];
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] samples: %d points, %d blocks, %llu ok, %llu outside, %llu off the band, %llu linear fallbacks, %llu flat, %llu not converged\n",
                npts, nblocks, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5]);
    if (info)
        for (int m = 0; m < SP_NPART; ++m) info[m] = (int64_t)tot[m];
    return LSF_OK;
}
