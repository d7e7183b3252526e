// lsf_host_extract_surface.hpp -- host side of lsf_extract_surface (kernels and design: lsf_extract_surface.hpp; argument checks: lsf_host_args.hpp): the
// launches, the two totals the host reads, and the result kept for the calling thread until lsf_extract_get copies it out.
// Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// the mesh of the last extraction of this thread: device arrays, Fortran-ordered, owned here until a get or a new extraction
struct ExtractResult {
    bool have = false;
    int device = 0;
    int nn = 0, nt = 0;
    double* x = nullptr;   // (nn,3)
    int32_t* e = nullptr;  // (nt,3), 1-based
};
thread_local ExtractResult g_extract;

void extract_drop()
{
    ExtractResult& R = g_extract;
    if (R.x) (void)hipFree(R.x);
    if (R.e) (void)hipFree(R.e);
    R = ExtractResult{};
}

// arguments validated; d_phi is a device array.  Returns after the stream is synchronised.
int extract_core(const double* d_phi, int nx, int ny, int nz, double dx, const double xLo[3], double iso, int* nSurfNode, int* nSurfElem,
                 int64_t* info, hipStream_t st)
{
    int rc;
    Ctx& c = ctx();
    const long n = (long)(nx + 1) * (ny + 1) * (nz + 1);
    const long nTiles = (n + XS_TILE - 1) / XS_TILE;
    const int nbx = cdiv(nx + 1, XS_BX), nby = cdiv(ny + 1, XS_BY), nbz = cdiv(nz + 1, XS_KC);
    if ((double)nbx * nby * nbz > 2.0e9) return fail(LSF_ERR_INVALID, "lsf_extract_surface: too many blocks for one launch");
    if ((rc = ws(c.slot[S_XS_MASK], (size_t)n))) return rc;
    if ((rc = ws(c.slot[S_XS_BYTE], (size_t)n))) return rc;
    if ((rc = ws(c.slot[S_XS_NOFF], (size_t)n * sizeof(uint32_t)))) return rc;
    if ((rc = ws(c.slot[S_XS_TOFF], (size_t)n * sizeof(uint32_t)))) return rc;
    if ((rc = ws(c.slot[S_XS_SUMS], (size_t)nTiles * sizeof(uint2)))) return rc;
    if ((rc = ws(c.slot[S_XS_TILEOFF], (size_t)nTiles * sizeof(ulonglong2)))) return rc;
    if ((rc = ws(c.slot[S_XS_CTL], XS_CTL_LEN * sizeof(unsigned long long)))) return rc;
    unsigned char* mask = (unsigned char*)c.slot[S_XS_MASK].p;
    unsigned char* byte = (unsigned char*)c.slot[S_XS_BYTE].p;
    uint32_t* nodeOff = (uint32_t*)c.slot[S_XS_NOFF].p;
    uint32_t* triOff = (uint32_t*)c.slot[S_XS_TOFF].p;
    uint2* sums = (uint2*)c.slot[S_XS_SUMS].p;
    ulonglong2* tileOff = (ulonglong2*)c.slot[S_XS_TILEOFF].p;
    unsigned long long* ctl = (unsigned long long*)c.slot[S_XS_CTL].p;
    HIPCHK(hipMemsetAsync(ctl, 0, XS_CTL_LEN * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_extract_count, dim3((unsigned)((long)nbx * nby * nbz)), dim3(XS_BX, XS_BY), 0, st, d_phi, nx, ny, nz, iso, mask, byte, ctl,
                       nbx, nby);
    hipLaunchKernelGGL(k_extract_sums, dim3((unsigned)nTiles), dim3(XS_T), 0, st, (const unsigned char*)mask, (const unsigned char*)byte, n, sums);
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(XS_SCAN_T), 0, st, (const uint2*)sums, nTiles, tileOff, ctl);
    hipLaunchKernelGGL(k_extract_scatter, dim3((unsigned)nTiles), dim3(XS_T), 0, st, (const unsigned char*)mask, (const unsigned char*)byte, n,
                       (const ulonglong2*)tileOff, nodeOff, triOff);
    HIPCHK(hipGetLastError());
    unsigned long long h[XS_CTL_LEN];
    HIPCHK(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[XS_BAD])
        return fail(LSF_ERR_INVALID, "lsf_extract_surface: " + std::to_string(h[XS_BAD]) + " crossed edge(s) with a non-finite phi - iso on an endpoint");
    if (h[XS_NODES] > 2147483647ull) return fail(LSF_ERR_INVALID, "lsf_extract_surface: " + std::to_string(h[XS_NODES]) + " nodes, more than 2^31 - 1");
    if (h[XS_TRIS] > 2147483647ull) return fail(LSF_ERR_INVALID, "lsf_extract_surface: " + std::to_string(h[XS_TRIS]) + " triangles, more than 2^31 - 1");
    const long nn = (long)h[XS_NODES], nt = (long)h[XS_TRIS];
    ExtractResult& R = g_extract;
    if (nn > 0) { // (a crossed edge belongs to a crossed cell: nn > 0 means nt > 0)
        HIPCHK(hipMalloc((void**)&R.x, (size_t)nn * 3 * sizeof(double)));
        if (hipMalloc((void**)&R.e, (size_t)std::max(nt, 1L) * 3 * sizeof(int32_t)) != hipSuccess) {
            extract_drop();
            return fail(LSF_ERR_HIP, "lsf_extract_surface: out of device memory for the connectivity");
        }
        hipLaunchKernelGGL(k_extract_emit, dim3((unsigned)((n + XS_T - 1) / XS_T)), dim3(XS_T), 0, st, d_phi, nx, ny, nz, dx, xLo[0], xLo[1], xLo[2], iso,
                           (const unsigned char*)mask, (const unsigned char*)byte, (const uint32_t*)nodeOff, (const uint32_t*)triOff, R.x, nn, R.e, nt,
                           ctl);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            extract_drop();
            return fail(LSF_ERR_HIP, std::string("lsf_extract_surface: ") + hipGetErrorString(e));
        }
    }
    R.have = true, R.device = g_device, R.nn = (int)nn, R.nt = (int)nt;
    *nSurfNode = (int)nn, *nSurfElem = (int)nt;
    if (info) info[0] = nn, info[1] = nt, info[2] = (int64_t)h[XS_CELLS], info[3] = (int64_t)h[XS_T1];
    return LSF_OK;
}

// the kept result -> the caller's arrays (host: st unused; device: on st), then released
int extract_get(double* surfX, int32_t* surfElem, bool to_device, hipStream_t st)
{
    ExtractResult& R = g_extract;
    if (!R.have) return fail(LSF_ERR_INVALID, "lsf_extract_get without a kept lsf_extract_surface result");
    if (R.nn == 0) { // an empty mesh: nothing to write
        extract_drop();
        return LSF_OK;
    }
    if (!surfX || !surfElem) return fail(LSF_ERR_INVALID, "NULL pointer");
    int rc = ensure_device();
    if (rc) return rc;
    if (R.device != g_device) return fail(LSF_ERR_INVALID, "lsf_extract_get: the result was kept on another device (lsf_set_device)");
    const size_t bx = (size_t)R.nn * 3 * sizeof(double), be = (size_t)R.nt * 3 * sizeof(int32_t);
    if (to_device) {
        HIPCHK(hipMemcpyAsync(surfX, R.x, bx, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(surfElem, R.e, be, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // the kept arrays are freed below
    } else {
        HIPCHK(hipMemcpy(surfX, R.x, bx, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(surfElem, R.e, be, hipMemcpyDeviceToHost));
    }
    extract_drop();
    return LSF_OK;
}
