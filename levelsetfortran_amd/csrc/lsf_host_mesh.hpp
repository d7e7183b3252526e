// lsf_host_mesh.hpp -- host side of lsf_mesh_check / lsf_mesh_distance (kernels and design: lsf_mesh_distance.hpp): validation, the
// mesh preparation (degenerate triangles, edge and vertex pseudonormals, defective edges, signed volume), the chunk table and the
// launches.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

struct MeshPrep {
    std::vector<double> rec;   // MD_REC doubles per NON-DEGENERATE triangle, in triangle order
    int64_t ndegenerate = 0, ndefective = 0;
    double volume = 0.0;       // sum(v0 . (v1 x v2)) / 6 over all triangles
};

// Everything that depends on the mesh alone.  with_normals = false (LSF_MESH_UNSIGNED) leaves the pseudonormals zero.
int mesh_prepare(const double* surfX, int nSurfNode, const int32_t* surfElem, int nSurfElem, bool with_normals, MeshPrep& M)
{
    if (!surfX || !surfElem) return fail(LSF_ERR_INVALID, "NULL pointer");
    if (nSurfNode < 1 || nSurfElem < 1) return fail(LSF_ERR_INVALID, "empty surface (nSurfNode and nSurfElem must be >= 1)");
    const size_t nN = (size_t)nSurfNode, nE = (size_t)nSurfElem;
    for (size_t m = 0; m < 3 * nE; ++m)
        if (surfElem[m] < 1 || surfElem[m] > nSurfNode) return fail(LSF_ERR_INVALID, "surfElem index outside 1..nSurfNode");
    for (size_t m = 0; m < 3 * nN; ++m)
        if (!std::isfinite(surfX[m])) return fail(LSF_ERR_INVALID, "surfX holds a non-finite coordinate");
    auto node = [&](int id, double* v) {
        for (int c = 0; c < 3; ++c) v[c] = surfX[(size_t)(id - 1) + nN * c];
    };
    auto cross = [](const double* u, const double* v, double* w) {
        w[0] = u[1] * v[2] - u[2] * v[1], w[1] = u[2] * v[0] - u[0] * v[2], w[2] = u[0] * v[1] - u[1] * v[0];
    };
    struct Edge {
        int lo, hi, tri, e; // nodes (lo < hi), triangle, local edge (0 ab, 1 bc, 2 ca)
        bool fwd;           // traversed lo -> hi
    };
    std::vector<Edge> edges;
    std::vector<long> row(nE, -1); // triangle -> its record, -1: degenerate
    std::vector<double> vsum(with_normals ? 3 * nN : 0, 0.0);
    M = MeshPrep{};
    double vol = 0.0;
    for (size_t t = 0; t < nE; ++t) {
        int id[3];
        double v[3][3], e1[3], e2[3], n[3];
        for (int c = 0; c < 3; ++c) id[c] = surfElem[t + nE * c], node(id[c], v[c]);
        cross(v[1], v[2], n);
        vol += v[0][0] * n[0] + v[0][1] * n[1] + v[0][2] * n[2];
        for (int c = 0; c < 3; ++c) e1[c] = v[1][c] - v[0][c], e2[c] = v[2][c] - v[0][c];
        cross(e1, e2, n);
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(len > 0.0) || !std::isfinite(len)) { // zero-length normal: skipped, part of no pseudonormal and of no edge
            ++M.ndegenerate;
            continue;
        }
        row[t] = (long)(M.rec.size() / MD_REC);
        M.rec.resize(M.rec.size() + MD_REC, 0.0);
        double* r = &M.rec[(size_t)row[t] * MD_REC];
        for (int c = 0; c < 3; ++c) r[c] = v[0][c], r[3 + c] = v[1][c], r[6 + c] = v[2][c], r[9 + c] = n[c] / len;
        for (int e = 0; e < 3; ++e) {
            const int a = id[e], b = id[(e + 1) % 3];
            edges.push_back({std::min(a, b), std::max(a, b), (int)t, e, a < b});
        }
        if (with_normals) // angle-weighted vertex sums, in triangle order
            for (int k = 0; k < 3; ++k) {
                const double *p = v[k], *q = v[(k + 1) % 3], *s = v[(k + 2) % 3];
                double u[3], w[3], x[3];
                for (int c = 0; c < 3; ++c) u[c] = q[c] - p[c], w[c] = s[c] - p[c];
                cross(u, w, x);
                const double ang = std::atan2(std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), u[0] * w[0] + u[1] * w[1] + u[2] * w[2]);
                for (int c = 0; c < 3; ++c) vsum[(size_t)(id[k] - 1) * 3 + c] += ang * r[9 + c];
            }
    }
    M.volume = vol / 6.0;
    // edges: one not shared by exactly two non-degenerate triangles that traverse it in opposite directions is defective; a sound
    // one gets the sum of its two unit face normals, the lower triangle first, copied to both triangles (the same bits)
    std::sort(edges.begin(), edges.end(), [](const Edge& x, const Edge& y) { return std::tie(x.lo, x.hi, x.tri, x.e) < std::tie(y.lo, y.hi, y.tri, y.e); });
    for (size_t b = 0; b < edges.size();) {
        size_t e = b + 1;
        while (e < edges.size() && edges[e].lo == edges[b].lo && edges[e].hi == edges[b].hi) ++e;
        if (e - b != 2 || edges[b].fwd == edges[b + 1].fwd) {
            ++M.ndefective;
        } else if (with_normals) {
            double* r0 = &M.rec[(size_t)row[edges[b].tri] * MD_REC];
            double* r1 = &M.rec[(size_t)row[edges[b + 1].tri] * MD_REC];
            for (int c = 0; c < 3; ++c) r0[12 + 3 * edges[b].e + c] = r1[12 + 3 * edges[b + 1].e + c] = r0[9 + c] + r1[9 + c];
        }
        b = e;
    }
    if (with_normals)
        for (size_t t = 0; t < nE; ++t)
            if (row[t] >= 0)
                for (int k = 0; k < 3; ++k)
                    for (int c = 0; c < 3; ++c)
                        M.rec[(size_t)row[t] * MD_REC + 21 + 3 * k + c] = vsum[(size_t)(surfElem[t + nE * k] - 1) * 3 + c];
    return LSF_OK;
}

// validation and mesh preparation of one call; nothing is written anywhere before this has passed
int mesh_distance_prepare(int nx, int ny, int nz, double dx, const double* xLo, const double* surfX, int nSurfNode, const int32_t* surfElem,
                          int nSurfElem, double width, int flags, MeshPrep& M)
{
    int rc = mesh_args_ok(nx, ny, nz, dx, xLo, width, flags);
    if (rc) return rc;
    const bool with_sign = !(flags & LSF_MESH_UNSIGNED);
    if ((rc = mesh_prepare(surfX, nSurfNode, surfElem, nSurfElem, with_sign, M))) return rc;
    if (with_sign && M.ndefective)
        return fail(LSF_ERR_INVALID, "lsf_mesh_distance: the mesh has " + std::to_string(M.ndefective) +
                                         " defective edge(s) (not shared by exactly two triangles of opposite direction): no inside and "
                                         "outside; pass LSF_MESH_UNSIGNED for the unsigned distance");
    return LSF_OK;
}

int mesh_distance_run(double* d_phi, int nx, int ny, int nz, double dx, const double* xLo, double width, int flags, const MeshPrep& M,
                      int64_t* info, hipStream_t st)
{
    int rc;
    const bool with_sign = !(flags & LSF_MESH_UNSIGNED);
    const double far = width * dx;
    // boxes and chunks: bounding box padded by the width, plus one cell against the rounding of the division, clamped to the grid
    const size_t ntri = M.rec.size() / MD_REC;
    const int nmax[3] = {nx, ny, nz};
    const double pad = std::ceil(width) + 1.0;
    std::vector<double> rec;
    std::vector<int> box;
    std::vector<MdChunk> chunks;
    int64_t nmiss = 0;
    for (size_t t = 0; t < ntri; ++t) {
        const double* r = &M.rec[t * MD_REC];
        int lo[3], n[3];
        bool miss = false;
        for (int c = 0; c < 3; ++c) {
            const double mn = std::min(r[c], std::min(r[3 + c], r[6 + c])), mx = std::max(r[c], std::max(r[3 + c], r[6 + c]));
            const double a = std::floor((mn - xLo[c]) / dx) - pad, b = std::ceil((mx - xLo[c]) / dx) + pad;
            if (!(b >= 0.0) || !(a <= (double)nmax[c])) { // (a NaN from an overflowing difference misses too)
                miss = true;
                break;
            }
            lo[c] = (int)std::max(a, 0.0);
            n[c] = (int)std::min(b, (double)nmax[c]) - lo[c] + 1;
        }
        if (miss) {
            ++nmiss;
            continue;
        }
        const int32_t slot = (int32_t)(box.size() / MD_BOX);
        rec.insert(rec.end(), r, r + MD_REC);
        const int bx[MD_BOX] = {lo[0], lo[1], lo[2], n[0], n[1], n[2], 0, 0};
        box.insert(box.end(), bx, bx + MD_BOX);
        const int64_t npts = (int64_t)n[0] * n[1] * n[2];
        for (int64_t s = 0; s < npts; s += MD_CHUNK) chunks.push_back({slot, 0, s});
    }
    if (chunks.size() > (size_t)0x7fffffff) return fail(LSF_ERR_INVALID, "lsf_mesh_distance: more than 2^31 - 1 chunks of work (narrow the tube)");
    Ctx& c = ctx();
    const size_t n = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
    if ((rc = ws(c.slot[S_MD_CNT], 64))) return rc;
    unsigned long long* d_cnt = (unsigned long long*)c.slot[S_MD_CNT].p;
    HIPCHK(hipMemsetAsync(d_cnt, 0, 8, st));
    HIPCHK(hipMemsetAsync(d_phi, 0xFF, n * sizeof(double), st));
    if (!chunks.empty()) {
        if ((rc = ws(c.slot[S_MD_REC], rec.size() * sizeof(double)))) return rc;
        if ((rc = ws(c.slot[S_MD_BOX], box.size() * sizeof(int)))) return rc;
        if ((rc = ws(c.slot[S_MD_CHUNK], chunks.size() * sizeof(MdChunk)))) return rc;
        HIPCHK(hipMemcpyAsync(c.slot[S_MD_REC].p, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c.slot[S_MD_BOX].p, box.data(), box.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c.slot[S_MD_CHUNK].p, chunks.data(), chunks.size() * sizeof(MdChunk), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_md_scatter, dim3((unsigned)chunks.size()), dim3(MD_BLOCK), 0, st, (unsigned long long*)d_phi, nx, ny, dx, xLo[0], xLo[1],
                           xLo[2], far, with_sign ? 1 : 0, (const double*)c.slot[S_MD_REC].p, (const int*)c.slot[S_MD_BOX].p,
                           (const MdChunk*)c.slot[S_MD_CHUNK].p);
    }
    const double ext = (with_sign && M.volume < 0.0) ? -1.0 : 1.0; // the sign in front of a column's first tube point
    const size_t ncol = (size_t)(nx + 1) * (ny + 1);
    hipLaunchKernelGGL(k_md_finalize, dim3((unsigned)((ncol + MD_BLOCK - 1) / MD_BLOCK)), dim3(MD_BLOCK), 0, st, d_phi, nx, ny, nz, far, ext, d_cnt);
    HIPCHK(hipGetLastError());
    unsigned long long cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the tables are host temporaries
    if (getenv("LSF_TRACE"))
        fprintf(stderr, "[lsf] mesh distance: %zu triangles in %zu chunks, %llu tube points (%.2f %% of the grid)\n", box.size() / MD_BOX, chunks.size(),
                cnt, 100.0 * (double)cnt / (double)n);
    if (info) info[0] = (int64_t)cnt, info[1] = M.ndegenerate, info[2] = M.ndefective, info[3] = nmiss;
    return LSF_OK;
}
