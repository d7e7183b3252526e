// lsf_mesh_distance.hpp -- exact (clamped) signed distance from a triangle mesh: lsf_mesh_distance.  No reference counterpart
// (the reference's inside/outside test, set3d.f90:196-268, is k_phi0).  Contract: include/lsf.h; account: DESIGN.md section 4.10.
//
// Two kernels, the field itself as the only grid-sized storage:
//   k_md_scatter   triangle-centric.  The field is filled with 0xFF bytes and read as 64-bit KEYS.  A triangle's work is the grid
//                  box of its bounding box padded by the tube width (any superset is correct: membership is `d <= far` alone); the
//                  host cuts every box into chunks of MD_CHUNK points (lsf_host_mesh.hpp), one block per chunk, so a box of any
//                  size is shared among blocks and no wave walks a large one.  Lanes run with i fastest: a wave's atomics fall on
//                  runs of contiguous keys.  A lane computes the exact point-to-triangle distance d (closest point over the face,
//                  edge and vertex regions), the sign bit `neg` from the dot product of the offset with the pseudonormal of the
//                  closest FEATURE, and combines
//                      key = (bits(d) << 1) | neg          (lossless: a non-negative double has a clear top bit)
//                  into the field with a 64-bit unsigned atomicMin.  The order of non-negative doubles is the order of their bits,
//                  so the minimum is the smaller distance and, at equal distance bits, the positive sign; an integer minimum does
//                  not depend on the order of arrival, hence the field is bit-identical from run to run.  A plain load of the
//                  current key skips the atomic when the key cannot win: a stale load can only be larger than the truth, so a
//                  skip is never wrong.
//   k_md_finalize  one lane per (i,j) column, coalesced over i, walking k upwards: a key becomes +-d in place and sets the carried
//                  sign, an untouched point (all bits set) becomes +-far with the carried sign.  Tube points are counted per lane,
//                  summed per wave and per block, one atomic add per block.
// The per-triangle record (30 doubles: vertices, unit face normal, three edge and three vertex pseudonormals) is wave-uniform and
// read once per work item.  Contraction is allowed here: there is no reference bit pattern to match.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsf {

constexpr int MD_CHUNK = 2048;  // points of a box one block works through
constexpr int MD_BLOCK = 256;
constexpr int MD_REC = 30;      // doubles per triangle: a b c | unit normal | edge ab bc ca | vertex a b c
constexpr int MD_BOX = 8;       // ints per triangle: ilo jlo klo | bx by bz (points per axis) | 2 spare

struct MdChunk {
    int32_t tri;    // row of the record / box tables
    int32_t pad_;
    int64_t start;  // first point of the chunk in the box, i fastest
};

__device__ __forceinline__ double md_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Closest point of triangle (a, b, c) to p by the Voronoi regions of its features (Ericson, Real-Time Collision Detection, 5.1.5).
// Returns the distance and, through *s, the dot product of the offset with the pseudonormal of the closest feature (rec + 9:
// normal, edges ab bc ca, vertices a b c).  In the face region the distance is taken along the unit normal.
__device__ __forceinline__ double md_point_triangle(const double* __restrict__ rec, const double p[3], double* s)
{
    const double* a = rec;
    const double* b = rec + 3;
    const double* c = rec + 6;
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        ab[m] = b[m] - a[m], ac[m] = c[m] - a[m];
        ap[m] = p[m] - a[m], bp[m] = p[m] - b[m], cp[m] = p[m] - c[m];
    }
    const double d1 = md_dot(ab, ap), d2 = md_dot(ac, ap);
    const double d3 = md_dot(ab, bp), d4 = md_dot(ac, bp);
    const double d5 = md_dot(ab, cp), d6 = md_dot(ac, cp);
    const double* pn;
    double off[3];
    if (d1 <= 0.0 && d2 <= 0.0) { // vertex a
        pn = rec + 21;
        off[0] = ap[0], off[1] = ap[1], off[2] = ap[2];
    } else if (d3 >= 0.0 && d4 <= d3) { // vertex b
        pn = rec + 24;
        off[0] = bp[0], off[1] = bp[1], off[2] = bp[2];
    } else if (d6 >= 0.0 && d5 <= d6) { // vertex c
        pn = rec + 27;
        off[0] = cp[0], off[1] = cp[1], off[2] = cp[2];
    } else {
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { // edge ab
            const double t = d1 / (d1 - d3);
            pn = rec + 12;
#pragma unroll
            for (int m = 0; m < 3; ++m) off[m] = ap[m] - t * ab[m];
        } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { // edge ca
            const double t = d2 / (d2 - d6);
            pn = rec + 18;
#pragma unroll
            for (int m = 0; m < 3; ++m) off[m] = ap[m] - t * ac[m];
        } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) { // edge bc
            const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
            pn = rec + 15;
#pragma unroll
            for (int m = 0; m < 3; ++m) off[m] = bp[m] - t * (c[m] - b[m]);
        } else { // face: the offset is the normal component of ap
            const double h = md_dot(ap, rec + 9);
            *s = h;
            return fabs(h);
        }
    }
    *s = md_dot(off, pn);
    return sqrt(md_dot(off, off));
}

// One block per chunk.  keys: the field, (nx+1)(ny+1)(nz+1) 64-bit words preset to all ones.  The boxes are clamped to the grid by
// the host, so every point of a box is a point of the field.
__global__ __launch_bounds__(MD_BLOCK) void k_md_scatter(unsigned long long* __restrict__ keys, int nx, int ny, double dx, double x0, double y0,
                                                         double z0, double far, int with_sign, const double* __restrict__ recs,
                                                         const int* __restrict__ boxes, const MdChunk* __restrict__ chunks)
{
    const MdChunk ch = chunks[blockIdx.x];
    const double* rec = recs + (size_t)ch.tri * MD_REC;
    const int* box = boxes + (size_t)ch.tri * MD_BOX;
    const int ilo = box[0], jlo = box[1], klo = box[2];
    const unsigned bx = (unsigned)box[3], by = (unsigned)box[4];
    const long long npts = (long long)bx * by * (unsigned)box[5];
    const size_t sx = (size_t)(nx + 1), sy = (size_t)(ny + 1);
    // a point farther than far from the triangle's PLANE is farther than that from the triangle; the margin keeps the shortcut
    // clear of the rounding of the two expressions, membership itself stays `d <= far`
    const double plane_cut = far * (1.0 + 1.0e-6);
#pragma unroll 1
    for (int r = 0; r < MD_CHUNK / MD_BLOCK; ++r) {
        const long long q = ch.start + (long long)r * MD_BLOCK + threadIdx.x;
        if (q >= npts) break;
        const unsigned long long row = (unsigned long long)q / bx;
        const int i = ilo + (int)((unsigned long long)q - row * bx);
        const unsigned long long pl = row / by;
        const int j = jlo + (int)(row - pl * by), k = klo + (int)pl;
        const double p[3] = {x0 + i * dx, y0 + j * dx, z0 + k * dx};
        const double hp = (p[0] - rec[0]) * rec[9] + (p[1] - rec[1]) * rec[10] + (p[2] - rec[2]) * rec[11];
        if (fabs(hp) > plane_cut) continue;
        double s;
        const double d = md_point_triangle(rec, p, &s);
        if (!(d <= far)) continue;
        const unsigned long long key = ((unsigned long long)__double_as_longlong(d) << 1) | (unsigned long long)(with_sign && s < 0.0);
        unsigned long long* dst = keys + ((size_t)i + sx * ((size_t)j + sy * (size_t)k));
        if (key < *dst) atomicMin(dst, key);
    }
}

// One lane per column (i, j).  ext: the sign in front of the first tube point (+1 / -1).  count: tube points of the whole field.
__global__ __launch_bounds__(MD_BLOCK) void k_md_finalize(double* phi, int nx, int ny, int nz, double far, double ext,
                                                          unsigned long long* __restrict__ count)
{
    __shared__ unsigned red[MD_BLOCK / 64];
    const size_t sx = (size_t)(nx + 1), ncol = sx * (size_t)(ny + 1);
    const size_t col = (size_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    unsigned cnt = 0;
    if (col < ncol) {
        unsigned long long* key = reinterpret_cast<unsigned long long*>(phi) + col;
        double sgn = ext;
        constexpr int U = 8; // keys in flight per lane: the walk depends on the carried sign, the loads do not
        for (int k0 = 0; k0 <= nz; k0 += U) {
            unsigned long long u[U];
#pragma unroll
            for (int m = 0; m < U; ++m) u[m] = k0 + m <= nz ? key[(size_t)(k0 + m) * ncol] : ~0ull;
#pragma unroll
            for (int m = 0; m < U; ++m) {
                if (k0 + m > nz) break;
                double v;
                if (u[m] == ~0ull) {
                    v = sgn * far;
                } else {
                    const double d = __longlong_as_double((long long)(u[m] >> 1));
                    sgn = (u[m] & 1ull) ? -1.0 : 1.0;
                    v = sgn * d;
                    ++cnt;
                }
                phi[col + (size_t)(k0 + m) * ncol] = v;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < MD_BLOCK / 64; ++w) t += red[w];
        if (t) atomicAdd(count, t);
    }
}

} // namespace lsf
