// mesh_sdf.hip -- signed distance of query points / of a voxel grid to a triangle mesh (include/pn2_sdf.h:
// pn2s_mesh_sdf_points, pn2s_mesh_sdf_volume): the producer of the volumes the particle optimisers look up.  Reference:
// load_obj_oracle (optimization_obj.py:163-182, commented out there because it needs kaolin's point_to_mesh_distance and
// check_sign): "directly compute the SDF volume from a mesh if we assume the mesh is known", clamped to +-0.1.
//
// Definition.  |d|(p) = the exact minimum over all triangles of the distance from p to the triangle's closest point (face, edge
// or vertex); sign from the generalised winding number w(p) = (1/4pi) sum_f Omega_f(p), Omega_f = 2 atan2(a.(b x c),
// |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) with a, b, c = v - p (Van Oosterom-Strackee); inside (negative) iff w > 0.5.
// The face region is decided by three edge functions against the unit normal, n . ((end - start) x (p - start)) = |edge| times
// the distance of p's projection inside that edge's line, each held to a margin of 2^-20 |edge| |p - start|: the rounding of
// the expression stays below it, so a projection accepted as inside is inside, and one rejected within the margin lies within
// 2^-20 |p - start| of an edge, where the edge's distance exceeds the plane's by at most that (second order off the plane).
// The unit normal is built in fp64 by the prepare launch: the fp32 cross product of a sliver's edges keeps eps / sin(angle) of
// its direction, which tilts the plane by millimetres at sin = 1e-5.  Triangles down to the degeneracy threshold are exact to
// the same bound as well-shaped ones.
// A torch composition builds (points x faces) temporaries for every term; here a triangle is a 80-byte record prepared once,
// a workgroup stages the records through LDS and each thread keeps its query, its running minimum and its running sum of
// angles in registers.  No triangle is skipped; no atomics: a thread sums its angles in face order, so two runs are bitwise
// equal.
#include <hip/hip_fp16.h>

#include "pn2_common.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {

constexpr int kMsThreads = 256;
constexpr int kMsChunk = 512;      // triangles staged in LDS at a time: 40 KB of records -> 4 workgroups per CU
constexpr int kMsRec = 5;          // float4 per triangle record
constexpr int kMsHeader = 4;       // floats in front of the records: [0] = bad-face-index flag (int), 16-byte alignment
constexpr int kMsMaxFaces = 1 << 24, kMsMaxVerts = 1 << 24, kMsMaxRes = 1023;
// sin^2 of the angle at vertex a (in fp64, from the fp32 vertices) at or below which a triangle counts as degenerate (collinear
// or repeated vertices): a sliver this thin is its longest edge to fp32
constexpr double kMsDegenerate = 1e-12;
constexpr double kMsFaceMargin = 0x1p-20;  // 16 half-ulps: above the rounding of an edge function, see the header

__device__ __forceinline__ float ms_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

// Record of triangle f, 5 float4:
//   (a, 1/|b-a|^2) (b, 1/|c-b|^2) (c, 1/|a-c|^2)      the reciprocal is 0 for an edge of zero length
//   (n / |n|, 1)    n = (b-a) x (c-a) in fp64           (0, 0, 0, 0) marks a degenerate triangle: no face region, no solid angle
//   (|b-a|, |c-b|, |a-c|, 0) * kMsFaceMargin            the margins of the three edge functions
// A face index outside [0, nv) sets the flag and the triangle is built from vertex 0 (nothing is read out of bounds).
__global__ void __launch_bounds__(kMsThreads)
mesh_sdf_prepare_kernel(int nv, const float *__restrict__ verts, int nf, const int *__restrict__ faces, float *__restrict__ work) {
    const int f = blockIdx.x * kMsThreads + threadIdx.x;
    if (f >= nf) return;
    int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) {
        reinterpret_cast<int *>(work)[0] = 1;  // every writer stores the same value
        ia = ib = ic = 0;
    }
    const float ax = verts[3 * (size_t)ia], ay = verts[3 * (size_t)ia + 1], az = verts[3 * (size_t)ia + 2];
    const float bx = verts[3 * (size_t)ib], by = verts[3 * (size_t)ib + 1], bz = verts[3 * (size_t)ib + 2];
    const float cx = verts[3 * (size_t)ic], cy = verts[3 * (size_t)ic + 1], cz = verts[3 * (size_t)ic + 2];
    const float e0x = bx - ax, e0y = by - ay, e0z = bz - az;
    const float e1x = cx - ax, e1y = cy - ay, e1z = cz - az;
    const float e2x = cx - bx, e2y = cy - by, e2z = cz - bz;
    const float d00 = ms_dot(e0x, e0y, e0z, e0x, e0y, e0z), d11 = ms_dot(e1x, e1y, e1z, e1x, e1y, e1z),
                d22 = ms_dot(e2x, e2y, e2z, e2x, e2y, e2z);
    // the face's side in fp64: differences of fp32 values are exact there, the cross product is good to 1e-16 / sin(angle)
    const double f0x = (double)bx - ax, f0y = (double)by - ay, f0z = (double)bz - az;
    const double f1x = (double)cx - ax, f1y = (double)cy - ay, f1z = (double)cz - az;
    const double f2x = (double)cx - bx, f2y = (double)cy - by, f2z = (double)cz - bz;
    const double nx = f0y * f1z - f0z * f1y, ny = f0z * f1x - f0x * f1z, nz = f0x * f1y - f0y * f1x;
    const double nn = nx * nx + ny * ny + nz * nz, l0 = f0x * f0x + f0y * f0y + f0z * f0z, l1 = f1x * f1x + f1y * f1y + f1z * f1z,
                 l2 = f2x * f2x + f2y * f2y + f2z * f2z;
    const bool degenerate = !(nn > kMsDegenerate * l0 * l1);
    const double inv_n = degenerate ? 0.0 : 1.0 / sqrt(nn);
    float4 *rec = reinterpret_cast<float4 *>(work + kMsHeader) + (size_t)f * kMsRec;
    rec[0] = make_float4(ax, ay, az, d00 > 0.f ? 1.f / d00 : 0.f);
    rec[1] = make_float4(bx, by, bz, d22 > 0.f ? 1.f / d22 : 0.f);
    rec[2] = make_float4(cx, cy, cz, d11 > 0.f ? 1.f / d11 : 0.f);
    rec[3] = make_float4((float)(nx * inv_n), (float)(ny * inv_n), (float)(nz * inv_n), degenerate ? 0.f : 1.f);
    rec[4] = make_float4((float)(sqrt(l0) * kMsFaceMargin), (float)(sqrt(l2) * kMsFaceMargin), (float)(sqrt(l1) * kMsFaceMargin), 0.f);
}

// n . ((e - s) x q), q = query - s: |e - s| times the distance of the query's projection inside the line s -> e of a triangle
// with unit normal n (counter-clockwise seen from n)
__device__ __forceinline__ float ms_edge_fn(float qx, float qy, float qz, float sx, float sy, float sz, float ex, float ey, float ez,
                                            float nx, float ny, float nz) {
    const float dx = ex - sx, dy = ey - sy, dz = ez - sz;
    return ms_dot(nx, ny, nz, dy * qz - dz * qy, dz * qx - dx * qz, dx * qy - dy * qx);
}

// Squared distance from the query to the segment s -> e, given q = query - s: every edge of every triangle goes through this
// one function from its own start vertex, so an edge shared by two triangles (or repeated by a degenerate one) gives the
// same float wherever it appears and the minimum does not depend on the face order.
__device__ __forceinline__ float ms_segment(float qx, float qy, float qz, float sx, float sy, float sz, float ex, float ey, float ez,
                                            float inv_len2) {
    const float dx = ex - sx, dy = ey - sy, dz = ez - sz;
    float t = ms_dot(qx, qy, qz, dx, dy, dz) * inv_len2;
    t = __builtin_fminf(__builtin_fmaxf(t, 0.f), 1.f);
    const float rx = __builtin_fmaf(-t, dx, qx), ry = __builtin_fmaf(-t, dy, qy), rz = __builtin_fmaf(-t, dz, qz);
    return ms_dot(rx, ry, rz, rx, ry, rz);
}

// grid (ceil(m / 256)): thread i owns query i -- point i of `pts`, or (volume) voxel i = (ix*res + iy)*res + iz at
// ((ix, iy, iz) - res/2) * stride -- and walks all nf triangles, 512 at a time out of LDS.  A record's address is the same
// in every lane (LDS broadcast reads, no bank conflicts).  out_mode 0: out = signed distance fp32, unclamped; 1 / 2: clamped
// to [-clamp, clamp] and stored as fp32 / rounded once to fp16.  wn: the winding number per query, or NULL.
__global__ void __launch_bounds__(kMsThreads)
mesh_sdf_kernel(int m, const float *__restrict__ pts, int res, float stride, int nf, const float *__restrict__ work, float clamp,
                int out_mode, void *__restrict__ out, float *__restrict__ wn) {
    __shared__ float4 tri[kMsChunk * kMsRec];
    const int i = blockIdx.x * kMsThreads + (int)threadIdx.x;
    const int q = i < m ? i : m - 1;  // a thread past the end repeats the last query and stores nothing
    float px, py, pz;
    if (pts != nullptr) {
        px = pts[3 * (size_t)q];
        py = pts[3 * (size_t)q + 1];
        pz = pts[3 * (size_t)q + 2];
    } else {
        const int iz = q % res, iy = (q / res) % res, ix = q / (res * res), h = res / 2;
        px = (float)(ix - h) * stride;
        py = (float)(iy - h) * stride;
        pz = (float)(iz - h) * stride;
    }
    const float4 *__restrict__ rec = reinterpret_cast<const float4 *>(work + kMsHeader);
    float best = __builtin_inff(), angles = 0.f;
    for (int c0 = 0; c0 < nf; c0 += kMsChunk) {
        const int cnt = (nf - c0) < kMsChunk ? (nf - c0) : kMsChunk;
        __syncthreads();  // the previous chunk has been read
        for (int j = threadIdx.x; j < cnt * kMsRec; j += kMsThreads) tri[j] = rec[(size_t)c0 * kMsRec + j];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4 A = tri[j * kMsRec], B = tri[j * kMsRec + 1], C = tri[j * kMsRec + 2], N = tri[j * kMsRec + 3],
                         D = tri[j * kMsRec + 4];
            const float ax = px - A.x, ay = py - A.y, az = pz - A.z;  // query - vertex
            const float bx = px - B.x, by = py - B.y, bz = pz - B.z;
            const float cx = px - C.x, cy = py - C.y, cz = pz - C.z;
            // the three edges a->b, b->c, c->a
            float d2 = ms_segment(ax, ay, az, A.x, A.y, A.z, B.x, B.y, B.z, A.w);
            d2 = __builtin_fminf(d2, ms_segment(bx, by, bz, B.x, B.y, B.z, C.x, C.y, C.z, B.w));
            d2 = __builtin_fminf(d2, ms_segment(cx, cy, cz, C.x, C.y, C.z, A.x, A.y, A.z, C.w));
            const float la = __builtin_sqrtf(ms_dot(ax, ay, az, ax, ay, az)), lb = __builtin_sqrtf(ms_dot(bx, by, bz, bx, by, bz)),
                        lc = __builtin_sqrtf(ms_dot(cx, cy, cz, cx, cy, cz));
            // the face, where the projection falls inside all three edges' lines by more than the margin
            const bool inside = N.w != 0.f && ms_edge_fn(ax, ay, az, A.x, A.y, A.z, B.x, B.y, B.z, N.x, N.y, N.z) >= D.x * la &&
                                ms_edge_fn(bx, by, bz, B.x, B.y, B.z, C.x, C.y, C.z, N.x, N.y, N.z) >= D.y * lb &&
                                ms_edge_fn(cx, cy, cz, C.x, C.y, C.z, A.x, A.y, A.z, N.x, N.y, N.z) >= D.z * lc;
            const float nd = ms_dot(ax, ay, az, N.x, N.y, N.z);
            d2 = inside ? __builtin_fminf(d2, nd * nd) : d2;
            best = __builtin_fminf(best, d2);
            // Van Oosterom-Strackee with (query - vertex) vectors: the dot products are those of (vertex - query), the triple
            // product changes sign
            const float kx = by * cz - bz * cy, ky = bz * cx - bx * cz, kz = bx * cy - by * cx;
            const float num = -ms_dot(ax, ay, az, kx, ky, kz);
            const float den = __builtin_fmaf(ms_dot(cx, cy, cz, ax, ay, az), lb,
                                             __builtin_fmaf(ms_dot(bx, by, bz, cx, cy, cz), la,
                                                            __builtin_fmaf(ms_dot(ax, ay, az, bx, by, bz), lc, la * lb * lc)));
            // a degenerate triangle adds exactly zero, whatever rounding leaves in den (atan2f(0, den < 0) would be pi)
            angles += N.w != 0.f ? atan2f(num, den) : 0.f;
        }
    }
    if (i >= m) return;
    const float w = angles * 0.15915494309189535f;  // sum of Omega / 4 pi = sum of atan2 / 2 pi
    float d = __builtin_sqrtf(best);
    d = w > 0.5f ? -d : d;
    if (wn != nullptr) wn[i] = w;
    if (out_mode == 0) {
        reinterpret_cast<float *>(out)[i] = d;
    } else {
        d = __builtin_fminf(__builtin_fmaxf(d, -clamp), clamp);
        if (out_mode == 1) reinterpret_cast<float *>(out)[i] = d;
        else reinterpret_cast<__half *>(out)[i] = __float2half_rn(d);
    }
}

static int mesh_sdf_launch(int m, const float *pts, int res, float stride, int nv, const float *verts, int nf, const int *faces,
                           float clamp, int out_mode, void *out, float *wn, float *work, long work_floats, hipStream_t st) {
    if (nv > kMsMaxVerts || nf > kMsMaxFaces) return PN2_ERANGE;
    if (work_floats < kMsHeader + 4L * kMsRec * nf) return PN2_ESCRATCH;
    if (((uintptr_t)work & 15) != 0) return PN2_EINVAL;
    if (hipMemsetAsync(work, 0, kMsHeader * sizeof(float), st) != hipSuccess) return check_launch();
    hipLaunchKernelGGL(mesh_sdf_prepare_kernel, dim3((nf + kMsThreads - 1) / kMsThreads), dim3(kMsThreads), 0, st, nv, verts, nf, faces,
                       work);
    hipLaunchKernelGGL(mesh_sdf_kernel, dim3((m + kMsThreads - 1) / kMsThreads), dim3(kMsThreads), 0, st, m, pts, res, stride, nf,
                       (const float *)work, clamp, out_mode, out, wn);
    return check_launch();
}

}  // namespace pn2

extern "C" long pn2s_mesh_sdf_work_floats(int nf) {
    return nf < 0 ? (long)PN2_EINVAL : pn2::kMsHeader + 4L * pn2::kMsRec * nf;
}

extern "C" int pn2s_mesh_sdf_points(int m, const float *pts, int nv, const float *verts, int nf, const int *faces, float *out_sdf,
                                     float *out_wn, float *work, long work_floats, void *stream) {
    if (m < 0 || nv < 0 || nf < 0) return PN2_EINVAL;
    if (m == 0) return PN2_OK;
    if (nv == 0 || nf == 0) return PN2_EINVAL;
    if (!pts || !verts || !faces || !out_sdf || !work) return PN2_ENULL;
    return pn2::mesh_sdf_launch(m, pts, 1, 0.f, nv, verts, nf, faces, 0.f, 0, out_sdf, out_wn, work, work_floats, (hipStream_t)stream);
}

extern "C" int pn2s_mesh_sdf_volume(int nv, const float *verts, int nf, const int *faces, int res, float stride, float clamp, void *out,
                                     int out_f16, float *work, long work_floats, void *stream) {
    if (nv <= 0 || nf <= 0 || res <= 1 || res % 2 == 0 || !(stride > 0.f) || !(clamp > 0.f)) return PN2_EINVAL;
    if (!verts || !faces || !out || !work) return PN2_ENULL;
    if (res > pn2::kMsMaxRes) return PN2_ERANGE;
    return pn2::mesh_sdf_launch(res * res * res, nullptr, res, stride, nv, verts, nf, faces, clamp, out_f16 ? 2 : 1, out, nullptr, work,
                                work_floats, (hipStream_t)stream);
}
