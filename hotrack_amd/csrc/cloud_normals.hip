// cloud_normals.hip -- oriented surface normals of a point cloud (include/pn2_ext.h: pn2x_cloud_normals), the
// neighbourhood operator of the reference's observed-surface bookkeeping (optimization_obj.py:335-343: open3d's
// estimate_normals on the host, a device -> host -> device hop per frame).
//
// One WAVE owns a query, one launch covers the batch:
//   1. selection: knn_wave.h's register-resident keys ((fp32 squared distance bits << 32) | index, P per lane, sorted by
//      the compile-time network), masked points and points with a non-finite coordinate keyed out; kk = min(k, valid points)
//      rounds of "wave-min over the lane heads -> lowest lane holding it pops".  The popped index of round r stays in lane
//      r's register: the (B, N, k) list never exists in memory.
//   2. covariance: lane r < kk loads its neighbour; mean, then the six centred second moments, as wave sums on the DPP
//      ladder (wave_sum_f32: fixed order, no LDS).  Two passes, never E[x^2] - E[x]^2.
//   3. eigenvector: kJacobiSweeps cyclic Jacobi sweeps in fp32 on the covariance divided by its trace, every lane the
//      same arithmetic on wave-uniform values (nothing to exchange); the column of the smallest diagonal entry.
//   4. orientation, and lane 0 writes the four floats.
// No LDS, no scratch memory, no atomics: two calls give the same bits.
#include "pn2_common.h"
#include "knn_wave.h"
#include "../../include/pn2_ext.h"

namespace pn2 {

constexpr int kJacobiSweeps = 5;  // 3x3 cyclic Jacobi converges quadratically: fp32 is reached in 3-4 sweeps

// One Jacobi rotation in the (p, q) plane of the symmetric matrix {app, aqq, apq, arp, arq} (r the third index), applied to
// the eigenvector columns (v?p, v?q) as well.  apq == 0 is the identity rotation.
#define PN2_JACOBI_ROTATE(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                       \
    {                                                                                                                  \
        const bool skip = apq == 0.f;                                                                                  \
        const float theta = (aqq - app) / (2.f * (skip ? 1.f : apq));                                                  \
        const float at = __builtin_fabsf(theta);                                                                       \
        float t = 1.f / (at + __builtin_sqrtf(theta * theta + 1.f)); /* theta^2 overflowing to inf gives t = 0 */      \
        t = theta < 0.f ? -t : t;                                                                                      \
        t = skip ? 0.f : t;                                                                                            \
        const float c = 1.f / __builtin_sqrtf(t * t + 1.f), s = t * c;                                                 \
        const float h = t * apq;                                                                                       \
        app = app - h;                                                                                                 \
        aqq = aqq + h;                                                                                                 \
        apq = 0.f;                                                                                                     \
        const float rp = arp, rq = arq;                                                                                \
        arp = c * rp - s * rq;                                                                                         \
        arq = s * rp + c * rq;                                                                                         \
        const float e0 = v0p, f0 = v0q, e1 = v1p, f1 = v1q, e2 = v2p, f2 = v2q;                                        \
        v0p = c * e0 - s * f0;                                                                                         \
        v0q = s * e0 + c * f0;                                                                                         \
        v1p = c * e1 - s * f1;                                                                                         \
        v1q = s * e1 + c * f1;                                                                                         \
        v2p = c * e2 - s * f2;                                                                                         \
        v2q = s * e2 + c * f2;                                                                                         \
    }

template <int P>
__global__ void __launch_bounds__(256)
cloud_normals_kernel(int n, int k, int orient, const float *__restrict__ points_all, const unsigned char *__restrict__ valid_all,
                     const float *__restrict__ viewpoint_all, float *__restrict__ normals_all, float *__restrict__ variation_all) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n) return;  // wave-uniform; the kernel has no workgroup barrier
    const int lane = threadIdx.x & 63;
    const float *__restrict__ pts = points_all + (size_t)b * n * 3;
    const unsigned char *__restrict__ valid = valid_all ? valid_all + (size_t)b * n : nullptr;
    float *__restrict__ on = normals_all + ((size_t)b * n + q) * 3;
    float *__restrict__ ov = variation_all + (size_t)b * n + q;
    const float ux = pts[(size_t)3 * q], uy = pts[(size_t)3 * q + 1], uz = pts[(size_t)3 * q + 2];

    float nx = 0.f, ny = 0.f, nz = 0.f, var = 0.f;
    // a masked query; a query with a non-finite coordinate finds no finite distance below and ends with zero neighbours
    const bool query_ok = valid == nullptr || valid[q] != 0;
    if (query_ok) {  // wave-uniform
        unsigned long long key[P];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int c = lane * P + j;
            const bool in = c < n;
            const int cs = in ? c : 0;
            const float *src = pts + (size_t)3 * cs;
            const float d = sqdist(ux, uy, uz, src[0], src[1], src[2]);
            const bool ok = in && (valid == nullptr || valid[cs] != 0) && (d < __builtin_inff());  // NaN / inf never pass
            key[j] = ok ? (((unsigned long long)(unsigned)f2i(d) << 32) | (unsigned)c) : kInfKey;
            cnt += ok ? 1 : 0;
        }
        const int nvalid = (int)wave_sum_f32((float)cnt);  // <= 2048: exact
        const int kk = k < nvalid ? k : nvalid;
        if (kk >= 3) {  // wave-uniform
            sort_keys<P>(key);
            int mine = 0;
            unsigned farthest = 0;  // squared distance bits of the last neighbour popped
            for (int r = 0; r < kk; ++r) {
                const unsigned hd = (unsigned)(key[0] >> 32);
                const unsigned mn = wave_min_u32(hd);
                const uint64_t tie = __ballot(hd == mn);
                const int wl = __builtin_ctzll(tie);  // lanes own ascending index ranges: lowest lane = lowest index
                const int picked = __builtin_amdgcn_readlane((int)(unsigned)key[0], wl);
                mine = lane == r ? picked : mine;
                farthest = mn;
                if (lane == wl) {
#pragma unroll
                    for (int j = 0; j + 1 < P; ++j) key[j] = key[j + 1];
                    key[P - 1] = kInfKey;
                }
            }
            const bool act = lane < kk;
            const float *src = pts + (size_t)3 * lds_index(mine, n);
            const float px = act ? src[0] : 0.f, py = act ? src[1] : 0.f, pz = act ? src[2] : 0.f;
            const float inv = 1.f / (float)kk;
            const float mx = wave_sum_f32(px) * inv, my = wave_sum_f32(py) * inv, mz = wave_sum_f32(pz) * inv;
            const float dx = act ? px - mx : 0.f, dy = act ? py - my : 0.f, dz = act ? pz - mz : 0.f;
            float a00 = wave_sum_f32(dx * dx), a11 = wave_sum_f32(dy * dy), a22 = wave_sum_f32(dz * dz);
            float a01 = wave_sum_f32(dx * dy), a02 = wave_sum_f32(dx * dz), a12 = wave_sum_f32(dy * dz);
            const float tr = (a00 + a11) + a22;
            // all neighbours coincide with the query -- told by the distances: the mean of equal values need not be that value
            // in fp32, so the moments may hold rounding instead of zeros -- or the moments overflowed: zeros
            if (farthest != 0u && tr > 0.f && tr < __builtin_inff()) {
                const float sc = 1.f / tr;
                a00 *= sc; a11 *= sc; a22 *= sc; a01 *= sc; a02 *= sc; a12 *= sc;
                float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
#pragma unroll
                for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
                    PN2_JACOBI_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
                    PN2_JACOBI_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
                    PN2_JACOBI_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
                }
                // smallest eigenvalue, the lower index on a tie
                float l0 = a00, ex = v00, ey = v10, ez = v20;
                if (a11 < l0) { l0 = a11; ex = v01; ey = v11; ez = v21; }
                if (a22 < l0) { l0 = a22; ex = v02; ey = v12; ez = v22; }
                const float len = __builtin_sqrtf((ex * ex + ey * ey) + ez * ez);
                ex /= len; ey /= len; ez /= len;
                var = (l0 > 0.f ? l0 : 0.f) / ((a00 + a11) + a22);
                bool flip;
                if (orient == 0) {  // the component of largest magnitude is positive
                    const float ax = __builtin_fabsf(ex), ay = __builtin_fabsf(ey), az = __builtin_fabsf(ez);
                    const float big = (ax >= ay && ax >= az) ? ex : (ay >= az ? ey : ez);
                    flip = big < 0.f;
                    nx = flip ? -ex : ex; ny = flip ? -ey : ey; nz = flip ? -ez : ez;
                } else {
                    const float *vp = viewpoint_all + (size_t)3 * b;
                    const float wx = vp[0] - ux, wy = vp[1] - uy, wz = vp[2] - uz;
                    if (orient == 1) {  // towards the viewpoint
                        flip = ((ex * wx + ey * wy) + ez * wz) < 0.f;
                        nx = flip ? -ex : ex; ny = flip ? -ey : ey; nz = flip ? -ez : ez;
                    } else {  // the reference's per-component rule: (2 * (n * (camera - p) > 0) - 1) * n
                        nx = ex * wx > 0.f ? ex : -ex;
                        ny = ey * wy > 0.f ? ey : -ey;
                        nz = ez * wz > 0.f ? ez : -ez;
                    }
                }
                if (!(len > 0.f)) { nx = 0.f; ny = 0.f; nz = 0.f; var = 0.f; }
            }
        }
    }
    if (lane == 0) {
        on[0] = nx; on[1] = ny; on[2] = nz;
        *ov = var;
    }
}

}  // namespace pn2

extern "C" int pn2x_cloud_normals(int b, int n, int k, int orient, const float *points, const unsigned char *valid,
                                   const float *viewpoint, float *normals, float *variation, void *stream) {
    if (b < 1 || n < 3 || n > PN2X_CLOUD_NORMALS_MAX_N || k < 3 || k > PN2X_CLOUD_NORMALS_MAX_K || orient < 0 || orient > 2)
        return PN2_EINVAL;
    if (b > PN2X_CLOUD_NORMALS_MAX_B) return PN2_ERANGE;
    if (!points || !viewpoint || !normals || !variation) return PN2_ENULL;
    const dim3 grid((n + 3) / 4, b);
    hipStream_t st = (hipStream_t)stream;
#define PN2_CN_CASE(PP)                                                                                                              \
    if (n <= 64 * PP) {                                                                                                              \
        hipLaunchKernelGGL(pn2::cloud_normals_kernel<PP>, grid, dim3(256), 0, st, n, k, orient, points, valid, viewpoint, normals,    \
                           variation);                                                                                               \
        return pn2::check_launch();                                                                                                  \
    }
    PN2_CN_CASE(1) PN2_CN_CASE(2) PN2_CN_CASE(4) PN2_CN_CASE(8) PN2_CN_CASE(16) PN2_CN_CASE(32)
#undef PN2_CN_CASE
    static_assert(PN2X_CLOUD_NORMALS_MAX_N == 64 * 32, "the register-resident selection holds 32 keys per lane");
    return PN2_EINVAL;
}

extern "C" void pn2x_cloud_normals_limits(int *max_b, int *max_n, int *max_k) {
    if (max_b) *max_b = PN2X_CLOUD_NORMALS_MAX_B;
    if (max_n) *max_n = PN2X_CLOUD_NORMALS_MAX_N;
    if (max_k) *max_k = PN2X_CLOUD_NORMALS_MAX_K;
}
