// seq_eval.hip -- the per-sequence evaluation of the object trackers on the device (include/pn2_ext.h: pn2x_posed_chamfer,
// pn2x_obj_pose_metrics).  Reference: track_network.py:91-94 (compute_chamfer), :429-433 (the two posed clouds per frame),
// pose_utils/metrics.py:6-143 (rot_diff_rad / trans_diff), part_dof_utils.py:54-78 (eval_part_full).  The reference builds an
// (M, N, 3) difference tensor per frame, twice; here all T frames of a sequence are one launch + a T-thread reduction, the
// distances never leave the registers, and nothing synchronises with the host.
#include "pn2_common.h"
#include "../../include/pn2_ext.h"

namespace pn2 {

constexpr int kCfThreads = 256;
constexpr int kCfQ = 2;                      // queries per thread: one packed fp32 pair (sqdist2)
constexpr int kCfTile = kCfThreads * kCfQ;   // queries per workgroup
constexpr int kCfChunk = 2048;               // candidates staged in LDS at a time: 32 KB of float4
constexpr int kCfUnroll = 8;                 // candidates per inner-loop trip (a chunk is padded to a multiple)

static inline int cf_tiles(int n) { return (n + kCfTile - 1) / kCfTile; }

struct CfPose {
    float r[9], t[3];
};

// p' = R p + t in the reference's order: a product, two multiply-adds along the row of R, then the translation
// (torch.matmul(p, R^T) + t).  Queries and candidates go through this one function, so a cloud posed twice with the same
// pose gives the same floats and its chamfer is exactly zero.
__device__ __forceinline__ void cf_pose(const CfPose &P, const float *__restrict__ p, float &x, float &y, float &z) {
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    x = __builtin_fmaf(p2, P.r[2], __builtin_fmaf(p1, P.r[1], p0 * P.r[0])) + P.t[0];
    y = __builtin_fmaf(p2, P.r[5], __builtin_fmaf(p1, P.r[4], p0 * P.r[3])) + P.t[1];
    z = __builtin_fmaf(p2, P.r[8], __builtin_fmaf(p1, P.r[7], p0 * P.r[6])) + P.t[2];
}

// grid (T, tiles(N) + tiles(M)): workgroup (t, g) handles, in frame t, 512 query points of A against all of B (g < tiles(N):
// direction 0) or 512 query points of B against all of A (direction 1) and writes the SUM of its queries' nearest distances to
// partial[t * tiles + g].  Every thread keeps two posed queries in registers; the other cloud is posed once per workgroup
// into LDS as float4, 2048 points at a time, and read back with one 16-byte read per candidate whose address is the same in
// every lane (a broadcast: no bank conflicts).  Squared distances in the difference form (pn2_common.h: sqdist2), the square
// root once per query on its minimum (sqrt is monotone and correctly rounded: the same float as the minimum of the roots).
__global__ void __launch_bounds__(kCfThreads)
posed_chamfer_kernel(int N, int M, const float *__restrict__ A, const float *__restrict__ B, const float *__restrict__ Ra,
                     const float *__restrict__ ta, const float *__restrict__ Rb, const float *__restrict__ tb,
                     float *__restrict__ partial) {
    __shared__ float4 cand[kCfChunk];
    __shared__ float wsum[kCfThreads / kWave];
    const int t = blockIdx.x, g = blockIdx.y, tilesA = (N + kCfTile - 1) / kCfTile;
    const bool fwd = g < tilesA;
    const int nq = fwd ? N : M, nc = fwd ? M : N, tile = fwd ? g : g - tilesA;
    const float *__restrict__ Q = fwd ? A : B, *__restrict__ C = fwd ? B : A;
    CfPose Pq, Pc;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float a = Ra[(size_t)t * 9 + i], b = Rb[(size_t)t * 9 + i];
        Pq.r[i] = fwd ? a : b;
        Pc.r[i] = fwd ? b : a;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a = ta[(size_t)t * 3 + i], b = tb[(size_t)t * 3 + i];
        Pq.t[i] = fwd ? a : b;
        Pc.t[i] = fwd ? b : a;
    }
    // queries tile * 512 + {tid, tid + 256}; an index past the cloud re-reads the last point and contributes nothing
    const int q0 = tile * kCfTile + (int)threadIdx.x, q1 = q0 + kCfThreads;
    pn2_f32x2 qx, qy, qz;
    {
        float x, y, z;
        cf_pose(Pq, Q + 3 * (size_t)(q0 < nq ? q0 : nq - 1), x, y, z);
        qx.x = x; qy.x = y; qz.x = z;
        cf_pose(Pq, Q + 3 * (size_t)(q1 < nq ? q1 : nq - 1), x, y, z);
        qx.y = x; qy.y = y; qz.y = z;
    }
    float m0 = __builtin_inff(), m1 = __builtin_inff();
    for (int c0 = 0; c0 < nc; c0 += kCfChunk) {
        const int cnt = (nc - c0) < kCfChunk ? (nc - c0) : kCfChunk;
        const int padded = (cnt + kCfUnroll - 1) / kCfUnroll * kCfUnroll;  // <= kCfChunk (a multiple of kCfUnroll)
        __syncthreads();  // the previous chunk has been read
        for (int j = threadIdx.x; j < padded; j += kCfThreads) {
            float x, y, z;
            cf_pose(Pc, C + 3 * (size_t)(c0 + (j < cnt ? j : 0)), x, y, z);  // padding repeats the chunk's first point
            cand[j] = make_float4(x, y, z, 0.f);
        }
        __syncthreads();
        for (int j = 0; j < padded; j += kCfUnroll) {
#pragma unroll
            for (int u = 0; u < kCfUnroll; ++u) {
                const float4 c = cand[j + u];
                const pn2_f32x2 d = sqdist2(qx, qy, qz, c.x, c.y, c.z);
                m0 = __builtin_fminf(m0, d.x);
                m1 = __builtin_fminf(m1, d.y);
            }
        }
    }
    float s = (q0 < nq ? __builtin_sqrtf(m0) : 0.f) + (q1 < nq ? __builtin_sqrtf(m1) : 0.f);
    s = wave_sum_f32(s);  // fixed order
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = wsum[0];
#pragma unroll
        for (int w = 1; w < kCfThreads / kWave; ++w) tot += wsum[w];
        partial[(size_t)t * gridDim.y + g] = tot;
    }
}

// out[t] = (sum of the direction-0 partials in tile order) / N + (direction 1) / M
__global__ void __launch_bounds__(64)
posed_chamfer_sum_kernel(int T, int N, int M, int tilesA, int tilesB, const float *__restrict__ partial, float *__restrict__ out) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const float *p = partial + (size_t)t * (tilesA + tilesB);
    float sa = 0.f, sb = 0.f;
    for (int i = 0; i < tilesA; ++i) sa += p[i];
    for (int i = 0; i < tilesB; ++i) sb += p[tilesA + i];
    out[t] = sa / (float)N + sb / (float)M;
}

// clamp to [-1, 1] that keeps a NaN: fminf / fmaxf return the bound instead, and a NaN rotation would read as an angle (0
// degrees under |cos|, so both accuracy flags set); the reference's torch.clamp keeps it and the flags' comparisons fail
__device__ __forceinline__ float pm_clamp(float c) { return c < -1.f ? -1.f : (c > 1.f ? 1.f : c); }

__device__ __forceinline__ float pm_angle(float trace) { return acosf(pm_clamp((trace - 1.f) / 2.f)); }

// One thread per frame: out[t] = {tdiff, rdiff (degrees), 5deg5cm, 10deg10cm}.  rot_diff_rad's branches (metrics.py:6-136):
// axis 0..2 the angle between the chosen columns (|cos| when up/down symmetric), 3 the minimum over identity and the three
// 180-degree flips, -1 over identity and the xz flip, anything else the geodesic angle.  trace(R1 S R2^T) with S = diag(s)
// is sum_i sum_k s_k R1[i][k] R2[i][k], formed per diagonal entry like the reference's matmul.
__global__ void __launch_bounds__(64)
obj_pose_metrics_kernel(int T, const float *__restrict__ gR, const float *__restrict__ gt, const float *__restrict__ pR,
                        const float *__restrict__ pt, int axis, int sym, float *__restrict__ out) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    float a[9], b[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { a[i] = gR[(size_t)t * 9 + i]; b[i] = pR[(size_t)t * 9 + i]; }
    float rad;
    if (axis >= 0 && axis <= 2) {
        const int c = axis;
        float d = (c == 0 ? a[0] * b[0] : c == 1 ? a[1] * b[1] : a[2] * b[2]);
        d += (c == 0 ? a[3] * b[3] : c == 1 ? a[4] * b[4] : a[5] * b[5]);
        d += (c == 0 ? a[6] * b[6] : c == 1 ? a[7] * b[7] : a[8] * b[8]);
        d = pm_clamp(d);
        if (sym) d = fabsf(d);
        rad = acosf(d);
    } else {
        auto trace = [&](float s0, float s1, float s2) {
            float tr = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) tr += (s0 * a[3 * i] * b[3 * i] + s1 * a[3 * i + 1] * b[3 * i + 1]) + s2 * a[3 * i + 2] * b[3 * i + 2];
            return tr;
        };
        rad = pm_angle(trace(1.f, 1.f, 1.f));
        if (axis == 3) {
            rad = fminf(rad, pm_angle(trace(-1.f, -1.f, 1.f)));
            rad = fminf(rad, pm_angle(trace(-1.f, 1.f, -1.f)));
            rad = fminf(rad, pm_angle(trace(1.f, -1.f, -1.f)));
        } else if (axis == -1) {
            rad = fminf(rad, pm_angle(trace(-1.f, 1.f, -1.f)));
        }
    }
    const float deg = rad / 3.14159265358979323846f * 180.f;
    const float dx = gt[(size_t)t * 3] - pt[(size_t)t * 3], dy = gt[(size_t)t * 3 + 1] - pt[(size_t)t * 3 + 1],
                dz = gt[(size_t)t * 3 + 2] - pt[(size_t)t * 3 + 2];
    const float td = sqrtf(dx * dx + dy * dy + dz * dz);
    float *o = out + (size_t)t * 4;
    o[0] = td;
    o[1] = deg;
    o[2] = (deg <= 5.f && td <= 0.05f) ? 1.f : 0.f;
    o[3] = (deg <= 10.f && td <= 0.10f) ? 1.f : 0.f;
}

}  // namespace pn2

extern "C" long pn2x_posed_chamfer_partial_floats(int n, int m, int t) {
    if (n < 0 || m < 0 || t < 0) return -1;
    return (long)t * (pn2::cf_tiles(n) + pn2::cf_tiles(m));
}

extern "C" int pn2x_posed_chamfer(int n, int m, int t, const float *a, const float *b, const float *ra, const float *ta,
                                   const float *rb, const float *tb, float *partial, long partial_floats, float *out,
                                   void *stream) {
    if (n < 0 || m < 0 || t < 0) return PN2_EINVAL;
    if (t == 0) return PN2_OK;
    if (n == 0 || m == 0) return PN2_EINVAL;
    if (!a || !b || !ra || !ta || !rb || !tb || !partial || !out) return PN2_ENULL;
    const int tilesA = pn2::cf_tiles(n), tilesB = pn2::cf_tiles(m);
    if (tilesA + tilesB > 65535) return PN2_ERANGE;
    if (partial_floats < (long)t * (tilesA + tilesB)) return PN2_ESCRATCH;
    hipLaunchKernelGGL(pn2::posed_chamfer_kernel, dim3(t, tilesA + tilesB), dim3(pn2::kCfThreads), 0, (hipStream_t)stream, n, m, a, b,
                       ra, ta, rb, tb, partial);
    hipLaunchKernelGGL(pn2::posed_chamfer_sum_kernel, dim3((t + 63) / 64), dim3(64), 0, (hipStream_t)stream, t, n, m, tilesA, tilesB,
                       (const float *)partial, out);
    return pn2::check_launch();
}

extern "C" int pn2x_obj_pose_metrics(int t, const float *gt_r, const float *gt_t, const float *pred_r, const float *pred_t, int axis,
                                      int up_and_down_sym, float *out, void *stream) {
    if (t < 0) return PN2_EINVAL;
    if (t == 0) return PN2_OK;
    if (!gt_r || !gt_t || !pred_r || !pred_t || !out) return PN2_ENULL;
    hipLaunchKernelGGL(pn2::obj_pose_metrics_kernel, dim3((t + 63) / 64), dim3(64), 0, (hipStream_t)stream, t, gt_r, gt_t, pred_r, pred_t,
                       axis, up_and_down_sym ? 1 : 0, out);
    return pn2::check_launch();
}
