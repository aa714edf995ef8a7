// iknet.hip -- eval-mode IKNet forward (reference hand_network.py:246-322) for up to 16 rows, fp32, BatchNorm folded into
// the Linear layers by the caller.
//
//   126 -> 6 x (1024, BN, ReLU) -> 60 at M <= 16 rows is a chain of GEMVs: 21.7 MB of weights, a few KB of activations.
//   Every launch streams its weight matrix once, straight into VGPRs with 16-byte loads issued before anything else, and
//   keeps the M x K activations in LDS.  One wave owns one output neuron: lane l holds the float4s l, l + 64, ... of the
//   neuron's weight row (coalesced 1 KB per load instruction), multiplies them with the same float4s of every activation
//   row, and the wave sums its 64 partials with the fixed DPP ladder of wave_sum_f32.  Workgroups of 4 waves -> 256
//   workgroups for a 1024-wide layer (every compute unit busy).  No atomics, no cross-workgroup communication: the order
//   of every sum is fixed, so two runs are bitwise equal, and a layer boundary is a launch boundary.
//
//   layer 1   builds its own input in LDS from the keypoints (no pack tensor): kp_hf = R^T (kp - t) / 0.2 ('kp' frame) or
//             kp * 5 ('camera' frame), bone = kp_hf - kp_hf[parent], pack = [kp_hf | bone] coordinate-major (x0..x20,
//             y0..y20, z0..z20; hand_network.py:283-292), padded to 128 columns (the weight's columns 126, 127 are zero).
//   layers 2-6 the same kernel on the previous layer's output (ping-pong work buffer).
//   head      one wave per joint computes its four quaternion outputs, adds the bias, writes raw_quat and converts the
//             quaternion to axis-angle (hand_utils.py:13-19 over rotations.py:144-152) in the same wave.
#include "pn2_common.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace iknet {

constexpr int MAXM = 16;     // rows per forward
constexpr int HID = 1024;    // hidden width
constexpr int KIN = 126;     // [kp_hf | bone], 2 x 63
constexpr int K1 = 128;      // KIN padded to a multiple of 4
constexpr int NJ = 15;       // joints of the head (15 x 4 quaternion outputs)
constexpr int NHID = 5;      // hidden 1024 -> 1024 layers
constexpr int NT = 256, NPB = NT / 64;

// parent of keypoint k in MANO order (hand_network.py:290): 0,0,1,2,3,0,5,6,7,0,...
__device__ __forceinline__ int parent_of(int k) { return (k == 0 || k % 4 == 1) ? 0 : k - 1; }

// keypoint k, axis a of row m in the network's frame
__device__ __forceinline__ float hand_frame(const float *kp, const float *R, const float *t, int camera, int m, int k, int a) {
    const float *p = kp + m * 63 + k * 3;
    if (camera) return p[a] * 5.f;
    const float *r = R + m * 9, *tt = t + m * 3;
    const float d0 = p[0] - tt[0], d1 = p[1] - tt[1], d2 = p[2] - tt[2];
    // (R^T d)_a = R[0][a] d0 + R[1][a] d1 + R[2][a] d2, then / scale (canonicalize, hand_utils.py:30-32)
    return (r[a] * d0 + r[3 + a] * d1 + r[6 + a] * d2) / 0.2f;
}

// y (M, N) = relu(x (M, K) W^T + b), W (N, K) row-major.  FIRST: x is built from kp / R / t (K == K1) and workgroup 0 also
// writes kp_hf (M, 3, 21) when kp_hf != nullptr.
template <int K, bool FIRST>
__global__ __launch_bounds__(NT) void iknet_layer_kernel(int M, int N, const float *__restrict__ x, const float *__restrict__ kp,
                                                         const float *__restrict__ R, const float *__restrict__ t, int camera,
                                                         float *__restrict__ kp_hf, const float *__restrict__ W,
                                                         const float *__restrict__ b, float *__restrict__ y) {
    constexpr int Q = K / 4;            // float4s per row
    constexpr int F = (Q + 63) / 64;    // float4s per lane
    extern __shared__ float4 xs4[];     // (M, Q)
    float *xs = reinterpret_cast<float *>(xs4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * NPB + wave;
    const bool live = n < N;

    // the weight row first: its loads are in flight while the activations are staged
    float4 w[F];
    const float4 *wr = reinterpret_cast<const float4 *>(W) + (size_t)(live ? n : 0) * Q;
#pragma unroll
    for (int j = 0; j < F; ++j) {
        const int q = lane + 64 * j;
        w[j] = (live && q < Q) ? wr[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }

    if constexpr (FIRST) {
        for (int i = tid; i < M * K; i += NT) {
            const int m = i / K, c = i % K;
            float v = 0.f;
            if (c < KIN) {
                const int bone = c >= 63, r = c - 63 * bone, a = r / 21, k = r % 21;
                v = hand_frame(kp, R, t, camera, m, k, a);
                if (bone) v = v - hand_frame(kp, R, t, camera, m, parent_of(k), a);
            }
            xs[i] = v;
        }
    } else {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        for (int i = tid; i < M * Q; i += NT) xs4[i] = x4[i];
    }
    __syncthreads();
    if constexpr (FIRST) {
        if (blockIdx.x == 0 && kp_hf != nullptr)
            for (int i = tid; i < M * 63; i += NT) kp_hf[i] = xs[(i / 63) * K + i % 63];
    }
    if (!live) return;

    const float bn = b[n];
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
        if (m < M) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < F; ++j) {
                const int q = lane + 64 * j;
                if (q < Q) {
                    const float4 v = xs4[m * Q + q];
                    a = __builtin_fmaf(w[j].x, v.x, a);
                    a = __builtin_fmaf(w[j].y, v.y, a);
                    a = __builtin_fmaf(w[j].z, v.z, a);
                    a = __builtin_fmaf(w[j].w, v.w, a);
                }
            }
            a = wave_sum_f32(a);
            if (lane == 0) y[(size_t)m * N + n] = fmaxf(a + bn, 0.f);
        }
    }
}

// head: workgroup = one wave = joint j; outputs 4j .. 4j+3 of raw_quat (M, 60), then MANO_theta (M, 45) columns 3j .. 3j+2
__global__ __launch_bounds__(64) void iknet_head_kernel(int M, const float *__restrict__ x, const float *__restrict__ W,
                                                        const float *__restrict__ b, float *__restrict__ raw,
                                                        float *__restrict__ theta) {
    constexpr int Q = HID / 4, F = Q / 64;
    extern __shared__ float4 xs4[];
    const int lane = threadIdx.x, j = blockIdx.x;
    float4 w[4][F];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float4 *wr = reinterpret_cast<const float4 *>(W) + (size_t)(4 * j + o) * Q;
#pragma unroll
        for (int f = 0; f < F; ++f) w[o][f] = wr[lane + 64 * f];
    }
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    for (int i = lane; i < M * Q; i += 64) xs4[i] = x4[i];
    __syncthreads();
    float bo[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) bo[o] = b[4 * j + o];

#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
        if (m < M) {
            float q[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float a = 0.f;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const float4 v = xs4[m * Q + lane + 64 * f];
                    a = __builtin_fmaf(w[o][f].x, v.x, a);
                    a = __builtin_fmaf(w[o][f].y, v.y, a);
                    a = __builtin_fmaf(w[o][f].z, v.z, a);
                    a = __builtin_fmaf(w[o][f].w, v.w, a);
                }
                q[o] = wave_sum_f32(a) + bo[o];
            }
            if (lane == 0) {
                float *rq = raw + (size_t)m * 60 + 4 * j;
                rq[0] = q[0];
                rq[1] = q[1];
                rq[2] = q[2];
                rq[3] = q[3];
                // q / (|q| + 1e-8); sin = sqrt(1 - w^2) -- 0 where rounding makes 1 - w^2 negative (the reference: NaN);
                // axis = xyz / max(sin, [sin < 1e-8]); angle = 2 acos(clamp(w, -1, 1)); no sign flip for w < 0
                const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) + 1e-8f;
                const float cw = q[0] / nrm, qx = q[1] / nrm, qy = q[2] / nrm, qz = q[3] / nrm;
                const float s2 = 1.f - cw * cw;
                const float s = s2 > 0.f ? sqrtf(s2) : 0.f;
                const float den = s < 1e-8f ? fmaxf(s, 1.f) : s;
                const float ang = 2.f * acosf(fminf(fmaxf(cw, -1.f), 1.f));
                float *th = theta + (size_t)m * 45 + 3 * j;
                th[0] = qx / den * ang;
                th[1] = qy / den * ang;
                th[2] = qz / den * ang;
            }
        }
    }
}

}  // namespace iknet
}  // namespace pn2

extern "C" int pn2x_iknet_supported(int m, int k_in, int hidden, int layers, int n_out) {
    using namespace pn2::iknet;
    return (m >= 1 && m <= MAXM && k_in == KIN && hidden == HID && layers == NHID + 1 && n_out == 4 * NJ) ? 1 : 0;
}

extern "C" long pn2x_iknet_work_floats(void) { return 2L * pn2::iknet::MAXM * pn2::iknet::HID; }

extern "C" int pn2x_iknet_forward(int m, int frame, const float *kp, const float *R, const float *t, const float *w1,
                                  const float *b1, const float *wh, const float *bh, const float *wo, const float *bo,
                                  float *work, float *kp_hf, float *raw_quat, float *theta, void *stream) {
    using namespace pn2;
    using namespace pn2::iknet;
    if (m < 1 || (frame != 0 && frame != 1)) return PN2_EINVAL;
    if (m > MAXM) return PN2_ERANGE;
    if (!kp || !w1 || !b1 || !wh || !bh || !wo || !bo || !work || !raw_quat || !theta) return PN2_ENULL;
    if (frame == 0 && (!R || !t)) return PN2_ENULL;
    for (const void *p : {(const void *)w1, (const void *)wh, (const void *)wo, (const void *)work})
        if ((uintptr_t)p % 16) return PN2_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float *a = work, *c = work + (size_t)MAXM * HID;
    const int grid = HID / NPB;
    hipLaunchKernelGGL((iknet_layer_kernel<K1, true>), dim3(grid), dim3(NT), (size_t)m * K1 * sizeof(float), st, m, HID, nullptr,
                       kp, R, t, frame, kp_hf, w1, b1, a);
    int rc = check_launch();
    if (rc) return rc;
    for (int l = 0; l < NHID; ++l) {
        hipLaunchKernelGGL((iknet_layer_kernel<HID, false>), dim3(grid), dim3(NT), (size_t)m * HID * sizeof(float), st, m, HID, a,
                           nullptr, nullptr, nullptr, 0, nullptr, wh + (size_t)l * HID * HID, bh + (size_t)l * HID, c);
        if ((rc = check_launch())) return rc;
        float *s = a;
        a = c;
        c = s;
    }
    hipLaunchKernelGGL(iknet_head_kernel, dim3(NJ), dim3(64), (size_t)m * HID * sizeof(float), st, m, a, wo, bo, raw_quat, theta);
    return check_launch();
}
