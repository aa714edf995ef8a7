// hand_lbs.h -- device arithmetic of posing a TABLE hand (HandModel.skinning_tables / lbs_forward_from_tables), shared by the
// hand-pose optimiser (hand_pose.hip) and the hand-object interaction report (hand_interact.hip): Rodrigues, the per-lane joint
// set-up, the level-by-level kinematic chain, the 12-float joint record, skinning one vertex, placing a point and the pose
// features.  One definition, so that the report measures the very hand the optimiser posed: for the same pose both kernels give
// the same floats (tests/test_gpu_hand_pose_interact_bits.py).  Anything changed here changes both kernels' bits at once.
// How the angles are formed, what is reduced over the vertices and how the pose-blend offset is formed stay with each kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_device.h"

namespace pn2 {
namespace lbs {

constexpr int NJ = 21, MAXK = 4, NPOSE = 45, NB = NPOSE / 3;  // joints, weights per vertex, joint angles, pose blocks
constexpr int NF = 9 * NB, KP = NF + 1;                       // pose features vec(R_b - I); a packed posedirs row (one zero column)
static_assert(KP % 8 == 0 && KP % 16 == 8, "eight full k-groups of 16 and one of 8");

// hand_model.rodrigues: I + sin K + (1 - cos) K K with K the cross-product matrix of aa / max(|aa|, 1e-12)
__device__ __forceinline__ void rodrigues(float ax, float ay, float az, float *R) {
    const float n = fmaxf(sqrtf(ax * ax + ay * ay + az * az), 1e-12f);
    const float kx = ax / n, ky = ay / n, kz = az / n;
    const float s = sinf(n), oc = 1.0f - cosf(n);
    R[0] = 1.0f + oc * (-(kz * kz) - ky * ky);  R[1] = s * -kz + oc * (kx * ky);            R[2] = s * ky + oc * (kx * kz);
    R[3] = s * kz + oc * (kx * ky);            R[4] = 1.0f + oc * (-(kz * kz) - kx * kx);  R[5] = s * -kx + oc * (ky * kz);
    R[6] = s * -ky + oc * (kx * kz);           R[7] = s * kx + oc * (ky * kz);             R[8] = 1.0f + oc * (-(ky * ky) - kx * kx);
}

// a pose block's features vec(R_b - I) (9 floats)
__device__ __forceinline__ void pose_features(const float *R, float *feat) {
#pragma unroll
    for (int k = 0; k < 9; ++k) feat[k] = R[k] - ((k & 3) == 0 ? 1.f : 0.f);
}

// What lane `lane` of the skeleton's wave owns: joint j (lanes >= NJ carry joint 0 and are masked where it matters), its parent,
// its pose block (-1: none, the root included), its depth in the tree and the deepest joint's.  The clamps keep an index outside
// the tables from ever being read through.
struct Joint {
    int j, pa, blk, depth, maxdepth;
    bool is_joint;
};

__device__ __forceinline__ Joint lane_joint(const int *parents, const int *pose_block, int lane) {
    Joint J;
    J.is_joint = lane < NJ;
    J.j = J.is_joint ? lane : 0;
    J.pa = J.j == 0 ? 0 : min(max(parents[J.j], 0), J.j - 1);
    J.blk = pose_block[J.j];
    if (J.blk < 0 || J.blk >= NB || J.j == 0) J.blk = -1;
    J.depth = 0;
    for (int s = 0, q = J.j; s < NJ; ++s)
        if (q != 0) {
            q = min(max(parents[q], 0), q - 1);
            ++J.depth;
        }
    J.maxdepth = J.depth;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) J.maxdepth = max(J.maxdepth, __shfl_xor(J.maxdepth, m, 64));
    return J;
}

// The kinematic chain, the whole wave in step: every lane starts at the root's rotation and rest position, and at level
// J.depth takes its parent's transform by cross-lane read: t = t_pa + R_pa off, R = R_pa Rl (R_pa for a joint without a block).
__device__ __forceinline__ void chain(const Joint &J, const float *Rl, const float *off, const float *rootR, const float *rootT,
                                      float *R, float *t) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rootR[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = rootT[k];
    for (int lvl = 1; lvl <= J.maxdepth; ++lvl) {
        float pR[9], pt[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) pR[k] = __shfl(R[k], J.pa, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = __shfl(t[k], J.pa, 64);
        if (J.depth == lvl) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                t[k] = pt[k] + fmaf(pR[3 * k + 2], off[2], fmaf(pR[3 * k + 1], off[1], pR[3 * k] * off[0]));
            if (J.blk >= 0) mat3_mul(pR, Rl, R);
            else {
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = pR[k];
            }
        }
    }
}

// the joint's record in the skeleton table: R (9, row-major), t (3); the barriers around it are the caller's
__device__ __forceinline__ void store_joint(float4 *sk, const Joint &J, const float *R, const float *t) {
    if (J.is_joint) {
        sk[3 * J.j] = make_float4(R[0], R[1], R[2], R[3]);
        sk[3 * J.j + 1] = make_float4(R[4], R[5], R[6], R[7]);
        sk[3 * J.j + 2] = make_float4(R[8], t[0], t[1], t[2]);
    }
}

// A vertex before the translation: sum over its k < K weights of w_k (R_j e_k + t_j), j = bits 5 k .. 5 k + 4 of the packed word
// `p`, the transform as fma(R2, e2, fma(R1, e1, R0 e0)) + t, the weights in index order.  ek(k, j) -> (e_k = v_rest - rest joint j,
// w_k) is the caller's; `blend` adds the pose-blend offset (bx, by, bz) to every e_k.
template <typename EK>
__device__ __forceinline__ void skin_vertex(int p, int K, const float4 *sk, bool blend, float bx, float by, float bz, EK ek, float &x,
                                            float &y, float &z) {
    x = 0.f; y = 0.f; z = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) {
            const int jn = min((p >> (5 * k)) & 31, NJ - 1);
            float4 e = ek(k, jn);
            if (blend) {
                e.x += bx; e.y += by; e.z += bz;
            }
            const float4 a = sk[3 * jn], b = sk[3 * jn + 1], d = sk[3 * jn + 2];
            const float qx = fmaf(a.z, e.z, fmaf(a.y, e.y, a.x * e.x)) + d.y;
            const float qy = fmaf(b.y, e.z, fmaf(b.x, e.y, a.w * e.x)) + d.z;
            const float qz = fmaf(d.x, e.z, fmaf(b.w, e.y, b.z * e.x)) + d.w;
            x = k == 0 ? qx * e.w : fmaf(qx, e.w, x);
            y = k == 0 ? qy * e.w : fmaf(qy, e.w, y);
            z = k == 0 ? qz * e.w : fmaf(qz, e.w, z);
        }
}

// a posed point (vertex or joint) in the camera frame: + translation, a MANO-structured hand centred first (cen: the root or zero)
__device__ __forceinline__ void place(bool mano, const float *cen, const float *tr, float &x, float &y, float &z) {
    if (mano) {
        x = (x - cen[0]) + tr[0]; y = (y - cen[1]) + tr[1]; z = (z - cen[2]) + tr[2];
    } else {
        x += tr[0]; y += tr[1]; z += tr[2];
    }
}

// the keypoint a MANO-structured hand's vertex is (skin_pack bits 25..29: the table joint; 0: none)
__device__ __forceinline__ int keypoint_of(int p) { return min((p >> 25) & 31, NJ - 1); }

}  // namespace lbs
}  // namespace pn2
