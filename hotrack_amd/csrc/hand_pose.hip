// hand_pose.hip -- the hand-pose particle optimiser (reference gf_optimize_hand_pose.evaluate / optimize,
// optimization_hand.py:215-293, :335-394) on the device: per iteration one launch that evaluates every candidate hand and
// one single-workgroup launch that applies the update.  No host sync, no atomics, no waits between workgroups.
//
// hand_pose_eval_kernel.  The hand model is a plain linear-blend-skinning table (HandModel.skinning_tables): a workgroup
// stages, once, per vertex and weight the rest offset v_rest - j_k and the weight (one float4) plus the packed joint indices
// into LDS; after that each of its four WAVES evaluates candidates on its own (candidate = wave, no workgroup barrier in
// the candidate loop, so one wave's serial skeleton phase overlaps the other waves' vertex phase):
//   skeleton: lane j owns joint j -- its pose block's angles, Rodrigues, then the kinematic chain level by level (the parent's
//             transform comes by cross-lane read), 12 floats per joint into the wave's LDS slot;
//   keypoint terms: lane j's distance to pred_kp / last_frame_kp, three wave sums;
//   vertices: lane l skins vertices l, l + 64, ... (13 for 778), and per vertex transforms into the object frame, reads the
//             nearest voxel with pn2s_nearest's arithmetic (sdf_device.h) and the silhouette pixel -- the two gathers of four
//             vertices are issued before any is used;
//   then wave reductions (max, five minima, an integer count) and lane 0 writes the candidate's terms.
// Sums over lanes are xor butterflies, the vertex loop is in index order: a candidate's result does not depend on the grid.
//
// hand_pose_update_kernel.  One workgroup of 1024 threads: gate, energies, weights and the 20 weighted sums (thread-strided
// in index order, a butterfly per wave, an in-order sum over the 16 waves -- as hand_shape.hip), then thread 0 applies the
// reference's update with its host branches as selects and threads 64..108 the 45 joint angles.
//
// hand_pose_eval_batch_kernel / hand_pose_update_batch_kernel (pn2x_hand_pose_opt_batch).  S independent problems per launch:
// the bodies above are the device functions hand_pose_eval_block / hand_pose_update_block, which the single kernels call with
// their own argument and the batched kernels with a Frame built from the batch's shared fields and the problem's record
// (pn2x_hand_pose_problem, a device array read at a workgroup-uniform address).  The eval grid's y and the update grid's x is
// the problem; a problem that is not active returns before it reads any of its record's pointers.  No workgroup waits for another.
//
// hand_pose_offsets_kernel / hand_pose_mano_eval_kernel (a pn2x_hand_pose_setup with posedirs set).  A hand with MANO's structure
// (skinning_tables' optional entries): per iteration a pre-pass builds every candidate's 135 pose features vec(R_b - I) -- the skeleton phase's
// own angle and Rodrigues functions -- and multiplies them with the packed pose blend shapes on the fp32 matrix cores into
// offsets (P, ceil16(3 V)); the MANO instantiation of hand_pose_eval_block (template <.., bool MANO>, if constexpr: the plain
// instantiations are the code they were) adds a vertex's offset to its staged v_rest - j_k, takes the fingertip keypoints from
// skinned vertices (the owner lane leaves the position in the tip joint's unused LDS slot; the keypoint terms run after the
// vertex loop), and centres on the root.  The update kernel is shared.
//
// hand_pose_offsets_batch_kernel / hand_pose_mano_eval_batch_kernel (pn2x_hand_pose_mano_opt_batch).  The MANO kernels for S
// problems per launch: the pre-pass is the device function hand_pose_offsets_block, which the single kernel calls with its own
// arguments and the batched one (grid z = the problem) with the record's state and slice z of ONE offsets workspace (S slices
// of P * ceil16(3 V) floats); an output element is the same 34 accumulations whatever the grid.  The batched evaluation builds
// its Frame as hand_pose_eval_batch_kernel does and points ManoExtra::offsets at the problem's slice.
//
// Posing the hand -- Rodrigues, the joint set-up, the chain, the joint record, skinning and placing a vertex, the pose features --
// is hand_lbs.h, shared with hand_interact.hip; the volume lookup is sdf_device.h's; the model's argument checks are hand_check.h's.
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstring>

#include "hand_check.h"
#include "hand_lbs.h"
#include "mfma_rows.h"
#include "pn2_common.h"
#include "sdf_device.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace hpose {

using namespace lbs;

constexpr int MAXP = 8192, MAXV = 1024, NC = 10, ND = 6 + NC;
// state (pn2_ext.h): rotation, translation, joint angles, search size, previous search size, previous success
constexpr int S_R = 0, S_T = 9, S_THETA = 12, S_SEARCH = 57, S_PREV = 73, S_PREV_OK = 89;
constexpr int TERMS = 4;  // per candidate: gate-independent energy, attraction term, penetration, 0
constexpr int UT = 1024, UW = UT / 64, NV = 3 + 1 + ND;  // update: w, w E, [E < origin], w * [qw | sample]

struct Frame {
    int P, V, K;
    const int *parents, *pose_block;
    const float *rest_j, *rest_v;
    const int *pack;
    const float *skin_w, *comps;
    float theta_scale;
    const float *pre, *state, *pred_kp, *last_kp;
    const unsigned char *vis;
    const float *obj_r, *obj_t;
    const void *vol;
    int res;
    float voxel_scale;
    const unsigned char *mask;
    int h, w;
    float fx, fy, cx, cy;
    float w_sil, w_pen, w_vis, w_invis, w_tmp, w_attr;
    float *terms, *out_verts, *out_kp;
};

// What the MANO instantiation reads beyond Frame (a kernel argument of its own: the plain kernels' arguments stay as they are).
struct ManoExtra {
    const float *offsets;    // (P, ldo): candidate-major pose-blend offsets, 3 v + coordinate
    const float *pose_mean;  // (45)
    const int *kp_vertex;    // (21): >= 0 = the keypoint is a skinned vertex (skin_pack bits 25..29 of that vertex name the joint)
    int ldo, centre;
};

inline size_t eval_lds_bytes(int v, int k) { return (size_t)v * k * sizeof(float4) + (size_t)v * sizeof(int); }

template <bool F16>
__device__ __forceinline__ float vol_round(float x) {  // a value of the volume's dtype (products and sums stay in it)
    if constexpr (F16) return __half2float(__float2half(x));
    else return x;
}

// [qw | pre[q] * search] of optimize() (:343-345): qw = sqrt(1 - x^2 - y^2 - z^2), NaN for a negative argument
__device__ __forceinline__ void candidate_sample(const float *__restrict__ pre, int q, const float *search, float *s) {
#pragma unroll
    for (int k = 0; k < ND; ++k) s[1 + k] = pre[(size_t)q * ND + k] * search[k];
    s[0] = sqrtf(1.0f - s[1] * s[1] - s[2] * s[2] - s[3] * s[3]);
}

// evaluate()'s last two lines (:284-293): the attraction term counts only when candidate 0 penetrates
__device__ __forceinline__ float candidate_energy(const float *__restrict__ terms, int q, bool gate) {
    const float base = terms[(size_t)q * TERMS], attr = terms[(size_t)q * TERMS + 1];
    return gate ? base + attr : base;
}

// a joint's angles: curr_theta + (coefficients @ comps[:10]) * theta_scale (get_kp_from_delta), for a MANO hand with the mean
// pose added as the model's forward() adds it
template <bool MANO>
__device__ __forceinline__ void joint_angles(const float *sp, const float (&cm)[NC][3], const float *cth, const float *pmean,
                                             float theta_scale, float *th) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float acc = sp[7] * cm[0][a];
#pragma unroll
        for (int cc = 1; cc < NC; ++cc) acc = fmaf(sp[7 + cc], cm[cc][a], acc);
        if constexpr (MANO) th[a] = pmean[a] + (cth[a] + acc * theta_scale);
        else th[a] = cth[a] + acc * theta_scale;
    }
}

// keypoint terms (:236-240, :259-262): lane j's distance to pred_kp / last_frame_kp, three wave sums
__device__ __forceinline__ void keypoint_terms(const Frame &A, int c, int j, bool is_joint, float kx, float ky, float kz,
                                               const float *pred, const float *last, float visf, float &vis_sum, float &inv_sum,
                                               float &tmp_sum) {
    if (A.out_kp && is_joint) {
        float *o = A.out_kp + ((size_t)c * NJ + j) * 3;
        o[0] = kx; o[1] = ky; o[2] = kz;
    }
    float dx = kx - pred[0], dy = ky - pred[1], dz = kz - pred[2];
    const float err = sqrtf(dx * dx + dy * dy + dz * dz);
    dx = kx - last[0]; dy = ky - last[1]; dz = kz - last[2];
    const float terr = sqrtf(dx * dx + dy * dy + dz * dz);
    vis_sum = wave_sum_xor(is_joint ? err * visf : 0.f);
    inv_sum = wave_sum_xor(is_joint ? err * (1.f - visf) : 0.f);
    tmp_sum = wave_sum_xor(is_joint ? terr : 0.f);
}

template <bool F16, bool MANO>
__device__ __forceinline__ void hand_pose_eval_block(const Frame A, const ManoExtra M) {
    extern __shared__ float4 dyn[];
    __shared__ float4 skel[4][NJ * 3];  // per wave and joint: R (9, row-major), t (3)
    const int V = A.V, K = A.K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float4 *tab = dyn;                                  // (K, V): v_rest - j_k, w_k
    int *pk = reinterpret_cast<int *>(dyn + (size_t)K * V);  // (V): joint indices 5 bits each, tip-region bits from bit 20

    for (int i = tid; i < V; i += 256) {
        const int p = A.pack[i];
        pk[i] = p;
        const float vx = A.rest_v[3 * i], vy = A.rest_v[3 * i + 1], vz = A.rest_v[3 * i + 2];
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) {
                const int jn = min((p >> (5 * k)) & 31, NJ - 1);
                tab[k * V + i] = make_float4(vx - A.rest_j[3 * jn], vy - A.rest_j[3 * jn + 1], vz - A.rest_j[3 * jn + 2], A.skin_w[i * K + k]);
            }
    }

    // ---- this lane's joint (lanes >= 21 carry joint 0's tables and are masked where it matters) ------------------------------
    const Joint J = lane_joint(A.parents, A.pose_block, lane);
    const bool is_joint = J.is_joint;
    const int j = J.j, pa = J.pa, blk = J.blk;
    float off[3], pred[3], last[3] = {0.f, 0.f, 0.f}, cth[3] = {0.f, 0.f, 0.f}, pmean[3] = {0.f, 0.f, 0.f}, cm[NC][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        off[a] = A.rest_j[3 * j + a] - A.rest_j[3 * pa + a];
        pred[a] = A.pred_kp[3 * j + a];
        if (A.last_kp) last[a] = A.last_kp[3 * j + a];
        if (blk >= 0) cth[a] = A.state[S_THETA + 3 * blk + a];
        if constexpr (MANO) {
            if (blk >= 0) pmean[a] = M.pose_mean[3 * blk + a];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) cm[c][a] = blk >= 0 ? A.comps[c * NPOSE + 3 * blk + a] : 0.f;
    }
    const float visf = A.vis[j] ? 1.f : 0.f;
    const unsigned long long vis_bits = __ballot(is_joint && A.vis[j]);
    const int nvis = __popcll(vis_bits), ninv = NJ - nvis;
    const float root[3] = {A.rest_j[0], A.rest_j[1], A.rest_j[2]};
    bool kp_from_vertex = false;  // MANO: this lane's keypoint is a skinned vertex (a fingertip)
    float cen[3] = {0.f, 0.f, 0.f};  // MANO: what is subtracted from vertices and keypoints before the translation
    if constexpr (MANO) {
        kp_from_vertex = is_joint && M.kp_vertex[j] >= 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[k] = M.centre ? root[k] : 0.f;
    }

    float R0[9], t0[3], search[ND], oR[9], ot[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        R0[k] = A.state[S_R + k];
        oR[k] = A.obj_r[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t0[k] = A.state[S_T + k];
        ot[k] = A.obj_t[k];
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) search[k] = A.state[S_SEARCH + k];
    const float fw = (float)A.w, fh = (float)A.h;
    float4 *sk = skel[wave];
    __syncthreads();

    for (int c0 = blockIdx.x * 4 + wave; c0 < A.P; c0 += gridDim.x * 4) {
        const int c = __builtin_amdgcn_readfirstlane(c0);
        float sp[1 + ND], S[9], Rg[9], tr[3];
        candidate_sample(A.pre, c, search, sp);
        quat_to_matrix(sp[0], sp[1], sp[2], sp[3], S);
        mat3_mul(R0, S, Rg);  // curr_r @ quat2mat(q), used as the root's rotation
#pragma unroll
        for (int k = 0; k < 3; ++k) tr[k] = t0[k] + sp[4 + k];

        // ---- skeleton -----------------------------------------------------------------------------------------------------------
        float th[3], Rl[9], R[9], t[3];
        joint_angles<MANO>(sp, cm, cth, pmean, A.theta_scale, th);
        rodrigues(th[0], th[1], th[2], Rl);
        chain(J, Rl, off, Rg, root, R, t);
        __builtin_amdgcn_wave_barrier();  // the previous candidate's reads of this slot are issued before these writes
        store_joint(sk, J, R, t);
        __builtin_amdgcn_wave_barrier();

        // ---- keypoint terms (a MANO hand's fingertips are skinned vertices: after the vertex loop) ------------------------------
        float vis_sum, inv_sum, tmp_sum;
        place(MANO, cen, tr, t[0], t[1], t[2]);  // from here on t is the lane's joint as a keypoint
        if constexpr (!MANO) keypoint_terms(A, c, j, is_joint, t[0], t[1], t[2], pred, last, visf, vis_sum, inv_sum, tmp_sum);

        // ---- vertices ------------------------------------------------------------------------------------------------------------
        float pen = 0.f, fmin5[5];
        int count = 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) fmin5[f] = __builtin_inff();
        constexpr int U = 4;
        for (int v0 = lane; v0 < V; v0 += 64 * U) {
            float sdf[U];
            int bg[U], bits[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int vv = min(v0 + 64 * u, V - 1);  // slots past the end repeat the last vertex and are masked below
                const int p = pk[vv];
                bits[u] = p >> 20;
                float x, y, z;
                float bx = 0.f, by = 0.f, bz = 0.f;  // MANO: the candidate's pose-blend offset of this vertex
                if constexpr (MANO) {
                    const float *b = M.offsets + (size_t)c * M.ldo + 3 * vv;
                    bx = b[0]; by = b[1]; bz = b[2];
                }
                skin_vertex(p, K, sk, MANO, bx, by, bz, [&](int k, int) { return tab[k * V + vv]; }, x, y, z);
                place(MANO, cen, tr, x, y, z);
                if constexpr (MANO) {
                    const int kj = keypoint_of(p);  // the keypoint this vertex is (0: none): its unused LDS slot
                    if (kj != 0 && v0 + 64 * u < V) sk[3 * kj + 2] = make_float4(0.f, x, y, z);
                }
                if (A.out_verts && v0 + 64 * u < V) {
                    float *o = A.out_verts + ((size_t)c * V + vv) * 3;
                    o[0] = x; o[1] = y; o[2] = z;
                }
                sdf[u] = sdf_nearest<F16>(A.vol, x, y, z, ot, oR, A.voxel_scale, A.res);
                // world2point2D (:13-21), .long() = truncation toward zero, clamp to the image (:242-246)
                const float px = x / z * A.fx + A.cx, py = y / z * A.fy + A.cy;
                const int row = min(max((int)fminf(fmaxf(py, -1.f), fh), 0), A.h - 1);
                const int col = min(max((int)fminf(fmaxf(px, -1.f), fw), 0), A.w - 1);
                bg[u] = A.mask[(size_t)row * A.w + col];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (v0 + 64 * u >= V) continue;
                const float s = sdf[u];
                if (s < 0.f) pen = fmaxf(pen, -s);
                const float tip = s > 0.f ? s : 0.f;  // sdf * (sdf > 0)
#pragma unroll
                for (int f = 0; f < 5; ++f)
                    if ((bits[u] >> f) & 1) fmin5[f] = fminf(fmin5[f], tip);
                count += bg[u] != 0;
            }
        }
        if constexpr (MANO) {
            __builtin_amdgcn_wave_barrier();  // the fingertip slots are written
            const float4 d = sk[3 * j + 2];
            keypoint_terms(A, c, j, is_joint, kp_from_vertex ? d.y : t[0], kp_from_vertex ? d.z : t[1], kp_from_vertex ? d.w : t[2],
                           pred, last, visf, vis_sum, inv_sum, tmp_sum);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            pen = fmaxf(pen, __shfl_xor(pen, m, 64));
            count += __shfl_xor(count, m, 64);
#pragma unroll
            for (int f = 0; f < 5; ++f) fmin5[f] = fminf(fmin5[f], __shfl_xor(fmin5[f], m, 64));
        }

        // ---- the candidate's terms, added in evaluate()'s order with torch's type promotion (:277-293) ----------------------------
        if (lane == 0) {
            float e = ((float)count / (float)V) * A.w_sil;
            e = e + vol_round<F16>(pen * A.w_pen);
            e = e + (vis_sum / (float)max(nvis, 1)) * A.w_vis;
            e = e + (inv_sum / (float)max(ninv, 1)) * A.w_invis;
            if (A.last_kp) e = e + (tmp_sum / (float)NJ) * A.w_tmp;
            constexpr int tipkp[5] = {8, 12, 16, 20, 4};  // get_attraction_loss: fingers whose tip keypoint is invisible
            float attr = 0.f;
#pragma unroll
            for (int f = 0; f < 5; ++f) attr = vol_round<F16>(attr + (((vis_bits >> tipkp[f]) & 1ull) ? fmin5[f] * 0.f : fmin5[f]));
            float *o = A.terms + (size_t)c * TERMS;
            o[0] = e;
            o[1] = vol_round<F16>(attr * A.w_attr);
            o[2] = pen;
            o[3] = 0.f;
        }
    }
}

template <bool F16>
__global__ void __launch_bounds__(256) hand_pose_eval_kernel(const Frame A) {
    hand_pose_eval_block<F16, false>(A, ManoExtra{});
}

template <bool F16>
__global__ void __launch_bounds__(256) hand_pose_mano_eval_kernel(const Frame A, const ManoExtra M) {
    hand_pose_eval_block<F16, true>(A, M);
}

// offsets (P, ldo) = features (P, 136) . posedirs^T: pd (ldo, 136) row-major, row 3 v + coordinate, column 135 and the rows
// from 3 V on zero.  A workgroup builds the features of OCT candidates in LDS -- thread per (candidate, pose block): the block's
// angles by joint_angles / rodrigues as the skeleton phase forms them, minus the identity -- and its four waves take 16-row
// tiles of pd (blockIdx.y-strided): the tile's 136 columns in registers, one v_mfma_f32_16x16x4_f32 per 4 columns against each
// of the four 16-candidate groups, a lane's four consecutive outputs as one 16-byte store.  In k-group g a lane supplies
// columns 16 g + 4 (lane / 16) + s of both operands (one 16-byte load each); the last group is half as wide.
constexpr int OCT = 64;

// The body is a device function: the single kernel calls it with its own arguments, the batched one with a problem's.
__device__ __forceinline__ void hand_pose_offsets_block(int P, int ntiles, const float *__restrict__ pd,
                                                        const float *__restrict__ pose_mean, const float *__restrict__ comps,
                                                        float theta_scale, const float *__restrict__ pre,
                                                        const float *__restrict__ state, float *__restrict__ out) {
    using mrows::f32x4;
    __shared__ float4 feat4[OCT * KP / 4];
    float *feat = reinterpret_cast<float *>(feat4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c0 = blockIdx.x * OCT;
    float search[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) search[k] = state[S_SEARCH + k];
    for (int i = tid; i < OCT * NB; i += 256) {
        const int cl = i / NB, b = i - cl * NB, c = c0 + cl;
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};  // a row past the end: zero features
        if (c < P) {
            float sp[1 + ND], cm[NC][3], cth[3], pmean[3], th[3];
            candidate_sample(pre, c, search, sp);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                cth[a] = state[S_THETA + 3 * b + a];
                pmean[a] = pose_mean[3 * b + a];
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) cm[cc][a] = comps[cc * NPOSE + 3 * b + a];
            }
            joint_angles<true>(sp, cm, cth, pmean, theta_scale, th);
            rodrigues(th[0], th[1], th[2], R);
        }
        pose_features(R, feat + cl * KP + 9 * b);
    }
    if (tid < OCT) feat[tid * KP + NF] = 0.f;
    __syncthreads();

    const int r = lane & 15, q = lane >> 4;
    for (int nt = blockIdx.y * 4 + wave; nt < ntiles; nt += gridDim.y * 4) {
        const float *arow = pd + (size_t)(16 * nt + r) * KP;
        f32x4 a[KP / 16];
#pragma unroll
        for (int g = 0; g < KP / 16; ++g) a[g] = *reinterpret_cast<const f32x4 *>(arow + 16 * g + 4 * q);
        const float2 a8 = *reinterpret_cast<const float2 *>(arow + 16 * (KP / 16) + 2 * q);
#pragma unroll
        for (int mt = 0; mt < OCT / 16; ++mt) {
            const float *xr = feat + (16 * mt + r) * KP;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < KP / 16; ++g) {
                const f32x4 x = *reinterpret_cast<const f32x4 *>(xr + 16 * g + 4 * q);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s], x[s], acc, 0, 0, 0);
            }
            const float2 x8 = *reinterpret_cast<const float2 *>(xr + 16 * (KP / 16) + 2 * q);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a8.x, x8.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a8.y, x8.y, acc, 0, 0, 0);
            const int cand = c0 + 16 * mt + r;
            if (cand < P) *reinterpret_cast<f32x4 *>(out + (size_t)cand * (16 * ntiles) + 16 * nt + 4 * q) = acc;
        }
    }
}

__global__ void __launch_bounds__(256) hand_pose_offsets_kernel(int P, int ntiles, const float *__restrict__ pd,
                                                                const float *__restrict__ pose_mean, const float *__restrict__ comps,
                                                                float theta_scale, const float *__restrict__ pre,
                                                                const float *__restrict__ state, float *__restrict__ out) {
    hand_pose_offsets_block(P, ntiles, pd, pose_mean, comps, theta_scale, pre, state, out);
}

// a record is read through the constant address space: nothing writes the table while a kernel that reads it runs, and a
// read-only, workgroup-uniform address makes every field a scalar load
typedef __attribute__((address_space(4))) pn2x_hand_pose_problem ConstProblem;

// The batch: `shared` holds what the problems have in common (its per-problem fields are unset), `prob` the S records.
struct Batch {
    Frame shared;
    const pn2x_hand_pose_problem *prob;
};

// the shared frame with a problem's fields set from its record: one in host memory, or a ConstProblem on the device
template <typename Record>
__host__ __device__ __forceinline__ Frame problem_frame(const Frame &shared, const Record *r) {
    Frame A = shared;
    A.rest_j = r->rest_joints; A.rest_v = r->rest_verts; A.state = r->state; A.pred_kp = r->pred_kp; A.last_kp = r->last_kp;
    A.vis = r->vis_mask; A.obj_r = r->obj_r; A.obj_t = r->obj_t; A.vol = r->vol; A.mask = r->mask; A.h = r->h; A.w = r->w;
    A.fx = r->fx; A.fy = r->fy; A.cx = r->cx; A.cy = r->cy; A.terms = r->work;
    return A;
}

template <bool F16>
__global__ void __launch_bounds__(256) hand_pose_eval_batch_kernel(const Batch B) {
    const ConstProblem *r = (const ConstProblem *)B.prob + blockIdx.y;
    if (!r->active) return;
    hand_pose_eval_block<F16, false>(problem_frame(B.shared, r), ManoExtra{});
}

// The MANO batch (pn2x_hand_pose_mano_opt_batch): M.offsets is the base of the batch's offsets workspace, s slices of P * ldo
// floats; problem z's pre-pass writes slice z (grid z = the problem) and its evaluation (grid y = the problem) reads it.
__global__ void __launch_bounds__(256) hand_pose_offsets_batch_kernel(int P, int ntiles, const float *__restrict__ pd,
                                                                      const float *__restrict__ pose_mean,
                                                                      const float *__restrict__ comps, float theta_scale,
                                                                      const float *__restrict__ pre,
                                                                      const pn2x_hand_pose_problem *__restrict__ prob,
                                                                      float *__restrict__ offsets) {
    const ConstProblem *r = (const ConstProblem *)prob + blockIdx.z;
    if (!r->active) return;
    hand_pose_offsets_block(P, ntiles, pd, pose_mean, comps, theta_scale, pre, r->state,
                            offsets + (size_t)blockIdx.z * (size_t)P * (size_t)(16 * ntiles));
}

template <bool F16>
__global__ void __launch_bounds__(256) hand_pose_mano_eval_batch_kernel(const Batch B, const ManoExtra M0) {
    const ConstProblem *r = (const ConstProblem *)B.prob + blockIdx.y;
    if (!r->active) return;
    ManoExtra M = M0;
    M.offsets = M0.offsets + (size_t)blockIdx.y * (size_t)B.shared.P * (size_t)M0.ldo;
    hand_pose_eval_block<F16, true>(problem_frame(B.shared, r), M);
}

__global__ void __launch_bounds__(256) hand_pose_energy_kernel(int P, const float *__restrict__ terms, float *__restrict__ energy) {
    const bool gate = terms[2] != 0.f;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < P; q += gridDim.x * 256) energy[q] = candidate_energy(terms, q, gate);
}

__device__ __forceinline__ void hand_pose_update_block(int P, const float *__restrict__ pre, const float *__restrict__ terms,
                                                       const float *__restrict__ comps, float theta_scale, float c2, float beta,
                                                       float one_minus_beta, float *__restrict__ state, float *__restrict__ trace) {
    __shared__ float red[UW * NV], tot[NV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool gate = terms[2] != 0.f;
    const float origin = candidate_energy(terms, 0, gate);
    float search[ND], acc[NV];
#pragma unroll
    for (int k = 0; k < ND; ++k) search[k] = state[S_SEARCH + k];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.f;
    for (int q = tid; q < P; q += UT) {
        const float e = candidate_energy(terms, q, gate);
        const bool better = e < origin;
        const float w = (origin - e) * (better ? 1.f : 0.f);  // (origin_energy - energy) * better_mask, NaN and all (:351)
        float s[1 + ND];
        candidate_sample(pre, q, search, s);
        acc[0] += w;
        acc[1] += e * w;
        acc[2] += better ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 1 + ND; ++k) acc[3 + k] += s[k] * w;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = wave_sum_xor(acc[v]);
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[wave * NV + v] = acc[v];
    }
    __syncthreads();
    if (tid < NV) {
        float a = 0.f;
        for (int w = 0; w < UW; ++w) a += red[w * NV + tid];
        tot[tid] = a;
    }
    __syncthreads();
    const float wsum = tot[0];
    const bool success = tot[2] > 0.f;

    if (tid >= 64 && tid < 64 + NPOSE && success) {  // curr_theta += (mt[7:] @ comps[:10]) * theta_scale (:363)
        const int a = tid - 64;
        float d = (tot[3 + 7] / wsum) * comps[a];
#pragma unroll
        for (int c = 1; c < NC; ++c) d = fmaf(tot[3 + 7 + c] / wsum, comps[c * NPOSE + a], d);
        state[S_THETA + a] = state[S_THETA + a] + d * theta_scale;
    }
    if (tid != 0) return;

    const float mean_e = success ? tot[1] / wsum : origin;
    float mt[1 + ND];
#pragma unroll
    for (int k = 0; k < 1 + ND; ++k) mt[k] = tot[3 + k] / wsum;  // NaN without a better candidate: selected away below
    const float qn = sqrtf(mt[0] * mt[0] + mt[1] * mt[1] + mt[2] * mt[2] + mt[3] * mt[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) mt[k] /= qn;
    if (success) {
        float R0[9], S[9], Rn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) R0[k] = state[S_R + k];
        quat_to_matrix(mt[0], mt[1], mt[2], mt[3], S);
        mat3_mul(R0, S, Rn);
        // re-projection onto SO(3): Gram-Schmidt on the first two rows (rotation_from_ortho6d + transpose, :377-378)
        float x[3] = {Rn[0], Rn[1], Rn[2]}, yr[3] = {Rn[3], Rn[4], Rn[5]}, z[3], y[3];
        normalize3(x);
        z[0] = x[1] * yr[2] - x[2] * yr[1]; z[1] = x[2] * yr[0] - x[0] * yr[2]; z[2] = x[0] * yr[1] - x[1] * yr[0];
        normalize3(z);
        y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            state[S_R + k] = x[k];
            state[S_R + 3 + k] = y[k];
            state[S_R + 6 + k] = z[k];
            state[S_T + k] = state[S_T + k] + mt[4 + k];
        }
    }
    // update_seach_size on mean_transform[:, 1:] (:295-298) and its smoothing (:381-386)
    float s[ND], nrm = 0.f;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        s[k] = fabsf(success ? mt[1 + k] : 0.f) + 1e-3f;
        nrm += s[k] * s[k];
    }
    nrm = sqrtf(nrm);
    const bool both = state[S_PREV_OK] != 0.f && success;
    if (trace) {
        trace[0] = origin;
        trace[1] = mean_e;
        trace[2] = success ? 1.f : 0.f;
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        float ns = mean_e * c2 * s[k] / nrm + 1e-3f;
        if (both) ns = beta * ns + one_minus_beta * state[S_PREV + k];
        state[S_SEARCH + k] = ns;
        if (success) state[S_PREV + k] = ns;
        if (trace) trace[3 + k] = ns;
    }
    state[S_PREV_OK] = success ? 1.f : 0.f;
}

__global__ void __launch_bounds__(UT) hand_pose_update_kernel(int P, const float *__restrict__ pre, const float *__restrict__ terms,
                                                              const float *__restrict__ comps, float theta_scale, float c2, float beta,
                                                              float one_minus_beta, float *__restrict__ state, float *__restrict__ trace) {
    hand_pose_update_block(P, pre, terms, comps, theta_scale, c2, beta, one_minus_beta, state, trace);
}

// one workgroup per problem; `it` picks the iteration's row of the problem's trace slice
__global__ void __launch_bounds__(UT) hand_pose_update_batch_kernel(int P, const float *__restrict__ pre,
                                                                    const pn2x_hand_pose_problem *__restrict__ prob,
                                                                    const float *__restrict__ comps, float theta_scale, float c2,
                                                                    float beta, float one_minus_beta, int it) {
    const ConstProblem *r = (const ConstProblem *)prob + blockIdx.x;
    if (!r->active) return;
    hand_pose_update_block(P, pre, r->work, comps, theta_scale, c2, beta, one_minus_beta, r->state,
                           r->trace ? r->trace + (size_t)it * (3 + ND) : nullptr);
}

// records handed over by value (kernel arguments are captured with a graph): thread t copies 8-byte word t of the chunk
constexpr int FILL = 16, REC_WORDS = sizeof(pn2x_hand_pose_problem) / 8;
static_assert(sizeof(pn2x_hand_pose_problem) == 128 && sizeof(pn2x_hand_pose_problem) % 8 == 0, "record layout (pn2_ext.h)");
struct ProblemChunk {
    unsigned long long w[FILL * REC_WORDS];
};

__global__ void __launch_bounds__(FILL * REC_WORDS) hand_pose_problems_fill_kernel(unsigned long long *__restrict__ dst, int n,
                                                                                   const ProblemChunk c) {
    const int t = threadIdx.x;
    if (t < n * REC_WORDS) dst[t] = c.w[t];
}

}  // namespace hpose
}  // namespace pn2

using namespace pn2;
using namespace pn2::hpose;

static_assert(sizeof(pn2x_hand_pose_setup) == 136, "record layout (pn2_ext.h)");

extern "C" int pn2x_hand_pose_opt_supported(int p, int v, int j, int k, int d_pose, int res) {
    return (p >= 1 && p <= MAXP && v >= 1 && v <= MAXV && j == NJ && k >= 1 && k <= MAXK && d_pose == NC && res >= 1 &&
            res <= 1024 && (res & 1) == 1) ? 1 : 0;
}

static inline int offsets_ld(int v) { return (3 * v + 15) / 16 * 16; }

extern "C" long pn2x_hand_pose_opt_work_floats(int p) { return p < 0 ? (long)PN2_EINVAL : (long)TERMS * p; }
extern "C" long pn2x_hand_pose_mano_work_floats(int p, int v) {
    return (p < 0 || v < 0) ? (long)PN2_EINVAL : (long)p * offsets_ld(v);
}
extern "C" long pn2x_hand_pose_opt_batch_work_floats(int p, int s) {
    return (p < 0 || s < 0) ? (long)PN2_EINVAL : (long)TERMS * p * s;
}
extern "C" long pn2x_hand_pose_mano_batch_work_floats(int p, int v, int s) {
    return (p < 0 || v < 0 || s < 0) ? (long)PN2_EINVAL : (long)s * p * offsets_ld(v);
}

// the optimiser's setup: the model (hand_check.h) and its own candidates
static void check_setup(const pn2x_hand_pose_setup *s, Faults &f) {
    if (!is_record(s, f)) return;
    check_hand_model(*s, f);
    f.inval |= s->p < 1;
    f.range |= !pn2x_hand_pose_opt_supported(s->p, s->v, s->j, s->k, NC, s->res);
    f.null |= !s->comps || !s->pre;
}

// a record in host memory: a single problem's frame, or an active record on its way into a batch's table
static void check_frame(const pn2x_hand_pose_problem *r, Faults &f) {
    if (!is_record(r, f)) return;
    f.inval |= r->h < 1 || r->w < 1;
    f.range |= (long)r->h * r->w >= (1L << 31);
    f.null |= !r->state || !r->work || !r->rest_joints || !r->rest_verts || !r->pred_kp || !r->vis_mask || !r->obj_r || !r->obj_t ||
              !r->vol || !r->mask;
}

// the candidates' pose-blend offsets, a MANO setup's scratch: 16-byte stores
static void check_offsets(const pn2x_hand_pose_setup *s, const float *offsets, Faults &f) {
    if (!is_record(s) || !s->posedirs) return;
    f.inval |= ((uintptr_t)offsets & 15) != 0;
    f.null |= !offsets;
}

// the kernel argument with the setup's fields set and the per-problem ones unset (the batched kernel sets them from its record)
static Frame shared_frame(const pn2x_hand_pose_setup &s) {
    Frame A;
    memset(&A, 0, sizeof(A));
    A.P = s.p; A.V = s.v; A.K = s.k;
    A.parents = s.parents; A.pose_block = s.pose_block; A.pack = s.skin_pack; A.skin_w = s.skin_w; A.comps = s.comps;
    A.theta_scale = s.theta_scale; A.pre = s.pre; A.res = s.res; A.voxel_scale = s.voxel_scale;
    A.w_sil = s.w_sil; A.w_pen = s.w_pen; A.w_vis = s.w_vis; A.w_invis = s.w_invis; A.w_tmp = s.w_temporal; A.w_attr = s.w_attr;
    return A;
}

// a single problem's kernel argument: what hand_pose_eval_batch_kernel takes from a record, from a record in host memory
static Frame single_frame(const pn2x_hand_pose_setup &s, const pn2x_hand_pose_problem &r) {
    return problem_frame(shared_frame(s), &r);
}

// One evaluation launch of `Kernel` (an instantiation of the three evaluation kernels), whose dynamic-LDS limit is raised once
// per device.  A workgroup's four waves take a candidate each; the grid's x deals a problem's ceil(p / 4) workgroups evenly
// over at most max(1, 3 * compute units / active), so the launch covers the device at most three times (a single problem
// is active == 1); its y is the problem.
template <auto Kernel, typename... Args>
static void launch_eval(const pn2x_hand_pose_setup &s, int active, int problems, hipStream_t st, const Args &...args) {
    static PerDeviceOnce raised;
    if (raised.first_use())
        (void)hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)eval_lds_bytes(MAXV, MAXK));
    const int wgs = (s.p + 3) / 4, share = 3 * num_compute_units() / active, cap = share < 1 ? 1 : share;
    const int rounds = (wgs + cap - 1) / cap, gx = (wgs + rounds - 1) / rounds;
    hipLaunchKernelGGL(Kernel, dim3(gx, problems), dim3(256), eval_lds_bytes(s.v, s.k), st, args...);
}

// what the MANO evaluation reads beyond its Frame; `offsets` is a single problem's scratch or the base of a batch's workspace
static ManoExtra mano_extra(const pn2x_hand_pose_setup &s, const float *offsets) {
    ManoExtra M;
    M.offsets = offsets; M.pose_mean = s.pose_mean; M.kp_vertex = s.kp_vertex; M.ldo = offsets_ld(s.v); M.centre = s.centre_root;
    return M;
}

// The pre-pass grid: x = groups of OCT candidates, y = as many strides over the 16-row tiles as cover the compute units three
// times, the device shared among the `active` problems (a single problem is active == 1); the batched launch's z is the problem.
static dim3 offsets_grid(const pn2x_hand_pose_setup &s, int active, int problems) {
    const int ntiles = offsets_ld(s.v) / 16, gx = (s.p + OCT - 1) / OCT, most = (ntiles + 3) / 4;
    const int cover = (int)(3L * num_compute_units() / ((long)gx * active));
    return dim3(gx, cover < 1 ? 1 : (cover > most ? most : cover), problems);
}

// a single problem's evaluation: the plain kernel, or for a MANO setup the pose-offset pre-pass and the MANO kernel
static void eval_single(const pn2x_hand_pose_setup &s, const Frame &A, float *offsets, hipStream_t st) {
    if (!s.posedirs) {
        if (s.vol_f16) launch_eval<hand_pose_eval_kernel<true>>(s, 1, 1, st, A);
        else launch_eval<hand_pose_eval_kernel<false>>(s, 1, 1, st, A);
        return;
    }
    const ManoExtra M = mano_extra(s, offsets);
    hipLaunchKernelGGL(hand_pose_offsets_kernel, offsets_grid(s, 1, 1), dim3(256), 0, st, s.p, M.ldo / 16, s.posedirs, s.pose_mean,
                       s.comps, s.theta_scale, s.pre, A.state, offsets);
    if (s.vol_f16) launch_eval<hand_pose_mano_eval_kernel<true>>(s, 1, 1, st, A, M);
    else launch_eval<hand_pose_mano_eval_kernel<false>>(s, 1, 1, st, A, M);
}

extern "C" int pn2x_hand_pose_energy(const pn2x_hand_pose_setup *setup, const pn2x_hand_pose_problem *frame, float *offsets,
                                     float *energy, float *out_verts, float *out_kp, void *stream) {
    Faults f;
    check_setup(setup, f);
    check_frame(frame, f);
    check_offsets(setup, offsets, f);
    f.null |= !energy;
    if (f.code() != PN2_OK) return f.code();
    Frame A = single_frame(*setup, *frame);
    A.out_verts = out_verts; A.out_kp = out_kp;
    hipStream_t st = (hipStream_t)stream;
    eval_single(*setup, A, offsets, st);
    hipLaunchKernelGGL(hand_pose_energy_kernel, dim3((setup->p + 255) / 256), dim3(256), 0, st, setup->p, frame->work, energy);
    return check_launch();
}

extern "C" int pn2x_hand_pose_opt(const pn2x_hand_pose_setup *setup, const pn2x_hand_pose_problem *frame, float *offsets,
                                  int iterations, double scaling_coefficient2, double beta, void *stream) {
    Faults f;
    check_setup(setup, f);
    f.inval |= iterations < 0;
    f.range |= iterations > 4096;
    if (iterations != 0) {  // nothing to do: the frame is not looked at
        check_frame(frame, f);
        check_offsets(setup, offsets, f);
    }
    if (f.code() != PN2_OK || iterations == 0) return f.code();
    const pn2x_hand_pose_setup &s = *setup;
    const Frame A = single_frame(s, *frame);
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < iterations; ++it) {
        eval_single(s, A, offsets, st);
        hipLaunchKernelGGL(hand_pose_update_kernel, dim3(1), dim3(UT), 0, st, s.p, s.pre, frame->work, s.comps, s.theta_scale,
                           (float)scaling_coefficient2, (float)beta, (float)(1.0 - beta), frame->state,
                           frame->trace ? frame->trace + (size_t)it * (3 + ND) : nullptr);
    }
    return check_launch();
}

extern "C" int pn2x_hand_pose_problems_fill(pn2x_hand_pose_problem *problems, int s, const pn2x_hand_pose_problem *host, void *stream) {
    Faults f;
    f.inval = s < 1;
    f.range = s > 65535;
    f.null = !problems || !host;
    if (f.code() != PN2_OK) return f.code();
    for (int q = 0; q < s; ++q)  // the records are host memory here: what the batched entry cannot check
        if (host[q].active) check_frame(host + q, f);
    if (f.code() != PN2_OK) return f.code();
    hipStream_t st = (hipStream_t)stream;
    for (int q0 = 0; q0 < s; q0 += FILL) {
        const int n = s - q0 < FILL ? s - q0 : FILL;
        ProblemChunk c;
        memset(&c, 0, sizeof(c));
        memcpy(c.w, host + q0, (size_t)n * sizeof(pn2x_hand_pose_problem));
        hipLaunchKernelGGL(hand_pose_problems_fill_kernel, dim3(1), dim3(FILL * REC_WORDS), 0, st,
                           reinterpret_cast<unsigned long long *>(problems + q0), n, c);
    }
    return check_launch();
}

// what the two batched entries check beside the setup
static void check_batch(int s, int active, int iterations, Faults &f) {
    f.inval |= s < 1 || active < 0 || active > s || iterations < 0;
    f.range |= s > 65535 || iterations > 4096;
}

// The batched entries' loop over checked arguments: per iteration, for a MANO setup (`offsets` is then the batch's workspace)
// the pre-pass over (candidate groups, tile strides, problem), then the evaluation over (candidates, problem) and the update
// with a workgroup per problem.
static int opt_batch_loop(const pn2x_hand_pose_setup &s, int n, int active, const pn2x_hand_pose_problem *problems, float *offsets,
                          int iterations, double scaling_coefficient2, double beta, hipStream_t st) {
    Batch B;
    B.shared = shared_frame(s);
    B.prob = problems;
    const bool mano = s.posedirs != nullptr;
    const ManoExtra M = mano_extra(s, offsets);
    for (int it = 0; it < iterations; ++it) {
        if (mano) {
            hipLaunchKernelGGL(hand_pose_offsets_batch_kernel, offsets_grid(s, active, n), dim3(256), 0, st, s.p, M.ldo / 16,
                               s.posedirs, s.pose_mean, s.comps, s.theta_scale, s.pre, problems, offsets);
            if (s.vol_f16) launch_eval<hand_pose_mano_eval_batch_kernel<true>>(s, active, n, st, B, M);
            else launch_eval<hand_pose_mano_eval_batch_kernel<false>>(s, active, n, st, B, M);
        } else if (s.vol_f16) {
            launch_eval<hand_pose_eval_batch_kernel<true>>(s, active, n, st, B);
        } else {
            launch_eval<hand_pose_eval_batch_kernel<false>>(s, active, n, st, B);
        }
        hipLaunchKernelGGL(hand_pose_update_batch_kernel, dim3(n), dim3(UT), 0, st, s.p, s.pre, problems, s.comps, s.theta_scale,
                           (float)scaling_coefficient2, (float)beta, (float)(1.0 - beta), it);
    }
    return check_launch();
}

extern "C" int pn2x_hand_pose_opt_batch(const pn2x_hand_pose_setup *setup, int s, int active, const pn2x_hand_pose_problem *problems,
                                        int iterations, double scaling_coefficient2, double beta, void *stream) {
    Faults f;
    check_setup(setup, f);
    check_batch(s, active, iterations, f);
    f.inval |= is_record(setup) && setup->posedirs;  // a MANO setup goes to pn2x_hand_pose_mano_opt_batch
    if (f.code() != PN2_OK || iterations == 0) return f.code();
    if (!problems) return PN2_ENULL;
    if (active == 0) return PN2_OK;
    return opt_batch_loop(*setup, s, active, problems, nullptr, iterations, scaling_coefficient2, beta, (hipStream_t)stream);
}

extern "C" int pn2x_hand_pose_mano_opt_batch(const pn2x_hand_pose_setup *setup, int s, int active,
                                             const pn2x_hand_pose_problem *problems, float *offsets, int iterations,
                                             double scaling_coefficient2, double beta, void *stream) {
    Faults f;
    check_setup(setup, f);
    check_batch(s, active, iterations, f);
    f.inval |= is_record(setup) && !setup->posedirs;  // a plain setup goes to pn2x_hand_pose_opt_batch
    const bool work = iterations != 0 && active != 0;  // nothing to do: neither the table nor the workspace is looked at
    if (work) {
        f.inval |= ((uintptr_t)offsets & 15) != 0;  // 16-byte stores; a slice is a multiple of 16 floats
        f.null |= !offsets || !problems;
    }
    if (f.code() != PN2_OK || !work) return f.code();
    return opt_batch_loop(*setup, s, active, problems, offsets, iterations, scaling_coefficient2, beta, (hipStream_t)stream);
}
