// hand_interact.hip -- hand-object penetration and contact of tracked hand sequences (include/pn2_ext.h:
// pn2x_hand_interaction_metrics): what the hand-pose optimiser minimises (reference optimization_hand.py:264-293), reported per
// frame and per sequence for the hands the tracker ended up with.  The definitions are this project's; the reference has no such
// evaluation.  Two launches for all F frames of S sequences, no host sync, no atomics, no waits between workgroups.
//
// hand_interact_rows_kernel.  One workgroup of four waves per FRAME (the hand-pose kernels pose thousands of candidates of one
// frame; here every frame has its own pose, shape table, object pose and volume):
//   wave 0      the skeleton, lane j = joint j: Rodrigues of its pose block's angles (+ pose_mean), then the kinematic chain level by
//               level under the frame's root rotation MATRIX (the parent's transform by cross-lane read), 12 floats per joint to LDS;
//   wave 1      a MANO-structured hand's 135 pose features vec(R_b - I), thread per pose block, to LDS;
//   wave 2      the frame's rest joints to LDS;
//   all waves   thread t skins vertices t, t + 256, ...: a MANO hand first adds its pose-blend offset (3 x 135 multiply-adds per
//               vertex in column order, on the vector ALUs: the frames' features differ, there is no candidate batch to put on the
//               matrix cores and no offsets workspace), then k <= 4 weighted joint transforms in weight order, the centring and
//               the translation; object frame and voxel exactly as pn2s_nearest (sdf_device.h), the volume's value as fp32;
//   reduction   max / min / integer count per thread, xor butterflies per wave, the four waves in index order;
//   wave 0      the 21 keypoints (joints, or a MANO hand's fingertip vertices, left in LDS by their owner threads) against pred_kp.
// hand_interact_reduce_kernel.  One workgroup per sequence: lane c sums column c of the sequence's rows in frame order (fp64).
//
// The posing arithmetic is hand_lbs.h, shared with hand_pose.hip (HandModel.lbs_forward_from_tables: v_rest - j_k [+ offset],
// fma(R2, e2, fma(R1, e1, R0 e0)) + t, weights in index order; fp32 throughout), and the lookup is sdf_device.h's: a frame whose
// pose is an optimiser's candidate gets that candidate's vertices and keypoints bit for bit
// (tests/test_gpu_hand_pose_interact_bits.py).  What differs is how the pose-blend offset is formed (above): with a non-zero
// posedirs table a MANO-structured hand agrees with the optimiser's to rounding, not to the bit.
#include "hand_check.h"
#include "hand_lbs.h"
#include "pn2_common.h"
#include "sdf_device.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace hinter {

using namespace lbs;

constexpr int COLS = 8, T = 256, W = T / 64;

struct Args {
    int F, S, G, V, K, res, centre, mano;
    const int *parents, *pose_block, *pack, *kp_vertex;
    const float *skin_w, *posedirs, *pose_mean;
    const float *global_r, *global_t, *theta, *obj_r, *obj_t, *pred_kp, *rest_j, *rest_v;
    const int *rest_of, *seq_off;
    const void *const *vols;
    float voxel_scale, contact;
    float *rows, *out_verts, *out_kp;
};

// a pose block's angles: theta (+ pose_mean for a MANO hand, as the model's forward() adds it)
__device__ __forceinline__ void block_angles(const Args &A, const float *theta, int b, float *th) {
#pragma unroll
    for (int a = 0; a < 3; ++a) th[a] = A.mano ? A.pose_mean[3 * b + a] + theta[3 * b + a] : theta[3 * b + a];
}

template <bool F16>
__global__ void __launch_bounds__(T) hand_interact_rows_kernel(const Args A) {
    __shared__ float4 skel[NJ * 3];  // per joint: R (9, row-major), t (3)
    __shared__ float4 restj[NJ];     // the frame's rest joints
    __shared__ float4 kpv[NJ];       // a MANO hand's keypoint vertices (slot = the table joint)
    __shared__ float4 feat4[KP / 4]; // vec(R_b - I), 135 features and a zero
    __shared__ float red_f[W][2 + 5];
    __shared__ int red_i[W][2];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = A.V, K = A.K;
    float *row = A.rows + (size_t)f * COLS;

    // the frame's sequence: the last q with seq_off[q] <= f (empty sequences share an offset with the next)
    int q = 0;
    for (int hi = A.S - 1; q < hi;) {
        const int mid = (q + hi + 1) >> 1;
        if (A.seq_off[mid] <= f) q = mid; else hi = mid - 1;
    }
    const void *vol = A.vols[q];
    if (vol == nullptr) {  // (a sequence with frames and no volume is the caller's error: the row is zero, nothing is read)
        if (tid < COLS) row[tid] = 0.f;
        return;
    }
    const int g = min(max(A.rest_of[f], 0), A.G - 1);  // (an index outside the tables can never be read through)
    const float *rest_j = A.rest_j + (size_t)g * NJ * 3, *rest_v = A.rest_v + (size_t)g * V * 3;
    const float *theta = A.theta + (size_t)f * NPOSE;
    float tr[3], oR[9], ot[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) oR[k] = A.obj_r[(size_t)f * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tr[k] = A.global_t[(size_t)f * 3 + k];
        ot[k] = A.obj_t[(size_t)f * 3 + k];
    }
    const float cen[3] = {A.centre ? rest_j[0] : 0.f, A.centre ? rest_j[1] : 0.f, A.centre ? rest_j[2] : 0.f};

    float t[3] = {0.f, 0.f, 0.f};  // wave 0, lane j: joint j's posed position
    if (wave == 0) {
        // ---- skeleton (lanes >= 21 carry joint 0 and write nothing) -----------------------------------------------------------------
        const Joint J = lane_joint(A.parents, A.pose_block, lane);
        float off[3], th[3] = {0.f, 0.f, 0.f}, Rl[9], R[9];
#pragma unroll
        for (int a = 0; a < 3; ++a) off[a] = rest_j[3 * J.j + a] - rest_j[3 * J.pa + a];
        if (J.blk >= 0) block_angles(A, theta, J.blk, th);
        rodrigues(th[0], th[1], th[2], Rl);
        chain(J, Rl, off, A.global_r + (size_t)f * 9, rest_j, R, t);
        store_joint(skel, J, R, t);
    } else if (wave == 1) {
        // ---- a MANO hand's pose features: the skeleton's own angle and Rodrigues functions, minus the identity ------------------------
        float *feat = reinterpret_cast<float *>(feat4);
        if (A.mano && lane < NB) {
            float th[3], R[9];
            block_angles(A, theta, lane, th);
            rodrigues(th[0], th[1], th[2], R);
            pose_features(R, feat + 9 * lane);
        }
        if (lane == NB) feat[NF] = 0.f;
    } else if (wave == 2) {
        if (lane < NJ) restj[lane] = make_float4(rest_j[3 * lane], rest_j[3 * lane + 1], rest_j[3 * lane + 2], 0.f);
    }
    __syncthreads();

    // ---- vertices ---------------------------------------------------------------------------------------------------------------------
    float pen = 0.f, smin = __builtin_inff(), fmin5[5];
    int count = 0, has = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) fmin5[i] = __builtin_inff();
    for (int v = tid; v < V; v += T) {
        const int p = A.pack[v];
        const float vx = rest_v[3 * v], vy = rest_v[3 * v + 1], vz = rest_v[3 * v + 2];
        float bx = 0.f, by = 0.f, bz = 0.f;  // MANO: the frame's pose-blend offset of this vertex
        if (A.mano) {
            // rows 3 v .. 3 v + 2 of the packed table (136 columns, 16-byte aligned rows): one chain per coordinate, column order
            const float4 *pd = reinterpret_cast<const float4 *>(A.posedirs + (size_t)3 * v * KP);
#pragma unroll 2
            for (int c = 0; c < KP / 4; ++c) {
                const float4 x = feat4[c], a = pd[c], b = pd[KP / 4 + c], d = pd[2 * (KP / 4) + c];
                bx = fmaf(a.w, x.w, fmaf(a.z, x.z, fmaf(a.y, x.y, fmaf(a.x, x.x, bx))));
                by = fmaf(b.w, x.w, fmaf(b.z, x.z, fmaf(b.y, x.y, fmaf(b.x, x.x, by))));
                bz = fmaf(d.w, x.w, fmaf(d.z, x.z, fmaf(d.y, x.y, fmaf(d.x, x.x, bz))));
            }
        }
        float x, y, z;
        skin_vertex(p, K, skel, A.mano, bx, by, bz, [&](int k, int jn) {
            const float4 rj = restj[jn];
            return make_float4(vx - rj.x, vy - rj.y, vz - rj.z, A.skin_w[(size_t)v * K + k]);
        }, x, y, z);
        place(A.mano, cen, tr, x, y, z);
        if (A.mano) {
            const int kj = keypoint_of(p);  // the keypoint this vertex is (0: none)
            if (kj != 0) kpv[kj] = make_float4(x, y, z, 0.f);
        }
        if (A.out_verts) {
            float *o = A.out_verts + ((size_t)f * V + v) * 3;
            o[0] = x; o[1] = y; o[2] = z;
        }
        const float s = sdf_nearest<F16>(vol, x, y, z, ot, oR, A.voxel_scale, A.res);
        if (s < 0.f) {
            pen = fmaxf(pen, -s);
            ++count;
        }
        smin = fminf(smin, s);
        const int bits = (p >> 20) & 31;
        has |= bits;
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if ((bits >> i) & 1) fmin5[i] = fminf(fmin5[i], s);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        pen = fmaxf(pen, __shfl_xor(pen, m, 64));
        smin = fminf(smin, __shfl_xor(smin, m, 64));
        count += __shfl_xor(count, m, 64);
        has |= __shfl_xor(has, m, 64);
#pragma unroll
        for (int i = 0; i < 5; ++i) fmin5[i] = fminf(fmin5[i], __shfl_xor(fmin5[i], m, 64));
    }
    if (lane == 0) {
        red_f[wave][0] = pen;
        red_f[wave][1] = smin;
#pragma unroll
        for (int i = 0; i < 5; ++i) red_f[wave][2 + i] = fmin5[i];
        red_i[wave][0] = count;
        red_i[wave][1] = has;
    }
    __syncthreads();  // (also: the keypoint vertices are in LDS)
    if (wave != 0) return;

    // ---- keypoints: joint positions, or a MANO hand's fingertip vertices; centred as the vertices are ----------------------------------
    const bool is_joint = lane < NJ;
    const int j = is_joint ? lane : 0;
    float kx = t[0], ky = t[1], kz = t[2];
    place(A.mano, cen, tr, kx, ky, kz);
    if (A.mano && A.kp_vertex[j] >= 0) {
        const float4 d = kpv[j];
        kx = d.x; ky = d.y; kz = d.z;
    }
    if (A.out_kp && is_joint) {
        float *o = A.out_kp + ((size_t)f * NJ + j) * 3;
        o[0] = kx; o[1] = ky; o[2] = kz;
    }
    float kerr = 0.f;
    if (A.pred_kp) {
        const float *pk = A.pred_kp + ((size_t)f * NJ + j) * 3;
        const float dx = kx - pk[0], dy = ky - pk[1], dz = kz - pk[2];
        kerr = wave_sum_xor(is_joint ? sqrtf(dx * dx + dy * dy + dz * dz) : 0.f);
    }
    if (lane != 0) return;
    pen = red_f[0][0]; smin = red_f[0][1]; count = red_i[0][0]; has = red_i[0][1];
#pragma unroll
    for (int i = 0; i < 5; ++i) fmin5[i] = red_f[0][2 + i];
    for (int w = 1; w < W; ++w) {
        pen = fmaxf(pen, red_f[w][0]);
        smin = fminf(smin, red_f[w][1]);
        count += red_i[w][0];
        has |= red_i[w][1];
#pragma unroll
        for (int i = 0; i < 5; ++i) fmin5[i] = fminf(fmin5[i], red_f[w][2 + i]);
    }
    int touching = 0, fingers = 0;
    float gap = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i)  // fingers in index order: a fixed sum
        if ((has >> i) & 1) {
            ++fingers;
            touching += fmin5[i] <= A.contact ? 1 : 0;
            gap += fmaxf(fmin5[i], 0.f);
        }
    row[0] = pen;
    row[1] = (float)count / (float)V;
    row[2] = pen > 0.f ? 1.f : 0.f;
    row[3] = (float)touching;
    row[4] = fingers ? gap / (float)fingers : 0.f;
    row[5] = smin;
    row[6] = A.pred_kp ? kerr / (float)NJ : 0.f;
    row[7] = touching > 0 ? 1.f : 0.f;
}

// rows (F,8) -> seq (S,8): lane c of the sequence's workgroup adds column c of its rows in frame order (fp64, serial: the order
// depends on nothing but the sequence) and divides by its length.  A sequence without frames gets zeros and reads nothing.
__global__ void __launch_bounds__(64)
hand_interact_reduce_kernel(int F, int S, const float *__restrict__ rows, const int *__restrict__ seq_off, float *__restrict__ seq) {
    const int q = blockIdx.x, col = threadIdx.x;
    if (q >= S || col >= COLS) return;
    const int f0 = min(max(seq_off[q], 0), F), f1 = min(seq_off[q + 1], F);  // (offsets outside the rows can never be read through)
    float v = 0.f;
    if (f1 > f0) {
        double acc = 0.0;
        for (int f = f0; f < f1; ++f) acc += (double)rows[(size_t)f * COLS + col];
        v = (float)(acc / (double)(f1 - f0));
    }
    seq[(size_t)q * COLS + col] = v;
}

}  // namespace hinter
}  // namespace pn2

using namespace pn2;
using namespace pn2::hinter;

extern "C" int pn2x_hand_interaction_metrics(const pn2x_hand_pose_setup *model, int f, int s, int g, const float *global_r,
                                             const float *global_t, const float *theta, const float *obj_r, const float *obj_t,
                                             const float *pred_kp, const float *rest_joints, const float *rest_verts, const int *rest_of,
                                             const void *const *vols, const int *seq_off, float contact_threshold, float *rows,
                                             float *seq, float *out_verts, float *out_kp, void *stream) {
    Faults bad;
    const bool work = f > 0 && s > 0;
    bad.inval = f < 0 || s < 0 || g < 0 || !(contact_threshold >= 0.f) || (work && g < 1);
    if (is_record(model, bad)) {
        check_hand_model(*model, bad);
        bad.range |= !pn2x_hand_pose_opt_supported(1, model->v, model->j, model->k, 10, model->res);
    }
    if (work)
        bad.null |= !global_r || !global_t || !theta || !obj_r || !obj_t || !rest_joints || !rest_verts || !rest_of || !vols ||
                    !seq_off || !rows || !seq;
    if (bad.code() != PN2_OK) return bad.code();
    const int mask = 0xbf | (pred_kp ? 0x40 : 0);  // columns 0-5 and 7, and 6 with pred_kp
    if (!work) return mask;
    const pn2x_hand_pose_setup &m = *model;
    Args A;
    A.F = f; A.S = s; A.G = g; A.V = m.v; A.K = m.k; A.res = m.res; A.mano = m.posedirs != nullptr; A.centre = A.mano ? m.centre_root : 0;
    A.parents = m.parents; A.pose_block = m.pose_block; A.pack = m.skin_pack; A.kp_vertex = m.kp_vertex;
    A.skin_w = m.skin_w; A.posedirs = m.posedirs; A.pose_mean = m.pose_mean;
    A.global_r = global_r; A.global_t = global_t; A.theta = theta; A.obj_r = obj_r; A.obj_t = obj_t; A.pred_kp = pred_kp;
    A.rest_j = rest_joints; A.rest_v = rest_verts; A.rest_of = rest_of; A.seq_off = seq_off; A.vols = vols;
    A.voxel_scale = m.voxel_scale; A.contact = contact_threshold;
    A.rows = rows; A.out_verts = out_verts; A.out_kp = out_kp;
    hipStream_t st = (hipStream_t)stream;
    if (m.vol_f16) hipLaunchKernelGGL(hand_interact_rows_kernel<true>, dim3(f), dim3(T), 0, st, A);
    else hipLaunchKernelGGL(hand_interact_rows_kernel<false>, dim3(f), dim3(T), 0, st, A);
    int rc = check_launch();
    if (rc != PN2_OK) return rc;
    hipLaunchKernelGGL(hand_interact_reduce_kernel, dim3(s), dim3(64), 0, st, f, s, (const float *)rows, seq_off, seq);
    rc = check_launch();
    return rc != PN2_OK ? rc : mask;
}
