// sdf_refine.hip -- the tracked object pose refined by damped Gauss-Newton on the SDF volume (include/pn2_sdf.h: pn2s_obj_refine,
// pn2s_obj_refine_batch): a few Levenberg-Marquardt steps on  sum_j w_j phi(R^T (p_j - t))^2  from the particle optimum of sdf.hip,
// one workgroup per problem, every iteration inside ONE launch.  The reference has no counterpart (its tracker is the particle
// search alone).  DESIGN.md 8o.
//
// All arithmetic is fp32, every operation rounded once unless it is written as fmaf; sums are plain additions in the order given.
// Pose: R (3,3) row-major and t (3); the object-frame point is q = R^T (p - t) (the tracker's (pcld - t) @ R).
//   1. point    e = p - t;  q_j = fmaf(e_2, R_2j, fmaf(e_1, R_1j, e_0 * R_0j))                            (to_object_frame)
//   2. cell     u_a = (q_a - bbox_min) / stride;  c_a = fminf(fmaxf(u_a, 0), (float)(res - 1));  i_a = (int)c_a;  f_a = c_a - (float)i_a
//               (x, y, z) = (f_0, f_1, f_2),  mx = 1 - x, my = 1 - y, mz = 1 - z;  cell (i_0 * res + i_1) * res + i_2 of the corner
//               layout holds d000 .. d111 (d_abc: a along x, c along z), the values Distance() reads.
//               inside = 0 < u_a < (float)(res - 1) for a = 0, 1, 2 (a NaN fails): the cell is not on the clamped border
//   3. value    c00 = d000 mz + d001 z,  c01 = d010 mz + d011 z,  c10 = d100 mz + d101 z,  c11 = d110 mz + d111 z
//               r = (c00 my + c01 y) mx + (c10 my + c11 y) x            (Distance's order, optimization_obj.py:223-226; NOT clamped)
//   4. gradient g_x = ((c10 - c00) my + (c11 - c01) y) / stride,   g_y = ((c01 - c00) mx + (c11 - c10) x) / stride,
//               g_z = (((d001 - d000) my + (d011 - d010) y) mx + ((d101 - d100) my + (d111 - d110) y) x) / stride
//               -- the exact derivative of the interpolant inside its cell, from the same eight values
//   5. Jacobian with the increment delta = (omega, dt),  R <- R exp([omega]x),  t <- t + dt:
//               J_0 = g_y q_z - g_z q_y,  J_1 = g_z q_x - g_x q_z,  J_2 = g_x q_y - g_y q_x                     (g x q)
//               J_(3+i) = -fmaf(R_i2, g_z, fmaf(R_i1, g_y, R_i0 * g_x))                                          (-R g)
//   6. weight   a = |r|;  valid = inside and a < band (a NaN or infinite sample fails);  knee = band * 0.5f
//               w = valid ? (a <= knee ? 1 : knee / a) : 0  (Huber);   an invalid point contributes r = 0, J = 0, w = 0
//   7. sums     per lane, over its points j = lane, lane + 256, ...:  v_k = w J_k;   A_kl += v_k J_l (k <= l, 21 values),
//               b_k += v_k r (6),  E += (w r) r,  n += valid ? 1 : 0           -- 29 values
//               then per wave by xor butterfly (lane l with l ^ 32 first), then the four waves added in the order 0, 1, 2, 3
//   8. decision (lane 0; state: accepted pose, its A, b, cost C_acc and count n_acc, lambda, the flag `stepped`)
//               C = E / fmaxf(n, 1)
//               first pass (iteration 0): the input pose is the accepted pose, C_0 = C, n_0 = n
//               stepped:  accept = C <= C_acc and n >= 0.5f * n_acc   (a NaN fails)
//                         accept:  the candidate becomes the accepted pose (with its A, b, C, n),  lambda = fmaxf(lambda / 3, 1e-7f)
//                         else:    the accepted pose stays,                                        lambda = fminf(lambda * 10, 1e7f)
//               not stepped: nothing is decided (the candidate IS the accepted pose)
//   9. step     (after the last pass: none)   M = A_acc,  M_kk = fmaf(lambda, A_kk, A_kk) + eps_n,  eps_n = 1e-5f * fmaxf(n_acc, 1)
//               Cholesky M = L L^T, column by column:  s = M_kk - sum_(m<k) L_km L_km (in order, one subtraction each),
//               L_kk = sqrtf(s),  L_ik = (M_ik - sum_(m<k) L_im L_km) / L_kk
//               y_k = (-b_k - sum_(m<k) L_km y_m) / L_kk,   delta_k = (y_k - sum_(m>k) L_mk delta_m) / L_kk  (k = 5 .. 0)
//               gain = 0 - b_0 delta_0 - .. - b_5 delta_5 (a product and a subtraction each): the decrease of E the model predicts
//               ok = n_acc >= 6 and every s > 0 and every |delta_k| finite and gain >= 1e-3f * (C_acc * fmaxf(n_acc, 1))  (a step that
//               promises under 0.1 % is not taken: the problem has converged, and a decision about it would be one about rounding)
//               not ok:  no step -- lambda = fminf(lambda * 10, 1e7f), stepped = false, the candidate is the accepted pose
//               ok:  stepped = true,  th2 = fmaf(o_2, o_2, fmaf(o_1, o_1, o_0 * o_0)),  th = sqrtf(th2)
//                    th2 < 1e-6f:  sa = 1 - th2 / 6,  ca = 0.5f - th2 / 24;   else  sa = sinf(th) / th,  h = sinf(0.5f * th),  ca = 2 h h / th2
//                    dR_ij = (i == j ? 1 - ca th2 : 0) + ca o_i o_j + sa K_ij,   K = [[0, -o_2, o_1], [o_2, 0, -o_0], [-o_1, o_0, 0]]
//                    (as  (diag + (ca o_i) o_j) + sa K_ij),   R' = R_acc dR (mat3_mul's chain), re-projected by the ortho6d rule of
//                    pn2s_obj_optimize (x = normalised row 0, z = normalised x x row 1, y = z x x; rows x, y, z),  t' = t_acc + dt
//  10. `iters` steps, iters + 1 passes: the last pass only evaluates and decides.  The result is the accepted pose, so the final cost
//      C_acc is never above C_0.  lambda starts at 1e-3f.
// stats (8): C_0, C_acc, n_0, n_acc, accepted steps, lambda, 0, 0.
// trace row k (kTraceRow = 72 floats, after pass k): [0..11] accepted pose, [12] lambda, [13] C_acc, [14] n_acc, [15] accept flag
//   (pass 0: 1), [16..27] the candidate evaluated in this pass, [28..48] its A (rows of the upper triangle), [49..54] its b, [55] its C,
//   [56] its n, [57] the lambda of this pass's solve, [58] ok, [59] whether this pass decided, [60..65] delta, [66..71] 0.
//
// One workgroup of 256 lanes per problem; the volume cell is one 16-byte (fp16) or two 16-byte (fp32) loads per point.  No atomics, no
// tickets, no scratch (the Cholesky's indices are compile-time constants), 560 bytes of LDS; two runs are bitwise equal; nothing
// is allocated or read back (capturable).  Data-dependent branches are selections; the loops are bounded by iters and n.
#include <cmath>

#include "frame_device.h"
#include "sdf_device.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {
namespace refine {

constexpr int kLanes = 256, kWaves = kLanes / kWave, kSums = 29, kTraceRow = PN2S_REFINE_TRACE_ROW, kMaxIters = PN2S_REFINE_MAX_ITERS;
constexpr float kLambda0 = 1e-3f, kLambdaMin = 1e-7f, kLambdaMax = 1e7f, kEps = 1e-5f, kMinGain = 1e-3f;

struct Args {
    const float *pcld;
    const int *cloud_off;        // batch: (s + 1) offsets in points; NULL for the single entry
    const void *vol;             // single entry
    const void *const *vols;     // batch
    float *poses, *stats, *trace;
    float bbox_min, stride, band;
    int n, res, iters;
};

constexpr int tri(int k, int l) { return k * 6 - k * (k - 1) / 2 + (l - k); }  // k <= l: row-wise upper triangle, 21 entries

// steps 1-7 for one point, added into the lane's 29 sums
template <bool F16>
__device__ __forceinline__ void add_point(const Args &A, const void *vol, float px, float py, float pz, const float *R, const float *t,
                                          float *acc) {
    float q[3];
    to_object_frame(px, py, pz, t, R, q[0], q[1], q[2]);
    const float top = (float)(A.res - 1);
    float f[3];
    int i[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = (q[a] - A.bbox_min) / A.stride;
        inside = inside && u > 0.f && u < top;
        i[a] = cell_split(fminf(fmaxf(u, 0.f), top), f[a]);  // a NaN gives 0: every index formed lies in [0, res^3)
    }
    float d[8], c[4];
    ld_corner_cell<F16>(vol, cell_index(i[0], i[1], i[2], A.res), d);
    const float x = f[0], y = f[1], mx = 1.f - x, my = 1.f - y;
    const float r0 = cell_blend(d, x, y, f[2], c), c00 = c[0], c01 = c[1], c10 = c[2], c11 = c[3];
    float g[3];
    g[0] = ((c10 - c00) * my + (c11 - c01) * y) / A.stride;
    g[1] = ((c01 - c00) * mx + (c11 - c10) * x) / A.stride;
    g[2] = (((d[1] - d[0]) * my + (d[3] - d[2]) * y) * mx + ((d[5] - d[4]) * my + (d[7] - d[6]) * y) * x) / A.stride;
    float J[6];
    J[0] = g[1] * q[2] - g[2] * q[1];
    J[1] = g[2] * q[0] - g[0] * q[2];
    J[2] = g[0] * q[1] - g[1] * q[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) J[3 + k] = -__builtin_fmaf(R[3 * k + 2], g[2], __builtin_fmaf(R[3 * k + 1], g[1], R[3 * k] * g[0]));
    const float a = fabsf(r0), knee = A.band * 0.5f;
    const bool valid = inside && a < A.band;
    const float w = valid ? (a <= knee ? 1.f : knee / a) : 0.f;
    const float r = valid ? r0 : 0.f;
    float v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        J[k] = valid ? J[k] : 0.f;
        v[k] = w * J[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int l = k; l < 6; ++l) acc[tri(k, l)] += v[k] * J[l];
        acc[21 + k] += v[k] * r;
    }
    acc[27] += (w * r) * r;
    acc[28] += valid ? 1.f : 0.f;
}

// step 9's solve: (A + lambda diag A + eps_n I) delta = -b.  false: a pivot that is not positive, a delta that is not finite, or a
// step whose predicted gain -b . delta is below kMinGain of the accepted sum E (converged)
__device__ __forceinline__ bool solve6(const float *S, float lambda, float eps_n, float e_acc, float *delta) {
    float L[21];  // L_ik (i >= k) at tri(k, i)
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float s = __builtin_fmaf(lambda, S[tri(k, k)], S[tri(k, k)]) + eps_n;
#pragma unroll
        for (int m = 0; m < k; ++m) s -= L[tri(m, k)] * L[tri(m, k)];
        ok = ok && s > 0.f;
        const float p = sqrtf(s);
        L[tri(k, k)] = p;
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            float e = S[tri(k, i)];
#pragma unroll
            for (int m = 0; m < k; ++m) e -= L[tri(m, i)] * L[tri(m, k)];
            L[tri(k, i)] = e / p;
        }
    }
    float y[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float e = -S[21 + k];
#pragma unroll
        for (int m = 0; m < k; ++m) e -= L[tri(m, k)] * y[m];
        y[k] = e / L[tri(k, k)];
    }
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        float e = y[k];
#pragma unroll
        for (int m = k + 1; m < 6; ++m) e -= L[tri(k, m)] * delta[m];
        delta[k] = e / L[tri(k, k)];
    }
    float gain = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        ok = ok && fabsf(delta[k]) < __builtin_inff();
        gain -= S[21 + k] * delta[k];
    }
    return ok && gain >= kMinGain * e_acc;
}

// step 9's update: pose' = (ortho6d(R exp([o]x)), t + dt)
__device__ __forceinline__ void apply_step(const float *P, const float *delta, float *out) {
    const float o0 = delta[0], o1 = delta[1], o2 = delta[2];
    const float th2 = __builtin_fmaf(o2, o2, __builtin_fmaf(o1, o1, o0 * o0)), th = sqrtf(th2);
    const bool small = th2 < 1e-6f;
    const float ths = small ? 1.f : th, th2s = small ? 1.f : th2;  // (no division by zero on the branch not taken)
    const float h = sinf(0.5f * ths);
    const float sa = small ? 1.f - th2 / 6.f : sinf(ths) / ths;
    const float ca = small ? 0.5f - th2 / 24.f : 2.f * h * h / th2s;
    const float dg = 1.f - ca * th2, c0 = ca * o0, c1 = ca * o1, c2 = ca * o2;
    float dR[9];
    dR[0] = dg + c0 * o0;               dR[1] = c0 * o1 + sa * (-o2);     dR[2] = c0 * o2 + sa * o1;
    dR[3] = c1 * o0 + sa * o2;          dR[4] = dg + c1 * o1;             dR[5] = c1 * o2 + sa * (-o0);
    dR[6] = c2 * o0 + sa * (-o1);       dR[7] = c2 * o1 + sa * o0;        dR[8] = dg + c2 * o2;
    float Rn[9];
    mat3_mul(P, dR, Rn);
    float x[3] = {Rn[0], Rn[1], Rn[2]}, yr[3] = {Rn[3], Rn[4], Rn[5]}, z[3], y[3];
    normalize3(x);
    z[0] = x[1] * yr[2] - x[2] * yr[1]; z[1] = x[2] * yr[0] - x[0] * yr[2]; z[2] = x[0] * yr[1] - x[1] * yr[0];
    normalize3(z);
    y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = x[k];
        out[3 + k] = y[k];
        out[6 + k] = z[k];
        out[9 + k] = P[9 + k] + delta[3 + k];
    }
}

// One problem: its n points at pcld, its volume, its pose / stats / trace records.  Shared by both kernels, so a problem of a batch
// has the bits of the single entry.
template <bool F16>
__device__ __forceinline__ void refine_problem(const Args &A, int n, const float *__restrict__ pcld, const void *vol, float *pose,
                                               float *stats, float *trace) {
    __shared__ float red[kWaves][kSums + 3];
    __shared__ float cand[12];
    const int tid = threadIdx.x;
    if (tid < 12) cand[tid] = pose[tid];
    __syncthreads();
    // lane 0's state
    float P[12], S[27], lambda = kLambda0, c_acc = 0.f, n_acc = 0.f, c_0 = 0.f, n_0 = 0.f, steps = 0.f;
    bool stepped = false;
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) S[k] = 0.f;
    for (int it = 0; it <= A.iters; ++it) {
        float C[12], acc[kSums];
#pragma unroll
        for (int k = 0; k < 12; ++k) C[k] = cand[k];
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = 0.f;
        for (int j = tid; j < n; j += kLanes) add_point<F16>(A, vol, pcld[3 * (size_t)j], pcld[3 * (size_t)j + 1], pcld[3 * (size_t)j + 2], C, C + 9, acc);
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] = wave_sum_xor(acc[k]);
        if ((tid & (kWave - 1)) == 0) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) red[tid / kWave][k] = acc[k];
        }
        __syncthreads();
        if (tid == 0) {
            float T[kSums];
#pragma unroll
            for (int k = 0; k < kSums; ++k) {
                float s = red[0][k];
#pragma unroll
                for (int wv = 1; wv < kWaves; ++wv) s += red[wv][k];
                T[k] = s;
            }
            const float cnt = T[28], cost = T[27] / fmaxf(cnt, 1.f);
            const bool first = it == 0;
            const bool accept = first || (stepped && cost <= c_acc && cnt >= 0.5f * n_acc);
            if (stepped) lambda = accept ? fmaxf(lambda / 3.f, kLambdaMin) : fminf(lambda * 10.f, kLambdaMax);
            steps += (stepped && accept) ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 12; ++k) P[k] = accept ? C[k] : P[k];
#pragma unroll
            for (int k = 0; k < 27; ++k) S[k] = accept ? T[k] : S[k];
            c_acc = accept ? cost : c_acc;
            n_acc = accept ? cnt : n_acc;
            c_0 = first ? cost : c_0;
            n_0 = first ? cnt : n_0;
            const bool decided = stepped;
            const float lambda_solve = lambda;
            float delta[6], next[12];
            bool ok = false;
#pragma unroll
            for (int k = 0; k < 6; ++k) delta[k] = 0.f;
            if (it < A.iters) {  // (uniform: the last pass takes no step)
                ok = solve6(S, lambda, kEps * fmaxf(n_acc, 1.f), c_acc * fmaxf(n_acc, 1.f), delta) && n_acc >= 6.f;
                apply_step(P, delta, next);
                lambda = ok ? lambda : fminf(lambda * 10.f, kLambdaMax);
                stepped = ok;
#pragma unroll
                for (int k = 0; k < 12; ++k) cand[k] = ok ? next[k] : P[k];
            }
            if (trace) {
                float *row = trace + (size_t)it * kTraceRow;
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    row[k] = P[k];
                    row[16 + k] = C[k];
                }
                row[12] = lambda; row[13] = c_acc; row[14] = n_acc; row[15] = accept ? 1.f : 0.f;
#pragma unroll
                for (int k = 0; k < 27; ++k) row[28 + k] = T[k];
                row[55] = cost; row[56] = cnt; row[57] = lambda_solve; row[58] = ok ? 1.f : 0.f; row[59] = decided ? 1.f : 0.f;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    row[60 + k] = ok ? delta[k] : 0.f;
                    row[66 + k] = 0.f;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = P[k];
        stats[0] = c_0; stats[1] = c_acc; stats[2] = n_0; stats[3] = n_acc; stats[4] = steps; stats[5] = lambda; stats[6] = 0.f; stats[7] = 0.f;
    }
}

template <bool F16>
__global__ __launch_bounds__(kLanes) void sdf_refine_kernel(const Args A) {
    const int k = blockIdx.x;
    int n = A.n;
    const float *pcld = A.pcld;
    const void *vol = A.vol;
    if (A.cloud_off && !problem_slice(A.cloud_off, A.vols, k, pcld, n, vol)) return;  // inactive: pose, stats and trace keep every byte
    refine_problem<F16>(A, n, pcld, vol, A.poses + 12 * (size_t)k, A.stats + 8 * (size_t)k,
                        A.trace ? A.trace + (size_t)k * (A.iters + 1) * kTraceRow : nullptr);
}

}  // namespace refine
}  // namespace pn2

using namespace pn2;
using namespace pn2::refine;

static_assert(sizeof(pn2s_refine) == 88, "record layout (pn2_sdf.h)");

static int refine_launch(const pn2s_refine &r, bool batch, void *stream) {
    Faults f;
    f.inval = r.problems < 0 || (!batch && (r.problems != 1 || r.n < 1)) || r.iters < 0 || r.res < 2 || (r.vol_fmt != 2 && r.vol_fmt != 3);
    f.inval |= !finite_positive(r.stride) || !finite_positive(r.band) || !std::isfinite(r.bbox_min);
    f.range = r.iters > kMaxIters || r.res > 1024 || r.problems > PN2S_REFINE_BATCH_MAX;
    if (f.code() != PN2_OK) return f.code();
    if (r.problems == 0) return PN2_OK;
    f.null = !r.pcld || !r.poses || !r.stats || (batch ? (!r.cloud_off || !r.vols) : !r.volume);
    if (f.code() != PN2_OK) return f.code();
    Args A;
    A.pcld = r.pcld; A.cloud_off = batch ? r.cloud_off : nullptr; A.vol = batch ? nullptr : r.volume; A.vols = batch ? r.vols : nullptr;
    A.poses = r.poses; A.stats = r.stats; A.trace = r.trace;
    A.bbox_min = r.bbox_min; A.stride = r.stride; A.band = r.band; A.n = r.n; A.res = r.res; A.iters = r.iters;
    hipStream_t st = (hipStream_t)stream;
    if (r.vol_fmt == 3) hipLaunchKernelGGL((sdf_refine_kernel<true>), dim3(r.problems), dim3(kLanes), 0, st, A);
    else hipLaunchKernelGGL((sdf_refine_kernel<false>), dim3(r.problems), dim3(kLanes), 0, st, A);
    return check_launch();
}

extern "C" int pn2s_obj_refine(const pn2s_refine *refine, void *stream) {
    if (!refine) return PN2_ENULL;
    return refine_launch(*refine, false, stream);
}

extern "C" int pn2s_obj_refine_batch(const pn2s_refine *refine, void *stream) {
    if (!refine) return PN2_ENULL;
    return refine_launch(*refine, true, stream);
}
