// hand_shape.hip -- the hand shape-code search (reference gf_optimize_hand_shape.optimize, optimization_hand.py:74-124) in
// one launch.
//
// At a fixed pose a linear-blend-skinned hand with linear shape blend directions has keypoints that are affine in the shape
// code: kp(beta) = K0 + sum_d beta_d K[d] (HandModel.shape_keypoint_basis).  So are the 15 bone vectors of kp2length
// (:24-28): bone_b(beta) = B0_b + sum_d beta_d B_d,b with B = K[bone] - K[parent].  A candidate's energy is then
// 15 x 3 x D fused multiply-adds, 15 square roots and 15 T absolute differences -- no hand-model evaluation.
//
// One workgroup of 1024 threads runs all iterations: the bone basis, the target lengths, the candidates' energies and the
// iteration state live in LDS.  Per iteration:
//   pass 1: candidate p (strided over the threads) evaluates x = h + pre[p] * search and writes E[p] to LDS;
//   pass 2: with origin = E[0], every thread accumulates w = (origin - E) [E < origin], w, w E, [E < origin] and
//           w * sample_d over its candidates in index order; a butterfly over each wave and an in-order sum over the 16
//           waves' partials give the workgroup totals;
//   thread 0 applies the update (the reference's two host branches as selects) and the search-size rule.
// Every sum runs in a fixed order and there are no atomics: two runs give bitwise-equal results.  A grid-wide barrier per
// iteration would cost more than one compute unit needs for 5120 candidates, so the search stays in one workgroup.
#include "pn2_common.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace hshape {

constexpr int NT = 1024, NW = NT / 64;
constexpr int MAXD = 16, MAXP = 8192, MAXT = 1024;
constexpr int NB = 15;            // bones of kp2length
constexpr int NV = MAXD + 3;      // reduced values: w, w E, [E < origin], w * sample_d
constexpr int ST = 3 * MAXD + 4;  // iteration state: h, search, prev_search, prev_success

// kp2length's tables: bone b = 1,2,3,5,6,7,...,17,18,19 and its parent 0,1,2,0,5,6,...,0,17,18
__device__ __forceinline__ int bone_of(int b) { return 4 * (b / 3) + b % 3 + 1; }
__device__ __forceinline__ int parent_of(int b) { return b % 3 == 0 ? 0 : bone_of(b) - 1; }

inline size_t lds_bytes(int p, int t) { return (size_t)(p + t * NB + 3 * NB * (MAXD + 1) + NW * NV + NV + ST) * sizeof(float); }

__global__ __launch_bounds__(NT) void hand_shape_kernel(int P, int D, int T, int iters, const float *__restrict__ k0,
                                                        const float *__restrict__ kb, const float *__restrict__ pre,
                                                        const float *__restrict__ tgt, const float *__restrict__ init_scale,
                                                        float sc2, float beta, float one_minus_beta, float *__restrict__ out,
                                                        float *__restrict__ trace) {
    extern __shared__ float sm[];
    float *E = sm;                   // (P)
    float *L = E + P;                // (T, 15) target lengths
    float *B = L + T * NB;           // (D + 1, 15, 3): bone vectors of K0, then of K[d]
    float *red = B + 3 * NB * (MAXD + 1);  // (NW, NV) per-wave partials
    float *tot = red + NW * NV;      // (NV)
    float *h = tot + NV, *s = h + MAXD, *ps = s + MAXD, *flag = ps + MAXD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < T * NB; i += NT) L[i] = tgt[i];
    for (int i = tid; i < 3 * NB * (D + 1); i += NT) {
        const int which = i / (3 * NB), r = i % (3 * NB), b = r / 3, c = r % 3;
        const float *src = which == 0 ? k0 : kb + (which - 1) * 63;
        B[i] = src[bone_of(b) * 3 + c] - src[parent_of(b) * 3 + c];
    }
    if (tid < MAXD) {
        const float v = tid < D ? init_scale[tid] : 0.f;
        h[tid] = 0.f;
        s[tid] = v;
        ps[tid] = v;
    }
    if (tid == 0) flag[0] = 1.f;  // prev_success
    __syncthreads();

    const float inv15 = 1.f / 15.f;
    for (int it = 0; it < iters; ++it) {
        // ---- pass 1: energies ------------------------------------------------------------------------------------------------
        for (int p = tid; p < P; p += NT) {
            float x[MAXD];
#pragma unroll
            for (int d = 0; d < MAXD; ++d) x[d] = d < D ? h[d] + pre[(size_t)p * D + d] * s[d] : 0.f;
            float len[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                float v0 = B[3 * b], v1 = B[3 * b + 1], v2 = B[3 * b + 2];
#pragma unroll
                for (int d = 0; d < MAXD; ++d) {
                    if (d < D) {
                        const float *bd = B + 3 * NB * (d + 1) + 3 * b;
                        v0 = __builtin_fmaf(x[d], bd[0], v0);
                        v1 = __builtin_fmaf(x[d], bd[1], v1);
                        v2 = __builtin_fmaf(x[d], bd[2], v2);
                    }
                }
                len[b] = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
            }
            // mean over the bones, then over the targets (:55).  The sum over the targets is compensated: a plain running sum
            // of T = 1024 rows is off by some 8 ulp, which the weights origin - E of pass 2 magnify by E / (origin - E).
            float e = 0.f, lost = 0.f;
            for (int t = 0; t < T; ++t) {
                const float *lt = L + t * NB;
                float a = 0.f;
#pragma unroll
                for (int b = 0; b < NB; ++b) a += fabsf(len[b] - lt[b]);
                const float y = a * inv15 - lost, sum = e + y;
                lost = (sum - e) - y;
                e = sum;
            }
            E[p] = e / (float)T;
        }
        __syncthreads();

        // ---- pass 2: weights and weighted sums ---------------------------------------------------------------------------------
        const float origin = E[0];
        float acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.f;
        for (int p = tid; p < P; p += NT) {
            const float e = E[p];
            const bool better = e < origin;
            const float w = better ? origin - e : 0.f;
            acc[0] += w;
            acc[1] += e * w;
            acc[2] += better ? 1.f : 0.f;
#pragma unroll
            for (int d = 0; d < MAXD; ++d)
                if (d < D) acc[3 + d] += (pre[(size_t)p * D + d] * s[d]) * w;
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc[v] += __shfl_xor(acc[v], m, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) red[wave * NV + v] = acc[v];
        }
        __syncthreads();
        if (tid < NV) {
            float a = 0.f;
            for (int w = 0; w < NW; ++w) a += red[w * NV + tid];
            tot[tid] = a;
        }
        __syncthreads();

        // ---- update (:96-121, host branches as selects) ----------------------------------------------------------------------
        if (tid == 0) {
            const float wsum = tot[0];
            const bool success = tot[2] > 0.f;
            const float mean_e = success ? tot[1] / wsum : origin;
            float mt[MAXD], sn = 0.f;
#pragma unroll
            for (int d = 0; d < MAXD; ++d) {
                mt[d] = (d < D && success) ? tot[3 + d] / wsum : 0.f;
                if (d < D) {
                    h[d] = success ? h[d] + mt[d] : h[d];
                    const float sd = fabsf(mt[d]) + 1e-3f;
                    sn += sd * sd;
                }
            }
            const float nrm = sqrtf(sn);
            const bool both = flag[0] != 0.f && success;
            float *tr = trace ? trace + (size_t)it * (3 + D) : nullptr;
            if (tr) {
                tr[0] = origin;
                tr[1] = mean_e;
                tr[2] = success ? 1.f : 0.f;
            }
#pragma unroll
            for (int d = 0; d < MAXD; ++d) {
                if (d < D) {
                    const float sd = fabsf(mt[d]) + 1e-3f;
                    float ns = mean_e * sc2 * sd / nrm + 1e-3f;
                    ns = both ? beta * ns + one_minus_beta * ps[d] : ns;
                    ps[d] = success ? ns : ps[d];
                    s[d] = ns;
                    if (tr) tr[3 + d] = ns;
                }
            }
            flag[0] = success ? 1.f : 0.f;
        }
        __syncthreads();
    }
    if (tid < D) out[tid] = h[tid];
}

}  // namespace hshape
}  // namespace pn2

extern "C" int pn2x_hand_shape_opt_supported(int p, int d, int t) {
    using namespace pn2::hshape;
    return (p >= 1 && p <= MAXP && d >= 1 && d <= MAXD && t >= 1 && t <= MAXT) ? 1 : 0;
}

extern "C" int pn2x_hand_shape_opt(int p, int d, int t, int iterations, const float *k0, const float *k, const float *pre,
                                   const float *targets, const float *initial_scale, double scaling_coefficient2, double beta,
                                   float *out, float *trace, void *stream) {
    using namespace pn2;
    using namespace pn2::hshape;
    if (p < 1 || d < 1 || t < 1 || iterations < 0) return PN2_EINVAL;
    if (p > MAXP || d > MAXD || t > MAXT || (long)iterations * (3 + d) >= (1L << 31)) return PN2_ERANGE;
    if (iterations == 0) return PN2_OK;
    if (!k0 || !k || !pre || !targets || !initial_scale || !out) return PN2_ENULL;
    static PerDeviceOnce raised;
    if (raised.first_use())
        (void)hipFuncSetAttribute((const void *)hand_shape_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes(MAXP, MAXT));
    hipLaunchKernelGGL(hand_shape_kernel, dim3(1), dim3(NT), lds_bytes(p, t), (hipStream_t)stream, p, d, t, iterations, k0, k,
                       pre, targets, initial_scale, (float)scaling_coefficient2, (float)beta, (float)(1.0 - beta), out, trace);
    return check_launch();
}
