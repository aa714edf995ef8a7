// tail.hip -- the 21-token tail of HandTrackNet (hand_network.py:139-147 with attn=False): after the keypoint
// branches only LayerNorms, two small FFNs and the 3-channel head remain.  On the GPU each torch op there is a
// launch-bound ~5 us kernel over a few KB; these kernels fuse the element-wise runs between the GEMMs:
//   add_layernorm : out = LN2( LN1( x + y + bias ) )      (residual add + bias + one or two LayerNorms, 1 launch)
//   perm_sum_rows / add_layernorm_perm : rearrange_module's five-slot neighbour sum taken after its product (no gathered
//                   (tokens x 5C) operand), alone or as the x operand of add_layernorm; add_layernorm_perm has an instance
//                   with the slot count at compile time (5) next to the run-time loop, same bits
//   pose_head     : delta = h W^T + b ; kp_hand = delta + xyz1 ; kp_cam = (kp_hand R^T) * scale + t   (1 launch for
//                   the reference's Conv1d(…,3,1) + add + matmul + mul + add, hand_network.py:141-147)
// The LayerNorm kernels are one wave per row and a few KB per launch: their time is the chain of dependent memory round trips,
// not bandwidth.  So a row's loads (operands, bias, both LayerNorms' affine constants) are all requested before the first add,
// and nothing is loaded inside a branch: a load that only a branch uses is issued there, one at a time behind a wait.
#include "pn2_common.h"
#include "../../include/pn2_ext.h"

namespace pn2 {

__device__ __forceinline__ float wave_sum(float v) { return wave_sum_f32(v); }  // DPP ladder, no ds_bpermute round trips

// The affine constants of both LayerNorms for this lane's channels.  They depend on nothing the row computes, so the kernels
// request them together with the row's own loads, before the first reduction: the 4-byte loads of a lane used to be issued one
// at a time, each behind a wait, after the second wave_sum (a memory round trip per element on a one-wave latency chain).
// Loads of channels beyond c read channel 0 instead (always there, c >= 1), an absent operand reads a present one, and neither
// is used: no branch around a load.
template <int EPL>
struct LnAffine {
    float g1[EPL], b1[EPL], g2[EPL], b2[EPL];
};

template <int EPL>
__device__ __forceinline__ void load_affine(LnAffine<EPL> &a, int lane, int c, const float *__restrict__ g1,
                                            const float *__restrict__ b1, const float *__restrict__ g2,
                                            const float *__restrict__ b2) {
    const float *__restrict__ g2s = g2 ? g2 : g1, *__restrict__ b2s = g2 ? b2 : b1;  // no second LayerNorm: loaded, never used
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int ch = lane + 64 * e, cs = ch < c ? ch : 0;
        a.g1[e] = g1[cs];
        a.b1[e] = b1[cs];
        a.g2[e] = g2s[cs];
        a.b2[e] = b2s[cs];
    }
    // The second LayerNorm is a branch of layernorm_row, and hipcc moves loads that only a branch uses into it (behind both
    // reductions again).  An empty statement that names the values keeps the loads here.
#pragma unroll
    for (int e = 0; e < EPL; ++e) asm volatile("" : "+v"(a.g2[e]), "+v"(a.b2[e]));
}

// The normalisation of one row held as v[e] = element lane + 64 e (0 beyond c), s = this lane's sum of them: LN1, the optional
// LN2 straight after it (TransT.s11 -> c11.norm1; has_ln2), and the store.  torch.nn.functional.layer_norm semantics: biased
// variance, eps inside the sqrt.  Shared by add_layernorm_kernel and add_layernorm_perm_kernel, which differ only in how they form v.
template <int EPL>
__device__ __forceinline__ void layernorm_row(float (&v)[EPL], float s, int lane, int c, const LnAffine<EPL> &a, float eps1,
                                              bool has_ln2, float eps2, float *__restrict__ out_row) {
    const float inv_c = 1.0f / (float)c;
    float mean = wave_sum(s) * inv_c, q = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const float d = (lane + 64 * e < c) ? v[e] - mean : 0.f;
        q += d * d;
    }
    float rstd = rsqrtf(wave_sum(q) * inv_c + eps1);
    s = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int ch = lane + 64 * e;
        v[e] = ch < c ? (v[e] - mean) * rstd * a.g1[e] + a.b1[e] : 0.f;
        s += v[e];
    }
    if (has_ln2) {  // a second LayerNorm straight after the first (TransT.s11 -> c11.norm1)
        mean = wave_sum(s) * inv_c;
        q = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const float d = (lane + 64 * e < c) ? v[e] - mean : 0.f;
            q += d * d;
        }
        rstd = rsqrtf(wave_sum(q) * inv_c + eps2);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int ch = lane + 64 * e;
            if (ch < c) v[e] = (v[e] - mean) * rstd * a.g2[e] + a.b2[e];
        }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int ch = lane + 64 * e;
        if (ch < c) out_row[ch] = v[e];
    }
}

// One wave per row; C <= 64 * EPL.  Every load of the row (x, y, bias, the affine constants) is requested before the first add.
template <int EPL>
__global__ void __launch_bounds__(256)
add_layernorm_kernel(long rows, int c, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ bias,
                     const float *__restrict__ g1, const float *__restrict__ b1, float eps1, const float *__restrict__ g2,
                     const float *__restrict__ b2, float eps2, float *__restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ ys = y ? y : x, *__restrict__ bs = bias ? bias : g1;
    float v[EPL], ty[EPL], tb[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int ch = lane + 64 * e, cs = ch < c ? ch : 0;
        v[e] = x[row * c + cs];
        ty[e] = ys[row * c + cs];
        tb[e] = bs[cs];
    }
    LnAffine<EPL> a;
    load_affine<EPL>(a, lane, c, g1, b1, g2, b2);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        float t = v[e];  // selects, no branches: a branch would take its operand's load (and the wait for it) inside
        t = y ? t + ty[e] : t;
        t = bias ? t + tb[e] : t;
        t = (lane + 64 * e < c) ? t : 0.f;
        v[e] = t;
        s += t;
    }
    layernorm_row<EPL>(v, s, lane, c, a, eps1, g2 != nullptr, eps2, out + row * c);
}

// rearrange_module's neighbour table (j tokens x re slots, entries < j), carried in the kernel arguments: the entries are
// range-checked on the host while they are packed, and a captured graph keeps its own copy.
constexpr int kPermMaxTokens = 256, kPermMaxEntries = 512;
constexpr int kPermFixedSlots = 5;  // rearrange_module's slot count: add_layernorm_perm_kernel's compile-time instance
struct PermTable {
    unsigned char p[kPermMaxEntries];
};

// out[b,t,:] = sum_r z[b, perm[t,r], r*c : (r+1)*c], r = 0 .. re-1 in that order: the five-slot sum of rearrange_module taken
// AFTER the product with the stacked slot weights (z = tokens x [W_0 | .. | W_re-1]^T, row stride ldz), so the (rows x re*c)
// gathered operand never exists.  One wave per token, one 16-byte load per slot and quad of channels.
__global__ void __launch_bounds__(256)
perm_sum_rows_kernel(long rows, int j, int re, int c4, const float *__restrict__ z, int ldz, PermTable tab, float *__restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long base = (row / j) * j;
    const unsigned char *__restrict__ p = tab.p + (int)(row - base) * re;
    for (int q = lane; q < c4; q += 64) {
        float4 a = reinterpret_cast<const float4 *>(z + (base + p[0]) * ldz)[q];
        for (int r = 1; r < re; ++r) {
            const float4 t = reinterpret_cast<const float4 *>(z + (base + p[r]) * ldz + (long)r * 4 * c4)[q];
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
        reinterpret_cast<float4 *>(out + row * 4 * c4)[q] = a;
    }
}

// add_layernorm_kernel with its x operand replaced by that sum (+ bias): out = LN2( LN1( sum_r z[..] + bias ) ), summed as
// ((((0 + z_0) + z_1) + ..) + z_re-1) + bias.  RE > 0: the slot count is a compile-time value (the network's 5), so the RE table
// bytes are read once per wave and all RE * EPL slice loads, the bias and the affine constants are requested before the first
// add.  RE = 0: any slot count, one slice after the other (the loads of a slice wait for the slice before).  Same sums in the
// same order, so both give the same bits.
template <int EPL, int RE>
__global__ void __launch_bounds__(256)
add_layernorm_perm_kernel(long rows, int j, int re, int c, const float *__restrict__ z, int ldz, PermTable tab,
                          const float *__restrict__ bias, const float *__restrict__ g1, const float *__restrict__ b1, float eps1,
                          const float *__restrict__ g2, const float *__restrict__ b2, float eps2, float *__restrict__ out) {
    // the row is the wave's: said to the compiler, so that the table bytes and the slice bases are scalar
    const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long base = (row / j) * j;
    const unsigned char *__restrict__ p = tab.p + (int)(row - base) * (RE ? RE : re);
    float v[EPL];
    LnAffine<EPL> a;
    if constexpr (RE > 0) {
        const float *zr[RE];
#pragma unroll
        for (int r = 0; r < RE; ++r) zr[r] = z + (base + p[r]) * ldz + (long)r * c;
        const float *__restrict__ bs = bias ? bias : g1;
        float t[RE][EPL], tb[EPL];
#pragma unroll
        for (int r = 0; r < RE; ++r) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int ch = lane + 64 * e;
                t[r][e] = zr[r][ch < c ? ch : 0];
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int ch = lane + 64 * e;
            tb[e] = bs[ch < c ? ch : 0];
        }
        load_affine<EPL>(a, lane, c, g1, b1, g2, b2);
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            float u = 0.f;  // selects, no branches: a branch would take its operand's load (and the wait for it) inside
#pragma unroll
            for (int r = 0; r < RE; ++r) u += t[r][e];
            u = bias ? u + tb[e] : u;
            v[e] = (lane + 64 * e < c) ? u : 0.f;
        }
    } else {
        load_affine<EPL>(a, lane, c, g1, b1, g2, b2);
#pragma unroll
        for (int e = 0; e < EPL; ++e) v[e] = 0.f;
        for (int r = 0; r < re; ++r) {
            const float *__restrict__ zr = z + (base + p[r]) * ldz + (long)r * c;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int ch = lane + 64 * e;
                if (ch < c) v[e] += zr[ch];
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int ch = lane + 64 * e;
            if (bias && ch < c) v[e] += bias[ch];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) s += v[e];
    layernorm_row<EPL>(v, s, lane, c, a, eps1, g2 != nullptr, eps2, out + row * c);
}

// Packs a host (j, re) int32 table into the kernel-argument form; PN2_EINVAL when it does not fit or an entry is outside [0, j).
static int pack_perm(int j, int re, const int *perm, PermTable &tab) {
    if (j < 1 || re < 1 || j > kPermMaxTokens || j * re > kPermMaxEntries) return PN2_EINVAL;
    for (int i = 0; i < j * re; ++i) {
        if (perm[i] < 0 || perm[i] >= j) return PN2_EINVAL;
        tab.p[i] = (unsigned char)perm[i];
    }
    return PN2_OK;
}

// One wave per token (b, j): three dot products of length c, then the rigid transform back to the camera frame.
__global__ void __launch_bounds__(256)
pose_head_kernel(int tokens, int j, int c, const float *__restrict__ h, const float *__restrict__ w, const float *__restrict__ bias,
                 const float *__restrict__ xyz1, const float *__restrict__ R, const float *__restrict__ t, float scale,
                 float *__restrict__ kp_hand, float *__restrict__ kp_cam, const int *__restrict__ nonfinite) {
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= tokens) return;
    const int lane = threadIdx.x & 63;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int ch = lane; ch < c; ch += 64) {
        const float hv = h[(size_t)tok * c + ch];
        a0 = fmaf(hv, w[ch], a0);
        a1 = fmaf(hv, w[c + ch], a1);
        a2 = fmaf(hv, w[2 * c + ch], a2);
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane == 0) {
        const int b = tok / j;
        float px = a0 + bias[0] + xyz1[3 * tok], py = a1 + bias[1] + xyz1[3 * tok + 1], pz = a2 + bias[2] + xyz1[3 * tok + 2];
        if (nonfinite && nonfinite[b]) px = py = pz = __builtin_nanf("");  // flagged by pn2x_hand_frame: non-finite input frame
        kp_hand[3 * tok] = px; kp_hand[3 * tok + 1] = py; kp_hand[3 * tok + 2] = pz;
        const float *Rb = R + 9 * b, *tb = t + 3 * b;
        // row vector times R^T: out_i = sum_k p_k R[i][k]
        kp_cam[3 * tok] = (px * Rb[0] + py * Rb[1] + pz * Rb[2]) * scale + tb[0];
        kp_cam[3 * tok + 1] = (px * Rb[3] + py * Rb[4] + pz * Rb[5]) * scale + tb[1];
        kp_cam[3 * tok + 2] = (px * Rb[6] + py * Rb[7] + pz * Rb[8]) * scale + tb[2];
    }
}

}  // namespace pn2

using namespace pn2;

extern "C" int pn2x_add_layernorm(long rows, int c, const float *x, const float *y, const float *bias, const float *g1,
                                  const float *b1, float eps1, const float *g2, const float *b2, float eps2, float *out,
                                  void *stream) {
    if (rows < 0 || c < 1 || c > 1024) return PN2_EINVAL;
    if (rows == 0) return PN2_OK;
    if (!x || !g1 || !b1 || !out || ((g2 == nullptr) != (b2 == nullptr))) return PN2_ENULL;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    hipStream_t st = (hipStream_t)stream;
#define PN2_LN(E) hipLaunchKernelGGL(add_layernorm_kernel<E>, dim3(blocks), dim3(256), 0, st, rows, c, x, y, bias, g1, b1, eps1, g2, b2, eps2, out)
    if (c <= 128) PN2_LN(2);
    else if (c <= 256) PN2_LN(4);
    else if (c <= 512) PN2_LN(8);
    else PN2_LN(16);
#undef PN2_LN
    return check_launch();
}

extern "C" int pn2x_perm_sum_rows(int b, int j, int re, int c, const float *z, int ldz, const int *perm, float *out, void *stream) {
    if (b < 0 || c < 1 || (c & 3) || ldz < 0 || (ldz & 3) || (long)ldz < (long)re * c) return PN2_EINVAL;
    if (!perm) return PN2_ENULL;
    PermTable tab;
    if (const int rc = pack_perm(j, re, perm, tab)) return rc;
    if (b == 0) return PN2_OK;
    if (!z || !out) return PN2_ENULL;
    if ((((uintptr_t)z | (uintptr_t)out) & 15) != 0) return PN2_EINVAL;  // 16-byte loads and stores
    const long rows = (long)b * j;
    hipLaunchKernelGGL(perm_sum_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows, j, re, c / 4, z,
                       ldz, tab, out);
    return check_launch();
}

// fixed_slots: launch the compile-time-slot instance where there is one for `re` (kPermFixedSlots).
static int add_layernorm_perm_launch(bool fixed_slots, int b, int j, int re, int c, const float *z, int ldz, const int *perm,
                                     const float *bias, const float *g1, const float *b1, float eps1, const float *g2,
                                     const float *b2, float eps2, float *out, void *stream) {
    if (b < 0 || c < 1 || c > 1024 || (c & 3) || ldz < 0 || (long)ldz < (long)re * c) return PN2_EINVAL;
    if (!perm) return PN2_ENULL;
    PermTable tab;
    if (const int rc = pack_perm(j, re, perm, tab)) return rc;
    if (b == 0) return PN2_OK;
    if (!z || !g1 || !b1 || !out || ((g2 == nullptr) != (b2 == nullptr))) return PN2_ENULL;
    const long rows = (long)b * j;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    hipStream_t st = (hipStream_t)stream;
#define PN2_LNP(E, R) hipLaunchKernelGGL((add_layernorm_perm_kernel<E, R>), dim3(blocks), dim3(256), 0, st, rows, j, re, c, z, ldz, tab, bias, g1, b1, eps1, g2, b2, eps2, out)
    if (fixed_slots && re == kPermFixedSlots) {
        if (c <= 128) PN2_LNP(2, kPermFixedSlots);
        else if (c <= 256) PN2_LNP(4, kPermFixedSlots);
        else if (c <= 512) PN2_LNP(8, kPermFixedSlots);
        else PN2_LNP(16, kPermFixedSlots);
    } else {
        if (c <= 128) PN2_LNP(2, 0);
        else if (c <= 256) PN2_LNP(4, 0);
        else if (c <= 512) PN2_LNP(8, 0);
        else PN2_LNP(16, 0);
    }
#undef PN2_LNP
    return check_launch();
}

extern "C" int pn2x_add_layernorm_perm(int b, int j, int re, int c, const float *z, int ldz, const int *perm, const float *bias,
                                       const float *g1, const float *b1, float eps1, const float *g2, const float *b2, float eps2,
                                       float *out, void *stream) {
    return add_layernorm_perm_launch(true, b, j, re, c, z, ldz, perm, bias, g1, b1, eps1, g2, b2, eps2, out, stream);
}

extern "C" int pn2x_add_layernorm_perm_any_slots(int b, int j, int re, int c, const float *z, int ldz, const int *perm,
                                                 const float *bias, const float *g1, const float *b1, float eps1, const float *g2,
                                                 const float *b2, float eps2, float *out, void *stream) {
    return add_layernorm_perm_launch(false, b, j, re, c, z, ldz, perm, bias, g1, b1, eps1, g2, b2, eps2, out, stream);
}

extern "C" int pn2x_pose_head(int b, int j, int c, const float *h, const float *w, const float *bias, const float *xyz1,
                               const float *R, const float *t, float scale, float *kp_hand, float *kp_cam, const int *nonfinite,
                               void *stream) {
    if (b < 0 || j < 1 || c < 1) return PN2_EINVAL;
    if (b == 0) return PN2_OK;
    if (!h || !w || !bias || !xyz1 || !R || !t || !kp_hand || !kp_cam) return PN2_ENULL;
    const int tokens = b * j;
    hipLaunchKernelGGL(pose_head_kernel, dim3((tokens + 3) / 4), dim3(256), 0, (hipStream_t)stream, tokens, j, c, h, w, bias, xyz1,
                       R, t, scale, kp_hand, kp_cam, nonfinite);
    return check_launch();
}
