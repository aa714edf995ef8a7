// mid_chain.hip -- sa3 and fp3 of the backbone as row-tiled layer chains on the fp32 matrix cores (eval fast path,
// network/models/fast_eval.py, large batches).
//
// sa3 (group-all) and fp3 run over the B * S level-2 rows (S = 128 per cloud):
//
//   x = sa3_in[r] = [l2_feat | l2_xyz | pad]                                 (132 floats)
//   sa3:  h1 = relu(W1 x[:131] + b1), h2 = relu(W2 h1 + b2), y = relu(W3 h2 + b3)        131 -> 128 -> 128 -> 512
//         l3[b] = max over the cloud's rows of y
//   fp3:  g[b] = Wg l3[b] + bg                                                (the per-cloud half of fp3's layer 1)
//         h = relu(Wa x[:128] + g[b]), l2_out[r] = relu(Wf h + bf)            128 -> 256 -> 256
//
// A workgroup runs one tile of 32 rows of one cloud (S is a multiple of 32, so a tile never spans two clouds) with the
// activations in LDS and the weights streamed from L2 (mfma_rows.h).  sa3's last layer never goes to LDS: the max over
// the tile's rows is taken on the accumulators (across the m-tiles in registers, then across the 16 lanes of a row group)
// and each tile writes its partial maximum; fp3's tiles take the max of their cloud's partials and compute g themselves.
// No atomics, no inter-workgroup waits: the results do not depend on the order in which tiles run.
#include "pn2_common.h"
#include "mfma_rows.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace mchain {

using mrows::f32x4;
using mrows::init_bias;
using mrows::mm;
using mrows::relu_to_lds;

constexpr int MT = 2, TR = 16 * MT;       // m-tiles and rows per tile: B * S / 32 tiles (256 at the bench batch) fill the chip
constexpr int CL2 = 128, CL3 = 512;       // l2_feat width, sa3's output width
constexpr int C1 = 128, C2 = 128;         // sa3 hidden widths
constexpr int CF = 256;                   // fp3 widths
constexpr int KX = 144;                   // sa3 layer 1: 128 features + 3 coordinates, zero-padded to 9 k-groups of 16
constexpr int XQ = 33;                    // 16-byte quads of an input row that hold data (132 floats)
constexpr int LDX = 152, LDH = 136, LDF = 264;  // LDS row strides, = 8 (mod 64)

constexpr size_t SA3_LDS = (size_t)TR * (LDX + LDH) * sizeof(float);
constexpr size_t FP3_LDS = (size_t)(TR * (LDH + LDF) + CL3 + 4 * CF + CF) * sizeof(float);

// max over the 16 lanes of each DPP row; every lane of the row ends with it
__device__ __forceinline__ float row16_max(float v) {
    PN2_DPP_STEP("v_max_f32_dpp", v, "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf");
    PN2_DPP_STEP("v_max_f32_dpp", v, "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf");
    PN2_DPP_STEP("v_max_f32_dpp", v, "row_half_mirror row_mask:0xf bank_mask:0xf");
    PN2_DPP_STEP("v_max_f32_dpp", v, "row_mirror row_mask:0xf bank_mask:0xf");
    return v;
}

__global__ __launch_bounds__(256) void sa3_chain_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ w1,
                                                        const float *__restrict__ b1, const float *__restrict__ w2,
                                                        const float *__restrict__ b2, const float *__restrict__ w3,
                                                        const float *__restrict__ b3, float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *r1 = smem, *r2 = smem + TR * LDX;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * TR;
    // input rows -> LDS, zero past column 130 (the row's pad float may hold anything)
    for (int i = tid; i < TR * (KX / 4); i += 256) {
        const int r = i / (KX / 4), q = i - r * (KX / 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < XQ) {
            v = *reinterpret_cast<const f32x4 *>(x + (row0 + r) * ldx + 4 * q);
            if (q == XQ - 1) v.w = 0.f;
        }
        *reinterpret_cast<f32x4 *>(r1 + r * LDX + 4 * q) = v;
    }
    __syncthreads();
    {  // layer 1: 144 -> 128, two n-tiles per wave
        f32x4 acc[2][MT];
        init_bias(acc, b1, 2 * w, lane);
        mm<2, MT, KX / 16, LDX>(acc, w1 + (size_t)(2 * w) * (KX / 16) * 256, r1, lane);
        relu_to_lds(acc, r2, LDH, 2 * w, lane);
    }
    __syncthreads();
    {  // layer 2: 128 -> 128
        f32x4 acc[2][MT];
        init_bias(acc, b2, 2 * w, lane);
        mm<2, MT, C1 / 16, LDH>(acc, w2 + (size_t)(2 * w) * (C1 / 16) * 256, r2, lane);
        relu_to_lds(acc, r1, LDH, 2 * w, lane);
    }
    __syncthreads();
    // layer 3: 128 -> 512, 32 n-tiles = 2 passes x 4 waves x 4, reduced to the tile's maximum on the accumulators.
    // relu(max) == max(relu): the ReLU is applied once, to the maximum.
    float *dst = part + (size_t)blockIdx.x * CL3 + 4 * (lane >> 4);
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {
        const int nt0 = (p * 4 + w) * 4;
        f32x4 acc[4][MT];
        init_bias(acc, b3, nt0, lane);
        mm<4, MT, C2 / 16, LDH>(acc, w3 + (size_t)nt0 * (C2 / 16) * 256, r1, lane);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            f32x4 m = acc[nt][0];
#pragma unroll
            for (int mt = 1; mt < MT; ++mt)
                m = (f32x4){fmaxf(m.x, acc[nt][mt].x), fmaxf(m.y, acc[nt][mt].y), fmaxf(m.z, acc[nt][mt].z), fmaxf(m.w, acc[nt][mt].w)};
            m = (f32x4){fmaxf(row16_max(m.x), 0.f), fmaxf(row16_max(m.y), 0.f), fmaxf(row16_max(m.z), 0.f), fmaxf(row16_max(m.w), 0.f)};
            if ((lane & 15) == 0) *reinterpret_cast<f32x4 *>(dst + (nt0 + nt) * 16) = m;
        }
    }
}

__global__ __launch_bounds__(256) void fp3_chain_kernel(int s, const float *__restrict__ x, int ldx, const float *__restrict__ part,
                                                        const float *__restrict__ wgt, const float *__restrict__ bg,
                                                        const float *__restrict__ wa, const float *__restrict__ wf,
                                                        const float *__restrict__ bf, float *__restrict__ out, int ldo) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *r1 = smem, *r2 = r1 + TR * LDH, *l3 = r2 + TR * LDF, *gp = l3 + CL3, *g = gp + 4 * CF;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * TR;
    const int np = s / TR;                          // partial maxima per cloud
    const int b = (int)(row0 / (size_t)s);
    for (int i = tid; i < TR * (CL2 / 4); i += 256) {  // l2_feat rows -> LDS
        const int r = i / (CL2 / 4), q = i - r * (CL2 / 4);
        *reinterpret_cast<f32x4 *>(r1 + r * LDH + 4 * q) = *reinterpret_cast<const f32x4 *>(x + (row0 + r) * ldx + 4 * q);
    }
    for (int k = tid; k < CL3; k += 256) {  // l3 of this cloud: the max of its tiles' partial maxima
        const float *pp = part + (size_t)b * np * CL3 + k;
        float m = pp[0];
        for (int i = 1; i < np; ++i) m = fmaxf(m, pp[(size_t)i * CL3]);
        l3[k] = m;
    }
    __syncthreads();
    {  // g = Wg l3 + bg: thread (kq, q) sums k in [128 kq, 128 kq + 128) for the four outputs 4q .. 4q + 3; wgt is Wg^T (512, 256)
        const int q = tid & 63, kq = tid >> 6;
        const f32x4 *wt = reinterpret_cast<const f32x4 *>(wgt) + (size_t)(kq * (CL3 / 4)) * 64 + q;
        const float *lk = l3 + kq * (CL3 / 4);
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int k = 0; k < CL3 / 4; ++k) a = __builtin_elementwise_fma(wt[(size_t)k * 64], (f32x4)lk[k], a);
        *reinterpret_cast<f32x4 *>(gp + kq * CF + 4 * q) = a;
    }
    __syncthreads();
    if (tid < CF / 4) {
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(gp) + tid;
        *reinterpret_cast<f32x4 *>(g + 4 * tid) =
            *reinterpret_cast<const f32x4 *>(bg + 4 * tid) + ((g4[0] + g4[CF / 4]) + (g4[2 * CF / 4] + g4[3 * CF / 4]));
    }
    __syncthreads();
    const int nt0 = 4 * w;  // 16 n-tiles of 256 outputs: four per wave, in both layers
    {  // h = relu(Wa x + g): 128 -> 256
        f32x4 acc[4][MT];
        init_bias(acc, g, nt0, lane);
        mm<4, MT, CL2 / 16, LDH>(acc, wa + (size_t)nt0 * (CL2 / 16) * 256, r1, lane);
        relu_to_lds(acc, r2, LDF, nt0, lane);
    }
    __syncthreads();
    {  // l2_out = relu(Wf h + bf): 256 -> 256, straight to the output rows
        f32x4 acc[4][MT];
        init_bias(acc, bf, nt0, lane);
        mm<4, MT, CF / 16, LDF>(acc, wf + (size_t)nt0 * (CF / 16) * 256, r2, lane);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            float *o = out + (row0 + mt * 16 + (lane & 15)) * ldo + nt0 * 16 + 4 * (lane >> 4);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const f32x4 v = acc[nt][mt];
                *reinterpret_cast<f32x4 *>(o + nt * 16) = (f32x4){fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
            }
        }
    }
}

inline bool misaligned16(std::initializer_list<const void *> ps) {
    uintptr_t u = 0;
    for (const void *p : ps) u |= (uintptr_t)p;
    return u % 16 != 0;
}

}  // namespace mchain
}  // namespace pn2

extern "C" int pn2x_sa3_chain_supported(int s, int c_in, int c1, int c2, int c3) {
    using namespace pn2::mchain;
    return (s > 0 && s % TR == 0 && c_in == CL2 && c1 == C1 && c2 == C2 && c3 == CL3) ? 1 : 0;
}

extern "C" int pn2x_sa3_chain(int b, int s, const float *x, int ldx, const float *w1, const float *b1, const float *w2,
                              const float *b2, const float *w3, const float *b3, float *part, void *stream) {
    using namespace pn2;
    using namespace pn2::mchain;
    if (b < 0 || s < 1 || s % TR || ldx < XQ * 4 || ldx % 4) return PN2_EINVAL;
    if ((long)b * s >= (1L << 31)) return PN2_ERANGE;
    if (b == 0) return PN2_OK;
    if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !part) return PN2_ENULL;
    if (misaligned16({x, w1, b1, w2, b2, w3, b3, part})) return PN2_EINVAL;
    static PerDeviceOnce raised;
    if (raised.first_use())
        (void)hipFuncSetAttribute((const void *)sa3_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SA3_LDS);
    hipLaunchKernelGGL(sa3_chain_kernel, dim3((unsigned)((long)b * s / TR)), dim3(256), SA3_LDS, (hipStream_t)stream, x, ldx, w1,
                       b1, w2, b2, w3, b3, part);
    return check_launch();
}

extern "C" int pn2x_fp3_chain_supported(int s, int c_l2, int c_l3, int c1, int c2) {
    using namespace pn2::mchain;
    return (s > 0 && s % TR == 0 && c_l2 == CL2 && c_l3 == CL3 && c1 == CF && c2 == CF) ? 1 : 0;
}

extern "C" int pn2x_fp3_chain(int b, int s, const float *x, int ldx, const float *part, const float *wgt, const float *bg,
                              const float *wa, const float *wf, const float *bf, float *out, int ldo, void *stream) {
    using namespace pn2;
    using namespace pn2::mchain;
    if (b < 0 || s < 1 || s % TR || ldx < CL2 || ldx % 4 || ldo < CF || ldo % 4) return PN2_EINVAL;
    if ((long)b * s >= (1L << 31)) return PN2_ERANGE;
    if (b == 0) return PN2_OK;
    if (!x || !part || !wgt || !bg || !wa || !wf || !bf || !out) return PN2_ENULL;
    if (misaligned16({x, part, wgt, bg, wa, wf, bf, out})) return PN2_EINVAL;
    static PerDeviceOnce raised;
    if (raised.first_use())
        (void)hipFuncSetAttribute((const void *)fp3_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FP3_LDS);
    hipLaunchKernelGGL(fp3_chain_kernel, dim3((unsigned)((long)b * s / TR)), dim3(256), FP3_LDS, (hipStream_t)stream, s, x, ldx,
                       part, wgt, bg, wa, wf, bf, out, ldo);
    return check_launch();
}
