// mfma_rows.h -- the fp32 matrix-core core of the row-tiled layer chains (row_chain.hip, mid_chain.hip).
//
// A chain runs consecutive per-row layers over a tile of up to 64 rows with the activations in LDS and the weights streamed
// from L2 straight into registers.  Products are transposed (D^T = W X^T on v_mfma_f32_16x16x4_f32, exact fp32), so every
// lane owns four consecutive output channels of one row: accumulator [nt][mt] of lane l holds channels
// 16 (nt0 + nt) + 4 (l / 16) + 0..3 of tile row 16 mt + l % 16, and goes to LDS / HBM as one 16-byte store.
//
// Weights: the operand layout of hotrack_amd/ext.py: row_chain_pack ((n_out, k) -> k zero-padded to a multiple of 16, then
// [n-tile][k-group][lane][4] with lane = 16 * (k quad inside the group) + (row inside the n-tile)): one wave's 16-byte loads
// of a k-group cover 1 KiB contiguously.
// LDS activations: row strides = 8 (mod 64) floats keep the 16-byte operand reads (16 rows x 4 k-quads per lane group)
// conflict-free.
#pragma once
#include <hip/hip_runtime.h>

namespace pn2 {
namespace mrows {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// acc[nt][mt] += W[tile nt] . X[rows of m-tile mt]^T over KG k-groups of 16, k-groups and the four k-steps of each in
// ascending order.  wp: packed weights of the first n-tile ([n-tile][k-group][lane][4], KG k-groups per n-tile); xs: LDS
// rows, ld floats apart.  Lane l supplies, in k-step s of a k-group, W[n0 + l%16][16 kg + 4 (l/16) + s] and
// X[m0 + l%16][16 kg + 4 (l/16) + s]: one 16-byte load of each per k-group.
//
// Three operand slots: the loads of k-group kg + 2 (NT weight loads from L2, MT LDS reads) are issued at the top of the step
// that consumes k-group kg, one load per MFMA (sched_group_barrier pins that order; left to itself hipcc issued a slot's
// loads a few MFMAs before the step that needs them and waited vmcnt(0) there, with one wave per SIMD and nothing else to
// issue).  A step waits only for operands requested two steps earlier, and the loads of kg + 1 and kg + 2 stay in flight
// behind it: vmcnt reaches 0 only in the last step of a layer.
template <int NT, int MT, int KG, int LD>
__device__ __forceinline__ void mm(f32x4 (&acc)[NT][MT], const float *__restrict__ wp, const float *xs, int lane) {
    static_assert(KG >= 5, "the pipeline is two k-groups deep");
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(wp) + lane;
    const float *xr = xs + (lane & 15) * LD + 4 * (lane >> 4);
    f32x4 w[3][NT], x[3][MT];
    auto load = [&](int kg, int slot) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) w[slot][nt] = w4[(nt * KG + kg) * 64];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) x[slot][mt] = *reinterpret_cast<const f32x4 *>(xr + mt * 16 * LD + 16 * kg);
    };
    auto step = [&](int slot) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[slot][nt][s], x[slot][mt][s], acc[nt][mt], 0, 0, 0);
    };
    load(0, 0);
    load(1, 1);
    constexpr int MAIN = (KG - 2) / 3;  // iterations of three steps in which every step has a k-group kg + 2 to load
#pragma unroll 1
    for (int it = 0; it < MAIN; ++it) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            load(3 * it + j + 2, (j + 2) % 3);
            step(j);
            // one load, one MFMA, ... until the NT + MT loads are out; then the rest of the step's 4 NT MT MFMAs
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT * MT - NT - MT, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int kg = 3 * MAIN; kg < KG; ++kg) {  // the last 2 .. 4 steps: nothing left to load in the last two
        if (kg + 2 < KG) load(kg + 2, (kg + 2) % 3);
        step(kg % 3);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// every accumulator of n-tile nt0 + nt starts at the bias of its four channels (bias may point to global memory or LDS)
template <int NT, int MT>
__device__ __forceinline__ void init_bias(f32x4 (&acc)[NT][MT], const float *__restrict__ bias, int nt0, int lane) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(bias + (nt0 + nt) * 16 + 4 * (lane >> 4));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = b;
    }
}

// relu(acc) -> LDS rows ld floats apart, columns of n-tiles nt0 ..
template <int NT, int MT>
__device__ __forceinline__ void relu_to_lds(const f32x4 (&acc)[NT][MT], float *dst, int ld, int nt0, int lane) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4 v = acc[nt][mt];
            *reinterpret_cast<f32x4 *>(dst + (mt * 16 + (lane & 15)) * ld + (nt0 + nt) * 16 + 4 * (lane >> 4)) =
                (f32x4){fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
        }
}

}  // namespace mrows
}  // namespace pn2
