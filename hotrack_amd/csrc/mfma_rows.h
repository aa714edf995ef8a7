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

// acc[nt][mt] += W[tile nt] . X[rows of m-tile mt]^T over KG k-groups of 16.  wp: packed weights of the first n-tile
// ([n-tile][k-group][lane][4], KG k-groups per n-tile); xs: LDS rows, ld floats apart.  Lane l supplies, in k-step s of a
// k-group, W[n0 + l%16][16 kg + 4 (l/16) + s] and X[m0 + l%16][16 kg + 4 (l/16) + s]: one 16-byte load of each per k-group.
template <int NT, int MT, int KG, int LD>
__device__ __forceinline__ void mm(f32x4 (&acc)[NT][MT], const float *__restrict__ wp, const float *xs, int lane) {
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(wp) + lane;
    const float *xr = xs + (lane & 15) * LD + 4 * (lane >> 4);
    f32x4 w[2][NT], x[2][MT];
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
    int kg = 0;
#pragma unroll 1
    for (; kg + 2 <= KG; kg += 2) {
        load(kg + 1, 1);
        step(0);
        if (kg + 2 < KG) load(kg + 2, 0);
        step(1);
    }
    if constexpr (KG & 1) step(0);
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
