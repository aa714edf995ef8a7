// sdf_device.h -- device arithmetic shared by the kernels that read an SDF volume (sdf.hip, sdf_refine.hip, sdf_raycast.hip,
// hand_pose.hip, hand_interact.hip, tsdf_fuse.hip, sdf_mesh.hip): the volume-element loader, the object-frame transform, torch's
// floor division and the nearest-voxel index of gf_optimize_hand_pose.query_sdf, the lookup fused into the hand kernels, the
// trilinear cell of gf_optimize_obj.Distance (coordinate split, flat index, corner-layout load, eight-value blend), a batched
// problem's slice of its packed inputs, and the small rotation helpers of the pose updates.  One definition, so that a lookup
// fused into another kernel reads the same voxel as pn2s_nearest and blends the same cell as pn2s_trilinear.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace pn2 {

__device__ __forceinline__ float clampf(float v, float lo, float hi) {  // torch.clamp: min(max(v, lo), hi)
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// (p - t) @ R with the fixed chain o_j = fma(q2, R2j, fma(q1, R1j, q0*R0j)) (same chain in oracle/sdf_oracle.c).
__device__ __forceinline__ void to_object_frame(float px, float py, float pz, const float *t, const float *R, float &ox,
                                                float &oy, float &oz) {
    const float q0 = px - t[0], q1 = py - t[1], q2 = pz - t[2];
    ox = fmaf(q2, R[6], fmaf(q1, R[3], q0 * R[0]));
    oy = fmaf(q2, R[7], fmaf(q1, R[4], q0 * R[1]));
    oz = fmaf(q2, R[8], fmaf(q1, R[5], q0 * R[2]));
}

// torch's `tensor // scalar` on floats is c10::div_floor_floating: fmod, (a - mod) / b, sign fix-up, floor, and a
// +1 if that floor fell below the rounding error -- for b > 0 and |a/b| < 2^22 that is exactly the mathematical
// floor of the real quotient a/b (derivation in DESIGN.md section 8).  fmodf costs ~100 instructions and made this
// kernel ALU-bound (39 us); the same integer comes from one correctly rounded division and one exact-sign FMA
// remainder:  k = floor(RN(a/b));  r = fma(-k, b, a)  has the sign of the true remainder a - k*b (an FMA rounds
// once and never rounds a non-zero value to zero, so its SIGN is exact -- its magnitude is not: a tiny negative a
// gives r = b - tiny, which rounds to b, hence the second test looks at the sign of a - (k+1)*b instead of r >= b);
// k is off by at most one, fixed by the two sign tests.  Beyond 2^22 both versions are far outside the clamp
// range [-res/2, res/2] applied next, so the voxel index is identical for every finite input
// (tests: bit-exact indices vs the literal restatement in oracle/sdf_oracle.c on adversarial k*b +- ulp inputs).
__device__ __forceinline__ float div_floor(float a, float b) {
    float k = floorf(a / b);
    if (fmaf(-k, b, a) < 0.0f) k -= 1.0f;                  // a - k*b < 0: k is one too large
    else if (fmaf(-(k + 1.0f), b, a) >= 0.0f) k += 1.0f;   // a - (k+1)*b >= 0: k is one too small
    return k;
}

// Flat index of the voxel query_sdf reads for the object-frame point (ox, oy, oz) (optimization_hand.py:252-262): per axis
// clamp(q // voxel_scale, -(res/2), res/2) + res/2, res odd.
__device__ __forceinline__ int nearest_voxel(float ox, float oy, float oz, float voxel_scale, int res) {
    const int half = res / 2;
    const float fh = (float)half;
    const int ix = (int)clampf(div_floor(ox, voxel_scale), -fh, fh) + half;
    const int iy = (int)clampf(div_floor(oy, voxel_scale), -fh, fh) + half;
    const int iz = (int)clampf(div_floor(oz, voxel_scale), -fh, fh) + half;
    return (ix * res + iy) * res + iz;
}

// Element i of a volume, linear or corner layout, fp16 or fp32, as fp32; and its store, an fp16 volume rounded to nearest even.
template <bool F16>
__device__ __forceinline__ float ld_vol(const void *vol, int i) {
    if (F16) return __half2float(reinterpret_cast<const __half *>(vol)[i]);
    return reinterpret_cast<const float *>(vol)[i];
}
template <bool F16>
__device__ __forceinline__ void st_vol(void *vol, int i, float x) {
    if (F16) reinterpret_cast<__half *>(vol)[i] = __float2half_rn(x);
    else reinterpret_cast<float *>(vol)[i] = x;
}

// query_sdf for one camera-frame point: the object frame, the nearest voxel, the volume's value (fp16 or fp32) as fp32
template <bool F16>
__device__ __forceinline__ float sdf_nearest(const void *vol, float x, float y, float z, const float *ot, const float *oR,
                                             float voxel_scale, int res) {
    float ox, oy, oz;
    to_object_frame(x, y, z, ot, oR, ox, oy, oz);
    return ld_vol<F16>(vol, nearest_voxel(ox, oy, oz, voxel_scale, res));
}

// ---- one trilinear cell (gf_optimize_obj.Distance, optimization_obj.py:184-228) ---------------------------------------------------
// How a coordinate is clamped into [0, res - 1], which cell a clamped coordinate on the top face belongs to, and how a linear
// volume is gathered differ between the callers on purpose and stay with them; what follows is what they share.

// a clamped grid coordinate c in [0, res - 1] -> its cell index and the fraction inside the cell (c >= 0: trunc == floor)
__device__ __forceinline__ int cell_split(float c, float &frac) {
    const int i = (int)c;
    frac = c - (float)i;
    return i;
}

__device__ __forceinline__ int cell_index(int ix, int iy, int iz, int res) { return (ix * res + iy) * res + iz; }

// Cell i of the corner layout (pn2s_build_corner_volume): the eight values d000 .. d111 (d_abc: a along x, c along z) that the
// reference fetches for i000 == i, already clamped its way -> ONE 16-byte (fp16) or two 16-byte (fp32) loads per point
template <bool F16>
__device__ __forceinline__ void ld_corner_cell(const void *vol, int i, float *d) {
    if constexpr (F16) {
        const uint4 w = reinterpret_cast<const uint4 *>(vol)[i];
        const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[2 * k] = __half2float(__ushort_as_half((unsigned short)(u[k] & 0xffffu)));
            d[2 * k + 1] = __half2float(__ushort_as_half((unsigned short)(u[k] >> 16)));
        }
    } else {
        const float4 a = reinterpret_cast<const float4 *>(vol)[2 * (size_t)i], b = reinterpret_cast<const float4 *>(vol)[2 * (size_t)i + 1];
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
        d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    }
}

// The cell's value at the fractions (x, y, z) in Distance's association order (:223-226; products and sums, no fmaf), NOT clamped.
// c[0..3] = c00, c01, c10, c11, the four blends along z, for a caller that differentiates the interpolant.
__device__ __forceinline__ float cell_blend(const float *d, float x, float y, float z, float *c) {
    const float mx = 1.0f - x, my = 1.0f - y, mz = 1.0f - z;
    c[0] = d[0] * mz + d[1] * z;
    c[1] = d[2] * mz + d[3] * z;
    c[2] = d[4] * mz + d[5] * z;
    c[3] = d[6] * mz + d[7] * z;
    return (c[0] * my + c[1] * y) * mx + (c[2] * my + c[3] * y) * x;
}
__device__ __forceinline__ float cell_blend(const float *d, float x, float y, float z) {
    float c[4];
    return cell_blend(d, x, y, z, c);
}

// ---- a batched problem's slice ----------------------------------------------------------------------------------------------------
// Problem k of a batch owns the rows [cloud_off[k], cloud_off[k+1]) of the packed cloud and the entry vols[k] of the volume table:
// pcld, n and vol become its own.  false: the slice is empty (or its start negative) and the problem is INACTIVE -- the caller
// returns at once, so everything the problem owns keeps every byte.  The table's ENTRY is loaded for every problem, the volume it
// points to is read by active ones only: an inactive problem's entry may be NULL.
__device__ __forceinline__ bool problem_slice(const int *cloud_off, const void *const *vols, int k, const float *&pcld, int &n,
                                              const void *&vol) {
    const int o0 = cloud_off[k], o1 = cloud_off[k + 1];
    vol = vols[k];
    if (o0 < 0 || o1 <= o0) return false;
    n = o1 - o0;
    pcld += 3 * (size_t)o0;
    return true;
}

__device__ __forceinline__ void quat_to_matrix(float w, float x, float y, float z, float *m) {  // rotations.py:105-113
    m[0] = 1.0f - 2.0f * y * y - 2.0f * z * z;  m[1] = 2.0f * x * y - 2.0f * z * w;         m[2] = 2.0f * x * z + 2.0f * y * w;
    m[3] = 2.0f * x * y + 2.0f * z * w;         m[4] = 1.0f - 2.0f * x * x - 2.0f * z * z;  m[5] = 2.0f * y * z - 2.0f * x * w;
    m[6] = 2.0f * x * z - 2.0f * y * w;         m[7] = 2.0f * y * z + 2.0f * x * w;         m[8] = 1.0f - 2.0f * x * x - 2.0f * y * y;
}

__device__ __forceinline__ void mat3_mul(const float *a, const float *b, float *o) {  // o = a @ b, fixed fma chain
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = fmaf(a[3 * i + 2], b[6 + j], fmaf(a[3 * i + 1], b[3 + j], a[3 * i] * b[j]));
}

__device__ __forceinline__ void normalize3(float *v) {  // rotations.py:328-340
    const float mag = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (mag > 1e-8f) {
        v[0] /= mag; v[1] /= mag; v[2] /= mag;
    } else {
        v[0] = 1.0f; v[1] = 0.0f; v[2] = 0.0f;
    }
}

}  // namespace pn2
