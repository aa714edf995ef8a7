// tsdf_fuse.hip -- tracked depth frames fused into an SDF volume (include/pn2_sdf.h: pn2s_tsdf_integrate): the online shape update
// for volumes that come from a mesh or are handed over, KinectFusion's weighted running average of truncated signed distances.
// The reference refits a DeepSDF latent instead (optimization_obj.py:345-403), which needs its decoder.
//
// One launch integrates `frames` depth frames, in order, into one volume in place.  Voxel (ix,iy,iz), linear (ix*res + iy)*res + iz,
// has the centre p = ((float)(i - res/2)) * voxel_scale per axis (one fp32 product; the grid of pn2s_mesh_sdf_volume).  Per frame,
// R (3,3 row-major), t (3), (fx, fy, cx, cy) read from device memory, all arithmetic fp32, every operation rounded once unless it
// is written as fmaf:
//   1. q_i = fmaf(R_i2, p_z, fmaf(R_i0, p_x, fmaf(R_i1, p_y, t_i)))          (q = R p + t: the tracker's cloud is (pcld - t) @ R)
//      flip_yz:  q_y = -q_y,  q_z = -q_z
//   2. skip unless q_z > 1e-6f
//   3. u = rintf(q_x / q_z * fx + cx),  v = rintf(q_y / q_z * fy + cy)        (a division, a product, a sum; round half to even)
//      skip unless 0 <= u <= w - 1 and 0 <= v <= h - 1 (compared as floats: a NaN skips)
//   4. D = depth[v, u], for uint16 counts (float)((double)raw * depth_scale);  skip unless D > 0 and D is finite
//   5. d = D - q_z;  the pixel is the object's iff seg[v / f, u / f, channel] == value  (f = h / hs, as depth_frame.hip)
//        object:      skip if d < -trunc;  s = fminf(d, trunc), g = 1
//        otherwise:   skip unless d > trunc;  s = trunc, g = carve_weight  (hand, background: free space only)
//      skip if g == 0  (carve_weight = 0: nothing is carved, and no 0 / 0 where the weight is 0 too)
//   6. V = fmaf(V, W, s * g) / (W + g);   W = fminf(W + g, max_weight)
// One lane owns kZ consecutive z of one (ix,iy) row and keeps their V and W in fp32 registers over all frames; a voxel that some
// frame updated is written once at the end, a voxel that no frame updated is not written at all (its bytes stay).  So the volume
// and the weights are read once and written at most once per launch however many frames are fused, there are no atomics, two
// runs are bitwise equal, and for an fp32 volume one launch of F frames gives the bits of F launches of one frame.  An fp16
// volume is rounded ONCE, at the final store (round to nearest even): F single-frame launches round F times and differ.
//
// Launch shape: block (64, 4) -- a wave is 64 lanes along z, kZ = 4 z each (256 z), the block's four waves are four y rows; grid
// (ceil(res / 256), ceil(res / 4), res): (ix,iy,iz) come from the block and thread indices, no division of a linear index.  A wave
// skips a frame's projections when none of its voxels lies in front of the camera, and its loads and updates when none projects
// into the image (ballots over values every lane computes anyway, so a skip never changes a result).
#include <hip/hip_fp16.h>
#include <cmath>

#include "pn2_common.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {
namespace tsdf {

constexpr int kZ = 4, kRows = 4, kMaxRes = 512;

struct Args {
    void *volume;
    float *weight;
    const void *depth;
    const unsigned char *seg;
    const float *intrinsics, *rotation, *translation;
    double depth_scale;
    float voxel_scale, trunc, carve_weight, max_weight;
    int res, frames, h, w, ws, hs, c, f, fshift, flip, channel, value;
};

__device__ __forceinline__ float decode(float raw, double) { return raw; }
__device__ __forceinline__ float decode(unsigned short raw, double scale) { return (float)((double)raw * scale); }

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

template <bool F16, typename D>
__global__ __launch_bounds__(kWave * kRows) void tsdf_integrate_kernel(const Args A) {
    const int res = A.res, half = res / 2;
    const int ix = blockIdx.z, iy = blockIdx.y * kRows + threadIdx.y, z0 = (blockIdx.x * kWave + threadIdx.x) * kZ;
    if (iy >= res) return;  // (uniform over the wave: a wave is one y row)
    const int base = (ix * res + iy) * res;  // res <= 512: res^3 fits an int
    float V[kZ], W[kZ], pz[kZ];
    unsigned live = 0, touched = 0;
#pragma unroll
    for (int j = 0; j < kZ; ++j) {
        V[j] = W[j] = 0.f;
        pz[j] = (float)(z0 + j - half) * A.voxel_scale;
        if (z0 + j < res) {
            live |= 1u << j;
            V[j] = ld_vol<F16>(A.volume, base + z0 + j);
            W[j] = A.weight[base + z0 + j];
        }
    }
    const float px = (float)(ix - half) * A.voxel_scale, py = (float)(iy - half) * A.voxel_scale;
    const size_t hw = (size_t)A.h * A.w, seg_frame = (size_t)A.hs * A.ws * A.c;
    const float umax = (float)(A.w - 1), vmax = (float)(A.h - 1);
    for (int fr = 0; fr < A.frames; ++fr) {
        const float *R = A.rotation + 9 * fr, *t = A.translation + 3 * fr, *K = A.intrinsics + 4 * fr;
        const float r02 = R[2], r12 = R[5], r22 = R[8];
        const float ax = __builtin_fmaf(R[0], px, __builtin_fmaf(R[1], py, t[0]));
        const float ay = __builtin_fmaf(R[3], px, __builtin_fmaf(R[4], py, t[1]));
        const float az = __builtin_fmaf(R[6], px, __builtin_fmaf(R[7], py, t[2]));
        float qx[kZ], qy[kZ], qz[kZ];
        unsigned front = 0;
#pragma unroll
        for (int j = 0; j < kZ; ++j) {
            qx[j] = __builtin_fmaf(r02, pz[j], ax);
            qy[j] = __builtin_fmaf(r12, pz[j], ay);
            qz[j] = __builtin_fmaf(r22, pz[j], az);
            if (A.flip) {
                qy[j] = -qy[j];
                qz[j] = -qz[j];
            }
            front |= (qz[j] > 1e-6f ? 1u : 0u) << j;
        }
        front &= live;
        if (!__any(front != 0)) continue;  // the whole wave behind the camera
        const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
        float uf[kZ], vf[kZ];
        unsigned inside = 0;
#pragma unroll
        for (int j = 0; j < kZ; ++j) {
            uf[j] = rintf(qx[j] / qz[j] * fx + cx);
            vf[j] = rintf(qy[j] / qz[j] * fy + cy);
            inside |= (uf[j] >= 0.f && uf[j] <= umax && vf[j] >= 0.f && vf[j] <= vmax ? 1u : 0u) << j;
        }
        inside &= front;
        if (!__any(inside != 0)) continue;  // the whole wave outside the image
        const D *depth = static_cast<const D *>(A.depth) + (size_t)fr * hw;
        const unsigned char *seg = A.seg + (size_t)fr * seg_frame;
#pragma unroll
        for (int j = 0; j < kZ; ++j) {
            if (!((inside >> j) & 1u)) continue;
            const int u = (int)uf[j], v = (int)vf[j];  // inside [0, w - 1] x [0, h - 1]
            const float Dz = decode(depth[(size_t)v * A.w + u], A.depth_scale);
            if (!(Dz > 0.f) || Dz == __builtin_inff()) continue;
            const int us = A.fshift >= 0 ? u >> A.fshift : u / A.f, vs = A.fshift >= 0 ? v >> A.fshift : v / A.f;
            const bool obj = seg[((size_t)vs * A.ws + us) * A.c + A.channel] == A.value;
            const float d = Dz - qz[j];
            float s, g;
            if (obj) {
                if (d < -A.trunc) continue;
                s = fminf(d, A.trunc);
                g = 1.f;
            } else {
                if (!(d > A.trunc)) continue;
                s = A.trunc;
                g = A.carve_weight;
            }
            if (g == 0.f) continue;
            const float wn = W[j] + g;
            V[j] = __builtin_fmaf(V[j], W[j], s * g) / wn;
            W[j] = fminf(wn, A.max_weight);
            touched |= 1u << j;
        }
    }
#pragma unroll
    for (int j = 0; j < kZ; ++j) {
        if ((touched >> j) & 1u) {  // (touched is a subset of live: z0 + j < res)
            st_vol<F16>(A.volume, base + z0 + j, V[j]);
            A.weight[base + z0 + j] = W[j];
        }
    }
}

}  // namespace tsdf
}  // namespace pn2

using namespace pn2;
using namespace pn2::tsdf;

static_assert(sizeof(pn2s_tsdf_frames) == 128, "record layout (pn2_sdf.h)");

static inline bool finite_positive(float x) { return std::isfinite(x) && x > 0.f; }

extern "C" int pn2s_tsdf_integrate(const pn2s_tsdf_frames *frames, void *stream) {
    if (!frames) return PN2_ENULL;
    const pn2s_tsdf_frames &r = *frames;
    const bool sizes = r.h >= 1 && r.w >= 1 && r.hs >= 1 && r.ws >= 1;
    bool inval = r.res < 2 || r.frames < 1 || !sizes || (r.vol_f16 != 0 && r.vol_f16 != 1) || (r.depth_u16 != 0 && r.depth_u16 != 1) ||
                 (r.flip_yz != 0 && r.flip_yz != 1) || (r.c != 1 && r.c != 3);
    inval |= !finite_positive(r.voxel_scale) || !finite_positive(r.trunc) || !finite_positive(r.max_weight) ||
             !(std::isfinite(r.carve_weight) && r.carve_weight >= 0.f);
    inval |= sizes && (r.h % r.hs != 0 || r.w % r.ws != 0 || r.h / r.hs != r.w / r.ws);
    inval |= r.channel < 0 || r.channel >= r.c || r.value < 0 || r.value > 255;
    inval |= r.depth_u16 == 1 && !(std::isfinite(r.depth_scale) && r.depth_scale > 0.0);
    if (inval) return PN2_EINVAL;
    if (r.res > kMaxRes || (long)r.h * r.w >= (1L << 29) || r.frames > 65535) return PN2_ERANGE;
    if (!r.volume || !r.weight || !r.depth || !r.seg || !r.intrinsics || !r.rotation || !r.translation) return PN2_ENULL;
    Args A;
    A.volume = r.volume; A.weight = r.weight; A.depth = r.depth; A.seg = r.seg; A.intrinsics = r.intrinsics;
    A.rotation = r.rotation; A.translation = r.translation; A.depth_scale = r.depth_scale;
    A.voxel_scale = r.voxel_scale; A.trunc = r.trunc; A.carve_weight = r.carve_weight; A.max_weight = r.max_weight;
    A.res = r.res; A.frames = r.frames; A.h = r.h; A.w = r.w; A.ws = r.ws; A.hs = r.hs; A.c = r.c; A.f = r.h / r.hs;
    A.fshift = -1;
    for (int s = 0; s < 30; ++s)
        if (A.f == (1 << s)) A.fshift = s;
    A.flip = r.flip_yz; A.channel = r.channel; A.value = r.value;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((r.res + kWave * kZ - 1) / (kWave * kZ), (r.res + kRows - 1) / kRows, r.res), block(kWave, kRows);
    if (r.vol_f16) {
        if (r.depth_u16) hipLaunchKernelGGL((tsdf_integrate_kernel<true, unsigned short>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((tsdf_integrate_kernel<true, float>), grid, block, 0, st, A);
    } else {
        if (r.depth_u16) hipLaunchKernelGGL((tsdf_integrate_kernel<false, unsigned short>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((tsdf_integrate_kernel<false, float>), grid, block, 0, st, A);
    }
    return check_launch();
}
