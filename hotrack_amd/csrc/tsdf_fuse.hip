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
//   5. d = D - q_z;  the pixel is the object's iff seg[v / f, u / f, channel] == value  (f = h / hs: frame_device.h)
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
//
// pn2s_tsdf_integrate_batch is the same rule (the one __device__ function below, called by both kernels) for the S volumes of a
// group of sequences tracked in lockstep, in ONE launch: sequence k integrates its slice of the group's packed frame arrays into
// its own volume, with the bits pn2s_tsdf_integrate gives for those frames alone.
#include "frame_device.h"
#include "sdf_device.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {
namespace tsdf {

constexpr int kZ = 4, kRows = 4, kMaxRes = 512;

struct Args {
    void *volume;
    float *weight;
    const void *depth;
    const float *intrinsics, *rotation, *translation;
    double depth_scale;
    float voxel_scale, trunc, carve_weight, max_weight;
    int res, frames, h, w, flip;
    SegMap object;
};

// The rule, once, for both launches: this lane's kZ voxels (ix, iy, z0 .. z0 + kZ - 1) of `volume` / `weight` over the frames
// [f0, f1) of A's frame arrays.  iy < res (the caller's duty; z is masked here).
template <bool F16, typename D>
__device__ __forceinline__ void integrate_voxels(const Args &A, void *volume, float *weight, int f0, int f1, int ix, int iy, int z0) {
    const int res = A.res, half = res / 2;
    const int base = (ix * res + iy) * res;  // res <= 512: res^3 fits an int
    float V[kZ], W[kZ], pz[kZ];
    unsigned live = 0, touched = 0;
#pragma unroll
    for (int j = 0; j < kZ; ++j) {
        V[j] = W[j] = 0.f;
        pz[j] = (float)(z0 + j - half) * A.voxel_scale;
        if (z0 + j < res) {
            live |= 1u << j;
            V[j] = ld_vol<F16>(volume, base + z0 + j);
            W[j] = weight[base + z0 + j];
        }
    }
    const float px = (float)(ix - half) * A.voxel_scale, py = (float)(iy - half) * A.voxel_scale;
    const size_t hw = (size_t)A.h * A.w;
    const float umax = (float)(A.w - 1), vmax = (float)(A.h - 1);
    for (int fr = f0; fr < f1; ++fr) {
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
        const unsigned char *seg = A.object.frame(fr);
#pragma unroll
        for (int j = 0; j < kZ; ++j) {
            if (!((inside >> j) & 1u)) continue;
            const int u = (int)uf[j], v = (int)vf[j];  // inside [0, w - 1] x [0, h - 1]
            const float Dz = decode(depth[(size_t)v * A.w + u], A.depth_scale);
            if (!(Dz > 0.f) || Dz == __builtin_inff()) continue;
            const bool obj = A.object.is_class(seg, v, u);
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
            st_vol<F16>(volume, base + z0 + j, V[j]);
            weight[base + z0 + j] = W[j];
        }
    }
}

template <bool F16, typename D>
__global__ __launch_bounds__(kWave * kRows) void tsdf_integrate_kernel(const Args A) {
    const int ix = blockIdx.z, iy = blockIdx.y * kRows + threadIdx.y, z0 = (blockIdx.x * kWave + threadIdx.x) * kZ;
    if (iy >= A.res) return;  // (uniform over the wave: a wave is one y row)
    integrate_voxels<F16, D>(A, A.volume, A.weight, 0, A.frames, ix, iy, z0);
}

// S volumes in one launch (pn2s_tsdf_integrate_batch).  Grid (ztiles * yblocks, res, S): blockIdx.x carries the z tile in its low
// `ztshift` bits (ztiles is 1 or 2: kMaxRes <= 2 * kWave * kZ) and the y block above them, so a sequence's workgroups come in
// the single launch's order (z tile, y block, ix) and no index is divided.  Sequence k owns the frames [off[k], off[k+1]) clamped
// to [0, total]; with an empty slice its waves leave before the tables or any volume are read.
struct BatchArgs {
    Args A;  // (volume, weight and frames unused)
    void *const *volumes;
    float *const *weights;
    const int *frame_off;
    int total, ztshift;
};
static_assert(kMaxRes <= 2 * kWave * kZ, "the z tile is one bit of blockIdx.x");

template <bool F16, typename D>
__global__ __launch_bounds__(kWave * kRows) void tsdf_integrate_batch_kernel(const BatchArgs B) {
    const int k = blockIdx.z;
    const int f0 = max(B.frame_off[k], 0), f1 = min(B.frame_off[k + 1], B.total);
    if (f1 <= f0) return;  // the sequence sits out (uniform over the workgroup)
    const int zt = blockIdx.x & ((1 << B.ztshift) - 1), yb = blockIdx.x >> B.ztshift;
    const int ix = blockIdx.y, iy = yb * kRows + threadIdx.y, z0 = (zt * kWave + threadIdx.x) * kZ;
    if (iy >= B.A.res) return;
    integrate_voxels<F16, D>(B.A, B.volumes[k], B.weights[k], f0, f1, ix, iy, z0);
}

}  // namespace tsdf
}  // namespace pn2

using namespace pn2;
using namespace pn2::tsdf;

static_assert(sizeof(pn2s_tsdf_frames) == 128, "record layout (pn2_sdf.h)");
static_assert(sizeof(pn2s_tsdf_group) == 144, "record layout (pn2_sdf.h)");

// The checks both records share (their fields carry the same names): PN2_EINVAL before PN2_ERANGE; the observed frames' own
// are frame_device.h's.  `frames` is the record's frame count, at least `frames_min`.
template <typename R>
static int check_record(const R &r, int frames_min) {
    Faults f;
    f.inval = r.res < 2 || r.frames < frames_min || (r.vol_f16 != 0 && r.vol_f16 != 1) || (r.flip_yz != 0 && r.flip_yz != 1) ||
              !finite_positive(r.voxel_scale) || !finite_positive(r.trunc) || !finite_positive(r.max_weight) ||
              !(std::isfinite(r.carve_weight) && r.carve_weight >= 0.f);
    f.range = r.res > kMaxRes;
    check_image_pair(r.frames, r.h, r.w, r.hs, r.ws, r.c, f);
    check_class(r.channel, r.value, r.c, f);
    check_depth_encoding(r.depth_u16, r.depth_scale, f);
    return f.code();
}

// The kernels' view of a checked record (volume, weight and frames are the single entry's own).
template <typename R>
static Args frame_args(const R &r) {
    Args A;
    A.volume = nullptr; A.weight = nullptr; A.frames = 0;
    A.depth = r.depth; A.object = seg_map(r.seg, r.h, r.hs, r.ws, r.c, r.channel, r.value); A.intrinsics = r.intrinsics;
    A.rotation = r.rotation; A.translation = r.translation; A.depth_scale = r.depth_scale;
    A.voxel_scale = r.voxel_scale; A.trunc = r.trunc; A.carve_weight = r.carve_weight; A.max_weight = r.max_weight;
    A.res = r.res; A.h = r.h; A.w = r.w; A.flip = r.flip_yz;
    return A;
}

extern "C" int pn2s_tsdf_integrate(const pn2s_tsdf_frames *frames, void *stream) {
    if (!frames) return PN2_ENULL;
    const pn2s_tsdf_frames &r = *frames;
    if (const int rc = check_record(r, 1)) return rc;
    if (!r.volume || !r.weight || !r.depth || !r.seg || !r.intrinsics || !r.rotation || !r.translation) return PN2_ENULL;
    Args A = frame_args(r);
    A.volume = r.volume; A.weight = r.weight; A.frames = r.frames;
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

extern "C" int pn2s_tsdf_integrate_batch(const pn2s_tsdf_group *group, void *stream) {
    if (!group) return PN2_ENULL;
    const pn2s_tsdf_group &r = *group;
    if (r.sequences < 0) return PN2_EINVAL;
    if (const int rc = check_record(r, 0)) return rc;
    if (r.sequences > PN2S_TSDF_BATCH_MAX) return PN2_ERANGE;
    if (r.sequences == 0 || r.frames == 0) return PN2_OK;  // nothing to integrate: nothing is read or launched
    if (!r.volumes || !r.weights || !r.frame_off || !r.depth || !r.seg || !r.intrinsics || !r.rotation || !r.translation)
        return PN2_ENULL;
    BatchArgs B;
    B.A = frame_args(r);
    B.volumes = r.volumes; B.weights = r.weights; B.frame_off = r.frame_off; B.total = r.frames;
    const int ztiles = (r.res + kWave * kZ - 1) / (kWave * kZ);  // 1 or 2
    B.ztshift = ztiles - 1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ztiles * ((r.res + kRows - 1) / kRows), r.res, r.sequences), block(kWave, kRows);
    if (r.vol_f16) {
        if (r.depth_u16) hipLaunchKernelGGL((tsdf_integrate_batch_kernel<true, unsigned short>), grid, block, 0, st, B);
        else hipLaunchKernelGGL((tsdf_integrate_batch_kernel<true, float>), grid, block, 0, st, B);
    } else {
        if (r.depth_u16) hipLaunchKernelGGL((tsdf_integrate_batch_kernel<false, unsigned short>), grid, block, 0, st, B);
        else hipLaunchKernelGGL((tsdf_integrate_batch_kernel<false, float>), grid, block, 0, st, B);
    }
    return check_launch();
}

