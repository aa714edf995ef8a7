// sdf_raycast.hip -- an SDF volume rendered to depth and normal maps at tracked poses (include/pn2_sdf.h: pn2s_volume_raycast), and
// the rendered frames compared with the observed ones (pn2s_raycast_compare): the raycast of the KinectFusion loop whose other
// stages are depth_frame.hip (frames -> clouds), sdf.hip (tracking), tsdf_fuse.hip (fusion) and sdf_mesh.hip (extraction).  The
// reference has no counterpart (vis_utils.py draws matplotlib scatter plots).  DESIGN.md 8m.
//
// The geometry is the inverse of pn2s_tsdf_integrate's: q = R p + t takes an object-frame point to the camera frame, pixel (u, v)
// sees q along c = ((u - cx) / fx, (v - cy) / fy, 1), and the ray parameter IS the depth z (the projective distance of tsdf_fuse.hip).
// One lane renders one pixel.  R (3,3 row-major), t (3), (fx, fy, cx, cy) are read from device memory per frame.  All arithmetic is
// fp32, every operation rounded once unless it is written as fmaf; fminf / fmaxf return the other operand when one is a NaN:
//   1. ray     c_x = ((float)u - cx) / fx,  c_y = ((float)v - cy) / fy,  c_z = 1;          flip_yz:  c_y = -c_y,  c_z = -1
//              d_j = fmaf(R_2j, c_z, fmaf(R_0j, c_x, R_1j * c_y))                           (d = R^T c)
//              o_j = -fmaf(R_2j, t_2, fmaf(R_0j, t_0, R_1j * t_1))                          (o = -R^T t)
//              speed = sqrtf(fmaf(d_2, d_2, fmaf(d_0, d_0, d_1 * d_1)))
//   2. box     lo = (float)(-(res / 2)) * voxel_scale,  hi = lo + (float)(res - 1) * voxel_scale    (the trilinear domain [lo, hi]^3)
//              per axis  a = (lo - o_j) / d_j,  b = (hi - o_j) / d_j;   z_in = max_j fminf(a, b),  z_out = min_j fmaxf(a, b)
//              (both folded with fmaxf / fminf, j = 0, 1, 2);   z_in = fmaxf(z_in, 1e-3f);   no ray unless z_out > z_in (a NaN: no ray)
//   3. sample  s(p):  g_j = fminf(fmaxf((p_j - lo) / voxel_scale, 0), (float)(res - 1)),  i_j = min((int)g_j, res - 2),  f_j = g_j - (float)i_j,
//              the eight values V[i + (a,b,c)] of the linear volume (ix * res + iy) * res + iz blended as the reference's Distance does
//              (optimization_obj.py:223-226; x = f_0, y = f_1, z = f_2, products and sums, no fmaf):
//                ((V000 (1 - z) + V001 z) (1 - y) + (V010 (1 - z) + V011 z) y) (1 - x) + ((V100 (1 - z) + V101 z) (1 - y) + (V110 (1 - z) + V111 z) y) x
//              with NO +-0.05 clamp: a volume truncated at +-trunc is seen as it is.   s(z) = s(p),  p_j = fmaf(z, d_j, o_j)
//   4. march   z = z_in, s = s(z);  no hit unless s > 0 (the ray starts inside the surface, or on a NaN);  m = min_step * voxel_scale;
//              at most max_steps times:  dz = fmaxf(s * step_scale, m) / speed,  z' = fminf(z + dz, z_out),  s' = s(z');
//                s' <= 0:  the bracket is [z, z'] with values (s, s'), stop;   else  !(z' < z_out):  no hit, stop;   else  z = z', s = s'
//              out of steps: no hit.  A NaN s' is not <= 0, so it never hits, and its step is m / speed: the march goes on.
//   5. refine  `refine` times:  z_m = (z_a + z_b) * 0.5f,  s_m = s(z_m);   s_m <= 0 ? (z_b, s_b) = (z_m, s_m) : (z_a, s_a) = (z_m, s_m)
//              z_hit = z_a + (z_b - z_a) * s_a / (s_a - s_b)            (a difference, a product, a difference, a division, a sum)
//   6. normal  p_j = fmaf(z_hit, d_j, o_j),  e = 0.5f * voxel_scale,  g_j = s(p + e unit_j) - s(p - e unit_j)  (p_j + e and p_j - e: one sum each)
//              n2 = fmaf(g_2, g_2, fmaf(g_0, g_0, g_1 * g_1));   n2 > 0:  g_j = g_j / sqrtf(n2),  else g = (0, 0, 0)  (the pixel stays a hit)
//              n_i = fmaf(R_i2, g_2, fmaf(R_i0, g_0, R_i1 * g_1));   flip_yz:  n_y = -n_y,  n_z = -n_z     (n = R g, the camera frame)
//   7. depth[v, u] = z_hit for a hit, else 0;  normal[v, u] = n for a hit, else (0, 0, 0).  The hit mask is depth > 0 (a bracket that
//      opened on a NaN value interpolates to a NaN, which is not a hit).
//
// Launch shape: block (8, 8, 4) -- a wave is one 8 x 8 pixel tile, so its rays touch neighbouring cells, and a block's four waves are
// four tiles side by side; grid (ceil(w / 32), ceil(h / 8), frames): pixel and frame come from block and thread indices, no division
// of a linear index.  A wave leaves the march when none of its lanes is still marching, and skips the refinement and the normals
// when none hit (ballots over values every lane computes anyway, so a skip never changes a result); a lane that has finished goes
// on sampling at its last position, inside the volume, and its results are discarded.  The loop is bounded by max_steps, not by
// convergence.  No atomics, no LDS, no scratch; every pixel of the image is written exactly once, and two runs are bitwise equal.
//
// pn2s_raycast_compare: one workgroup of 1024 lanes per frame walks the frame's pixels in a fixed order, counts in integers and sums
// |D - Z| in fp32 per lane, then per wave (xor butterfly), then over the 16 waves in order: no atomics, two runs are bitwise equal.
#include "frame_device.h"
#include "sdf_device.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {
namespace raycast {

constexpr int kTile = 8, kTilesPerBlock = 4, kMaxRes = 512, kCompareLanes = 1024;

struct Args {
    const void *volume;
    const float *intrinsics, *rotation, *translation;
    float *depth, *normal;
    float voxel_scale, step_scale, min_step;
    int res, h, w, flip, refine, max_steps;
};

// The volume as the sampler sees it: every index it forms lies in [0, res^3) whatever the point (a NaN coordinate clamps to 0).
struct Field {
    const void *vol;
    float lo, scale, top;  // top = (float)(res - 1)
    int res, rr;           // res <= 512: res^3 fits an int
};

template <bool F16>
__device__ __forceinline__ float sample(const Field &G, float px, float py, float pz) {
    const float gx = fminf(fmaxf((px - G.lo) / G.scale, 0.f), G.top);
    const float gy = fminf(fmaxf((py - G.lo) / G.scale, 0.f), G.top);
    const float gz = fminf(fmaxf((pz - G.lo) / G.scale, 0.f), G.top);
    const int ix = min((int)gx, G.res - 2), iy = min((int)gy, G.res - 2), iz = min((int)gz, G.res - 2);
    const float x = gx - (float)ix, y = gy - (float)iy, z = gz - (float)iz;
    const int i000 = cell_index(ix, iy, iz, G.res);
    const float d[8] = {ld_vol<F16>(G.vol, i000),                 ld_vol<F16>(G.vol, i000 + 1),
                        ld_vol<F16>(G.vol, i000 + G.res),         ld_vol<F16>(G.vol, i000 + G.res + 1),
                        ld_vol<F16>(G.vol, i000 + G.rr),          ld_vol<F16>(G.vol, i000 + G.rr + 1),
                        ld_vol<F16>(G.vol, i000 + G.rr + G.res),  ld_vol<F16>(G.vol, i000 + G.rr + G.res + 1)};
    return cell_blend(d, x, y, z);
}

template <bool F16, bool NORMALS>
__global__ __launch_bounds__(kTile * kTile * kTilesPerBlock) void sdf_raycast_kernel(const Args A) {
    const int u = (blockIdx.x * kTilesPerBlock + threadIdx.z) * kTile + threadIdx.x;
    const int v = blockIdx.y * kTile + threadIdx.y;
    const int fr = blockIdx.z;
    const bool in = u < A.w && v < A.h;
    if (!__any(in)) return;  // the whole tile outside the image (uniform over the wave)
    const float *R = A.rotation + 9 * fr, *t = A.translation + 3 * fr, *K = A.intrinsics + 4 * fr;
    const float r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
    Field G;
    G.vol = A.volume; G.res = A.res; G.rr = A.res * A.res; G.scale = A.voxel_scale; G.top = (float)(A.res - 1);
    G.lo = (float)(-(A.res / 2)) * A.voxel_scale;
    const float hi = G.lo + G.top * A.voxel_scale;
    // 1. the ray
    const float cx = ((float)u - K[2]) / K[0];
    float cy = ((float)v - K[3]) / K[1], cz = 1.f;
    if (A.flip) {
        cy = -cy;
        cz = -1.f;
    }
    const float d0 = __builtin_fmaf(r20, cz, __builtin_fmaf(r00, cx, r10 * cy));
    const float d1 = __builtin_fmaf(r21, cz, __builtin_fmaf(r01, cx, r11 * cy));
    const float d2 = __builtin_fmaf(r22, cz, __builtin_fmaf(r02, cx, r12 * cy));
    const float o0 = -__builtin_fmaf(r20, t[2], __builtin_fmaf(r00, t[0], r10 * t[1]));
    const float o1 = -__builtin_fmaf(r21, t[2], __builtin_fmaf(r01, t[0], r11 * t[1]));
    const float o2 = -__builtin_fmaf(r22, t[2], __builtin_fmaf(r02, t[0], r12 * t[1]));
    const float speed = sqrtf(__builtin_fmaf(d2, d2, __builtin_fmaf(d0, d0, d1 * d1)));
    // 2. the box
    const float a0 = (G.lo - o0) / d0, b0 = (hi - o0) / d0, a1 = (G.lo - o1) / d1, b1 = (hi - o1) / d1;
    const float a2 = (G.lo - o2) / d2, b2 = (hi - o2) / d2;
    float z_in = fmaxf(fmaxf(fminf(a0, b0), fminf(a1, b1)), fminf(a2, b2));
    const float z_out = fminf(fminf(fmaxf(a0, b0), fmaxf(a1, b1)), fmaxf(a2, b2));
    z_in = fmaxf(z_in, 1e-3f);
    const bool ray = in && z_out > z_in;
    // 4. the march
    float z = ray ? z_in : 0.f;
    float s = sample<F16>(G, __builtin_fmaf(z, d0, o0), __builtin_fmaf(z, d1, o1), __builtin_fmaf(z, d2, o2));
    bool alive = ray && s > 0.f, hit = false;
    float za = 0.f, zb = 0.f, sa = 0.f, sb = 0.f;
    const float m = A.min_step * A.voxel_scale;
    for (int it = 0; it < A.max_steps; ++it) {
        if (!__any(alive)) break;  // no lane of the wave is marching
        const float dz = fmaxf(s * A.step_scale, m) / speed;
        const float zn = fminf(z + dz, z_out);
        const float sn = sample<F16>(G, __builtin_fmaf(zn, d0, o0), __builtin_fmaf(zn, d1, o1), __builtin_fmaf(zn, d2, o2));
        const bool cross = alive && sn <= 0.f;
        if (cross) {
            za = z; sa = s; zb = zn; sb = sn;
            hit = true;
        }
        alive = alive && !cross && zn < z_out;
        if (alive) {
            z = zn;
            s = sn;
        }
    }
    const size_t pix = ((size_t)fr * A.h + (in ? v : 0)) * A.w + (in ? u : 0);
    if (!__any(hit)) {  // nothing of this tile to refine or shade
        if (in) {
            A.depth[pix] = 0.f;
            if (NORMALS) A.normal[3 * pix] = A.normal[3 * pix + 1] = A.normal[3 * pix + 2] = 0.f;
        }
        return;
    }
    // 5. the refinement
    for (int k = 0; k < A.refine; ++k) {
        const float zm = (za + zb) * 0.5f;
        const float sm = sample<F16>(G, __builtin_fmaf(zm, d0, o0), __builtin_fmaf(zm, d1, o1), __builtin_fmaf(zm, d2, o2));
        const bool neg = sm <= 0.f;
        zb = neg ? zm : zb; sb = neg ? sm : sb;
        za = neg ? za : zm; sa = neg ? sa : sm;
    }
    const float zh = za + (zb - za) * sa / (sa - sb);
    if (in) A.depth[pix] = hit ? zh : 0.f;
    if (NORMALS) {
        // 6. the normal
        const float p0 = __builtin_fmaf(zh, d0, o0), p1 = __builtin_fmaf(zh, d1, o1), p2 = __builtin_fmaf(zh, d2, o2);
        const float e = 0.5f * A.voxel_scale;
        float g0 = sample<F16>(G, p0 + e, p1, p2) - sample<F16>(G, p0 - e, p1, p2);
        float g1 = sample<F16>(G, p0, p1 + e, p2) - sample<F16>(G, p0, p1 - e, p2);
        float g2 = sample<F16>(G, p0, p1, p2 + e) - sample<F16>(G, p0, p1, p2 - e);
        const float n2 = __builtin_fmaf(g2, g2, __builtin_fmaf(g0, g0, g1 * g1));
        if (n2 > 0.f) {
            const float len = sqrtf(n2);
            g0 = g0 / len; g1 = g1 / len; g2 = g2 / len;
        } else {
            g0 = g1 = g2 = 0.f;
        }
        const float nx = __builtin_fmaf(r02, g2, __builtin_fmaf(r00, g0, r01 * g1));
        float ny = __builtin_fmaf(r12, g2, __builtin_fmaf(r10, g0, r11 * g1));
        float nz = __builtin_fmaf(r22, g2, __builtin_fmaf(r20, g0, r21 * g1));
        if (A.flip) {
            ny = -ny;
            nz = -nz;
        }
        if (in) {
            A.normal[3 * pix] = hit ? nx : 0.f;
            A.normal[3 * pix + 1] = hit ? ny : 0.f;
            A.normal[3 * pix + 2] = hit ? nz : 0.f;
        }
    }
}

// ---- rendered against observed -------------------------------------------------------------------------------------------------
struct CompareArgs {
    const float *rendered;
    const void *depth;
    float *out;
    double depth_scale;
    float occl_margin;
    int h, w;
    SegMap object;
};

// Frame blockIdx.x.  With D the observed depth (valid: D > 0 and finite), Z the rendered one (a hit: Z > 0) and `object` the pixel's
// segment byte seg[v / f, u / f, channel] == value (frame_device.h):
//   A = object and valid;   Occ = not object, valid, a hit, D < Z - occl_margin (something in front of the model);   B = a hit outside Occ
//   out[frame] = (|A n B|, |A u B|, sum over A n B of |D - Z|, |Occ|), the counts converted from integers at the end.
template <typename D>
__global__ __launch_bounds__(kCompareLanes) void sdf_raycast_compare_kernel(const CompareArgs A) {
    __shared__ unsigned cnt[kCompareLanes / kWave][3];
    __shared__ float res_sum[kCompareLanes / kWave];
    const int fr = blockIdx.x, tid = threadIdx.x;
    const float *Zf = A.rendered + (size_t)fr * A.h * A.w;
    const D *Df = static_cast<const D *>(A.depth) + (size_t)fr * A.h * A.w;
    const unsigned char *seg = A.object.frame(fr);
    unsigned n_and = 0, n_or = 0, n_occ = 0;
    float sum = 0.f;
    // rows by the lane's row of the workgroup, columns by its column: no division of a pixel index.  kCompareLanes = 16 rows of 64
    for (int v = tid >> 6; v < A.h; v += kCompareLanes / kWave) {
        const int vs = A.object.down(v);
        for (int u = tid & 63; u < A.w; u += kWave) {
            const float Z = Zf[(size_t)v * A.w + u];
            const float Dz = decode(Df[(size_t)v * A.w + u], A.depth_scale);
            const bool obj = A.object.holds(A.object.cell(seg, vs, A.object.down(u)));
            const bool valid = Dz > 0.f && Dz != __builtin_inff();
            const bool hit = Z > 0.f;
            const bool occ = !obj && valid && hit && Dz < Z - A.occl_margin;
            const bool a = obj && valid, b = hit && !occ;
            n_and += a && b;
            n_or += a || b;
            n_occ += occ;
            if (a && b) sum += fabsf(Dz - Z);
        }
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        n_and += __shfl_xor(n_and, msk, 64);
        n_or += __shfl_xor(n_or, msk, 64);
        n_occ += __shfl_xor(n_occ, msk, 64);
    }
    sum = wave_sum_xor(sum);
    if ((tid & 63) == 0) {
        cnt[tid >> 6][0] = n_and; cnt[tid >> 6][1] = n_or; cnt[tid >> 6][2] = n_occ;
        res_sum[tid >> 6] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned c0 = 0, c1 = 0, c2 = 0;
        float r = 0.f;
        for (int wv = 0; wv < kCompareLanes / kWave; ++wv) {
            c0 += cnt[wv][0]; c1 += cnt[wv][1]; c2 += cnt[wv][2];
            r += res_sum[wv];
        }
        float *o = A.out + 4 * fr;
        o[0] = (float)c0; o[1] = (float)c1; o[2] = r; o[3] = (float)c2;
    }
}

}  // namespace raycast
}  // namespace pn2

using namespace pn2;
using namespace pn2::raycast;

static_assert(sizeof(pn2s_raycast) == 96, "record layout (pn2_sdf.h)");
static_assert(sizeof(pn2s_raycast_frames) == 80, "record layout (pn2_sdf.h)");

extern "C" int pn2s_volume_raycast(const pn2s_raycast *raycast, void *stream) {
    if (!raycast) return PN2_ENULL;
    const pn2s_raycast &r = *raycast;
    bool inval = r.res < 2 || r.frames < 1 || r.h < 1 || r.w < 1 || (r.vol_f16 != 0 && r.vol_f16 != 1) || (r.flip_yz != 0 && r.flip_yz != 1);
    inval |= !finite_positive(r.voxel_scale) || !finite_positive(r.step_scale) || !finite_positive(r.min_step);
    inval |= r.refine < 0 || r.refine > 16 || r.max_steps < 1;
    if (inval) return PN2_EINVAL;
    if (r.res > kMaxRes || (long)r.h * r.w >= (1L << 29) || r.frames > 65535 || r.h > 65535 * kTile) return PN2_ERANGE;
    if (!r.volume || !r.intrinsics || !r.rotation || !r.translation || !r.depth) return PN2_ENULL;  // (normal may be NULL)
    Args A;
    A.volume = r.volume; A.intrinsics = r.intrinsics; A.rotation = r.rotation; A.translation = r.translation;
    A.depth = r.depth; A.normal = r.normal;
    A.voxel_scale = r.voxel_scale; A.step_scale = r.step_scale; A.min_step = r.min_step;
    A.res = r.res; A.h = r.h; A.w = r.w; A.flip = r.flip_yz; A.refine = r.refine; A.max_steps = r.max_steps;
    hipStream_t st = (hipStream_t)stream;
    const int span = kTile * kTilesPerBlock;
    const dim3 grid((r.w + span - 1) / span, (r.h + kTile - 1) / kTile, r.frames), block(kTile, kTile, kTilesPerBlock);
    if (r.vol_f16) {
        if (r.normal) hipLaunchKernelGGL((sdf_raycast_kernel<true, true>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((sdf_raycast_kernel<true, false>), grid, block, 0, st, A);
    } else {
        if (r.normal) hipLaunchKernelGGL((sdf_raycast_kernel<false, true>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((sdf_raycast_kernel<false, false>), grid, block, 0, st, A);
    }
    return check_launch();
}

extern "C" int pn2s_raycast_compare(const pn2s_raycast_frames *frames, void *stream) {
    if (!frames) return PN2_ENULL;
    const pn2s_raycast_frames &r = *frames;
    Faults f;
    f.inval = r.frames < 1 || !(std::isfinite(r.occl_margin) && r.occl_margin >= 0.f);
    check_image_pair(r.frames, r.h, r.w, r.hs, r.ws, r.c, f);
    check_class(r.channel, r.value, r.c, f);
    check_depth_encoding(r.depth_u16, r.depth_scale, f);
    f.null = !r.rendered || !r.depth || !r.seg || !r.out;
    if (f.code() != PN2_OK) return f.code();
    CompareArgs A;
    A.rendered = r.rendered; A.depth = r.depth; A.object = seg_map(r.seg, r.h, r.hs, r.ws, r.c, r.channel, r.value); A.out = r.out;
    A.depth_scale = r.depth_scale; A.occl_margin = r.occl_margin; A.h = r.h; A.w = r.w;
    hipStream_t st = (hipStream_t)stream;
    if (r.depth_u16) hipLaunchKernelGGL((sdf_raycast_compare_kernel<unsigned short>), dim3(r.frames), dim3(kCompareLanes), 0, st, A);
    else hipLaunchKernelGGL((sdf_raycast_compare_kernel<float>), dim3(r.frames), dim3(kCompareLanes), 0, st, A);
    return check_launch();
}
