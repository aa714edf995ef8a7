// depth_frame.hip -- hand and object clouds from depth frames (include/pn2_ext.h: pn2x_depth_frame_clouds).
//
// The reference's readers do this in numpy per frame (datasets/HO3D_dataset.py:66-112, :163-177): back-project the valid pixels,
// split them by segment, crop each segment to a ball, cap the cloud and hand it to FPS.  Here b frames go through two launches
// over a (tiles, b) grid, a tile being kTile consecutive pixels, four per thread:
//   depth_classify_kernel   classifies the pixels, writes the background mask and each tile's two class counts;
//   depth_place_kernel      sums the counts of the tiles before its own (and the total n), classifies its pixels again -- the same
//                           device function, so the same flags -- ranks them in pixel order (ballots and popcounts inside a
//                           wave, a prefix over the four waves) and stores every kept point at the slot its rank decides.
// The order across tiles comes from the launch boundary alone: no atomics, no workgroup waits for another, and every slot of
// every output is written by exactly one workgroup on every call.  Arithmetic is fp32 with every operation rounded once (the
// build sets -ffp-contract=off and correctly rounded '/' and sqrtf), so a numpy restatement reproduces it bit for bit.  What a
// depth pixel is in metres and which segment cell is its own: frame_device.h.
#include "frame_device.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace dframe {

constexpr int kThreads = 256, kPerThread = 4, kTile = kThreads * kPerThread, kWaves = kThreads / kWave;

struct Args {
    const void *depth;
    SegMap class0, class1;  // the two classes, over one seg
    const float *intrinsics, *centre0, *centre1;
    float *clouds;
    int *counts;
    unsigned char *background;
    int *work;
    double depth_scale;
    int h, w, cap, tiles, flip;
    float radius0, radius1;
};

__device__ __forceinline__ void load4(const float *p, float (&raw)[4]) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
}
__device__ __forceinline__ void load4(const unsigned short *p, unsigned short (&raw)[4]) {
    const ushort4 q = *reinterpret_cast<const ushort4 *>(p);
    raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
}

// The thread's four pixels p0 .. p0 + 3 of frame b (those below h w): their points, and per class a 4-bit mask of the pixels
// that belong to it; bg: the pixels whose segment bytes are all zero.
template <typename D>
__device__ __forceinline__ void classify(const Args &A, int b, int p0, float (&x)[4], float (&y)[4], float (&z)[4], unsigned &m0,
                                         unsigned &m1, unsigned &bg) {
    const int hw = A.h * A.w;
    const D *dp = static_cast<const D *>(A.depth) + (size_t)b * hw + p0;
    D raw[4] = {0, 0, 0, 0};
    if (p0 + kPerThread <= hw && ((uintptr_t)dp & (kPerThread * sizeof(D) - 1)) == 0) {
        load4(dp, raw);
    } else {
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
            if (p0 + j < hw) raw[j] = dp[j];
    }
    const float fx = A.intrinsics[4 * b], fy = A.intrinsics[4 * b + 1], cx = A.intrinsics[4 * b + 2], cy = A.intrinsics[4 * b + 3];
    const float ax = A.centre0[3 * b], ay = A.centre0[3 * b + 1], az = A.centre0[3 * b + 2];
    const float bx = A.centre1[3 * b], by = A.centre1[3 * b + 1], bz = A.centre1[3 * b + 2];
    const unsigned char *seg = A.class0.frame(b);
    int v = p0 / A.w, u = p0 - v * A.w;
    m0 = m1 = bg = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        x[j] = y[j] = z[j] = 0.f;
        if (p0 + j < hw) {
            const unsigned char *sp = A.class0.cell(seg, A.class0.down(v), A.class0.down(u));
            unsigned any = sp[0];
            if (A.class0.c == 3) any |= (unsigned)sp[1] | (unsigned)sp[2];
            bg |= (any == 0 ? 1u : 0u) << j;
            float pz = decode(raw[j], A.depth_scale);
            if (pz > 1e-6f) {
                const float px = ((float)u - cx) * pz / fx;
                float py = ((float)v - cy) * pz / fy;
                if (A.flip) {
                    py = -py;
                    pz = -pz;
                }
                x[j] = px; y[j] = py; z[j] = pz;
                if (A.class0.holds(sp)) {
                    const float dx = px - ax, dy = py - ay, dz = pz - az;
                    m0 |= (sqrtf((dx * dx + dy * dy) + dz * dz) < A.radius0 ? 1u : 0u) << j;
                }
                if (A.class1.holds(sp)) {
                    const float dx = px - bx, dy = py - by, dz = pz - bz;
                    m1 |= (sqrtf((dx * dx + dy * dy) + dz * dz) < A.radius1 ? 1u : 0u) << j;
                }
            }
        }
        if (++u == A.w) {
            u = 0;
            ++v;
        }
    }
}

// the pixels of mask bit j over the wave: how many there are (wave-uniform) and how many sit in lower lanes
__device__ __forceinline__ void wave_rank(unsigned m, int &below, int &total) {
    below = total = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const uint64_t bal = __ballot((m >> j) & 1u);
        below += prefix_popc(bal);
        total += __popcll(bal);
    }
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename D>
__global__ __launch_bounds__(kThreads) void depth_classify_kernel(const Args A) {
    __shared__ int wave_counts[2][kWaves];
    const int tile = blockIdx.x, b = blockIdx.y, hw = A.h * A.w, p0 = tile * kTile + threadIdx.x * kPerThread;
    float x[4], y[4], z[4];
    unsigned m0, m1, bg;
    classify<D>(A, b, p0, x, y, z, m0, m1, bg);
    unsigned char *bp = A.background + (size_t)b * hw + p0;
    if (p0 + kPerThread <= hw && ((uintptr_t)bp & 3) == 0) {
        *reinterpret_cast<unsigned *>(bp) = (bg & 1u) | ((bg & 2u) << 7) | ((bg & 4u) << 14) | ((bg & 8u) << 21);
    } else {
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
            if (p0 + j < hw) bp[j] = (unsigned char)((bg >> j) & 1u);
    }
    int below, t0, t1;
    wave_rank(m0, below, t0);
    wave_rank(m1, below, t1);
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wave_counts[0][wave] = t0;
        wave_counts[1][wave] = t1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
        for (int k = 0; k < kWaves; ++k) s += wave_counts[threadIdx.x][k];
        A.work[((size_t)b * 2 + threadIdx.x) * A.tiles + tile] = s;
    }
}

// One class of the placing launch: the slot rule for the thread's pixels of mask m, whose first one has rank `rank` among the
// n pixels of the class; the workgroup that holds rank 0 pads a short cloud, tile 0 zeroes an empty one.  before / in_tile / n
// are uniform over the workgroup, so the barrier is reached by all of its threads or by none.
__device__ __forceinline__ void place(float *cloud, int cap, int n, int before, int in_tile, int rank, unsigned m, const float (&x)[4],
                                      const float (&y)[4], const float (&z)[4], float (&first)[3], int tile) {
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        if (!((m >> j) & 1u)) continue;
        long slot = rank;
        bool keep = true;
        if (n > cap) {  // floor((r + 1) cap / n) > floor(r cap / n)  <=>  the remainder of r cap / n reaches n - cap
            const long rc = (long)rank * cap;
            slot = rc / n;
            keep = rc - slot * n + cap >= n;
        }
        if (keep && (unsigned long)slot < (unsigned long)cap) {
            cloud[3 * slot] = x[j];
            cloud[3 * slot + 1] = y[j];
            cloud[3 * slot + 2] = z[j];
        }
        if (rank == 0) {
            first[0] = x[j]; first[1] = y[j]; first[2] = z[j];
        }
        ++rank;
    }
    if (n < cap && ((n == 0 && tile == 0) || (before == 0 && in_tile > 0))) {
        if (n == 0 && threadIdx.x == 0) first[0] = first[1] = first[2] = 0.f;
        __syncthreads();
        for (int s = n + threadIdx.x; s < cap; s += kThreads) {
            cloud[3 * s] = first[0];
            cloud[3 * s + 1] = first[1];
            cloud[3 * s + 2] = first[2];
        }
    }
}

template <typename D>
__global__ __launch_bounds__(kThreads) void depth_place_kernel(const Args A) {
    __shared__ int sums[kWaves][4], wave_counts[2][kWaves];
    __shared__ float first[2][3];
    const int tile = blockIdx.x, b = blockIdx.y, p0 = tile * kTile + threadIdx.x * kPerThread;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    // the class counts of the tiles before this one, and of all tiles
    const int *tc0 = A.work + (size_t)b * 2 * A.tiles, *tc1 = tc0 + A.tiles;
    int bef0 = 0, bef1 = 0, n0 = 0, n1 = 0;
    for (int t = threadIdx.x; t < A.tiles; t += kThreads) {
        const int c0 = tc0[t], c1 = tc1[t];
        n0 += c0;
        n1 += c1;
        if (t < tile) {
            bef0 += c0;
            bef1 += c1;
        }
    }
    bef0 = wave_sum_i32(bef0); bef1 = wave_sum_i32(bef1); n0 = wave_sum_i32(n0); n1 = wave_sum_i32(n1);
    float x[4], y[4], z[4];
    unsigned m0, m1, bg;
    classify<D>(A, b, p0, x, y, z, m0, m1, bg);
    int below0, below1, t0, t1;
    wave_rank(m0, below0, t0);
    wave_rank(m1, below1, t1);
    if (lane == 0) {
        sums[wave][0] = bef0; sums[wave][1] = bef1; sums[wave][2] = n0; sums[wave][3] = n1;
        wave_counts[0][wave] = t0;
        wave_counts[1][wave] = t1;
    }
    __syncthreads();
    bef0 = bef1 = n0 = n1 = 0;
    int off0 = 0, off1 = 0, in0 = 0, in1 = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        bef0 += sums[k][0]; bef1 += sums[k][1]; n0 += sums[k][2]; n1 += sums[k][3];
        if (k < wave) {
            off0 += wave_counts[0][k];
            off1 += wave_counts[1][k];
        }
        in0 += wave_counts[0][k];
        in1 += wave_counts[1][k];
    }
    if (tile == 0 && threadIdx.x == 0) {
        A.counts[2 * b] = n0;
        A.counts[2 * b + 1] = n1;
    }
    float *cloud = A.clouds + (size_t)b * 2 * A.cap * 3;
    place(cloud, A.cap, n0, bef0, in0, bef0 + off0 + below0, m0, x, y, z, first[0], tile);
    place(cloud + (size_t)A.cap * 3, A.cap, n1, bef1, in1, bef1 + off1 + below1, m1, x, y, z, first[1], tile);
}

}  // namespace dframe
}  // namespace pn2

using namespace pn2;
using namespace pn2::dframe;

static_assert(sizeof(pn2x_depth_frame) == 144, "record layout (pn2_ext.h)");

static void check_geometry(int b, int h, int w, int hs, int ws, int c, int cap, Faults &f) {
    check_image_pair(b, h, w, hs, ws, c, f);
    f.inval |= cap < 1;
    f.range |= cap > 16384;
}

extern "C" int pn2x_depth_frame_supported(int h, int w, int hs, int ws, int c, int cap) {
    Faults f;
    check_geometry(0, h, w, hs, ws, c, cap, f);
    return f.code() == PN2_OK ? 1 : 0;
}

static inline long tiles_of(int h, int w) { return ((long)h * w + kTile - 1) / kTile; }

extern "C" long pn2x_depth_frame_work_ints(int b, int h, int w) {
    return (b < 0 || h < 1 || w < 1) ? (long)PN2_EINVAL : 2L * b * tiles_of(h, w);
}

extern "C" int pn2x_depth_frame_clouds(const pn2x_depth_frame *frames, void *stream) {
    if (!frames) return PN2_ENULL;
    const pn2x_depth_frame &r = *frames;
    Faults f;
    check_geometry(r.b, r.h, r.w, r.hs, r.ws, r.c, r.cap, f);
    // (b may be 0, and depth_scale is not looked at: a scale the decoding cannot use is the caller's own)
    f.inval |= r.b < 0 || (r.depth_u16 != 0 && r.depth_u16 != 1) || (r.flip_yz != 0 && r.flip_yz != 1);
    for (int k = 0; k < 2; ++k) {
        check_class(r.channel[k], r.value[k], r.c, f);
        f.inval |= !(r.radius[k] > 0.f);
    }
    if (r.b != 0)
        f.null |= !r.depth || !r.seg || !r.intrinsics || !r.centre[0] || !r.centre[1] || !r.clouds || !r.counts || !r.background || !r.work;
    if (f.code() != PN2_OK || r.b == 0) return f.code();
    Args A;
    A.depth = r.depth; A.intrinsics = r.intrinsics; A.centre0 = r.centre[0]; A.centre1 = r.centre[1];
    A.clouds = r.clouds; A.counts = r.counts; A.background = r.background; A.work = r.work; A.depth_scale = r.depth_scale;
    A.class0 = seg_map(r.seg, r.h, r.hs, r.ws, r.c, r.channel[0], r.value[0]);
    A.class1 = seg_map(r.seg, r.h, r.hs, r.ws, r.c, r.channel[1], r.value[1]);
    A.h = r.h; A.w = r.w; A.cap = r.cap; A.tiles = (int)tiles_of(r.h, r.w); A.flip = r.flip_yz;
    A.radius0 = r.radius[0]; A.radius1 = r.radius[1];
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(A.tiles, r.b), block(kThreads);
    if (r.depth_u16) {
        hipLaunchKernelGGL(depth_classify_kernel<unsigned short>, grid, block, 0, st, A);
        hipLaunchKernelGGL(depth_place_kernel<unsigned short>, grid, block, 0, st, A);
    } else {
        hipLaunchKernelGGL(depth_classify_kernel<float>, grid, block, 0, st, A);
        hipLaunchKernelGGL(depth_place_kernel<float>, grid, block, 0, st, A);
    }
    return check_launch();
}
