// sdf.hip -- the particle optimisers' signed-distance-volume lookups (include/pn2_sdf.h).
//
// Gather-bound work: every (particle, point) pair costs one 3x3 transform, a few dozen fp32 ops and 8 (trilinear)
// or 1 (nearest) reads of a 2-byte voxel.  The volume (201^3 fp16 = 16 MB) and the cloud (N x 12 B) are shared by
// all particles and stay in L2 / Infinity Cache; nothing of size P x N is ever written.  One workgroup per
// particle (P = 2048..5120 >> 256 CUs), 256 threads striding over the points, one block reduction per particle.
//
// Arithmetic follows the reference's torch expressions operation for operation (fp32, true division, same
// association; compiled with -ffp-contract=off), so Distance() is bit-identical to the reference.
#include "frame_device.h"
#include "sdf_device.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {

struct SdfVol {
    const void *p;
    int res;
    float bbox_min, stride, lo, hi;
};

// One point of gf_optimize_obj.Distance (optimization_obj.py:184-228), in three steps so that callers can issue
// the gathers of several points before blending any of them (the kernel is gather-latency bound).
struct TriPoint {
    int i000;
    float x, y, z;  // fractional parts
};

__device__ __forceinline__ TriPoint tri_setup(const SdfVol &A, float vx, float vy, float vz) {
    const float top = (float)(A.res - 1);
    // torch.clamp: a NaN coordinate stays NaN -- its cell is 0, its fraction and so the value NaN
    const float x = clampf((vx - A.bbox_min) / A.stride, 0.0f, top);
    const float y = clampf((vy - A.bbox_min) / A.stride, 0.0f, top);
    const float z = clampf((vz - A.bbox_min) / A.stride, 0.0f, top);
    TriPoint t;
    const int xi = cell_split(x, t.x), yi = cell_split(y, t.y), zi = cell_split(z, t.z);
    t.i000 = cell_index(xi, yi, zi, A.res);
    return t;
}

#ifndef SDF_PAIR
#define SDF_PAIR 1
#endif
#ifndef SDF_U
#define SDF_U 1  /* measured: 1, 2, 4 within 1% once SDF_PAIR is on (profiles/r01_sdf_sweep.txt) */
#endif

// Two z-adjacent voxels (i, i+1) with ONE load: the kernel is bound by the number of divergent gather lanes the
// texture-address path has to process, and z-neighbours are adjacent in memory (2-byte aligned only: memcpy lets
// the compiler pick an unaligned dword load, which gfx950 global memory supports).
template <int FMT>
__device__ __forceinline__ void vol_pair(const void *v, int i, float &a, float &b) {
    if constexpr (FMT & 1) {
        unsigned w;
        __builtin_memcpy(&w, reinterpret_cast<const __half *>(v) + i, 4);
        a = __half2float(__ushort_as_half((unsigned short)(w & 0xffffu)));
        b = __half2float(__ushort_as_half((unsigned short)(w >> 16)));
    } else {
        float2 w;
        __builtin_memcpy(&w, reinterpret_cast<const float *>(v) + i, 8);
        a = w.x;
        b = w.y;
    }
}

template <int FMT>
__device__ __forceinline__ void tri_gather(const SdfVol &A, const TriPoint &t, float *d) {
    const int R = A.res, RR = R * R, last = RR * R - 1, i = t.i000;
    if constexpr (FMT >= 2) {
        ld_corner_cell<FMT == 3>(A.p, i, d);
        return;
    }
    if (SDF_PAIR && i + 1 + R + RR <= last) {  // everywhere except the volume's last corner
        vol_pair<FMT>(A.p, i, d[0], d[1]);
        vol_pair<FMT>(A.p, i + R, d[2], d[3]);
        vol_pair<FMT>(A.p, i + RR, d[4], d[5]);
        vol_pair<FMT>(A.p, i + R + RR, d[6], d[7]);
        return;
    }
    // the reference clamps each corner index to [0, res^3 - 1] (:215-222); only the upper clamp can bind
    constexpr bool kF16 = (FMT & 1) != 0;
    d[0] = ld_vol<kF16>(A.p, i);                         d[1] = ld_vol<kF16>(A.p, min(i + 1, last));
    d[2] = ld_vol<kF16>(A.p, min(i + R, last));          d[3] = ld_vol<kF16>(A.p, min(i + 1 + R, last));
    d[4] = ld_vol<kF16>(A.p, min(i + RR, last));         d[5] = ld_vol<kF16>(A.p, min(i + 1 + RR, last));
    d[6] = ld_vol<kF16>(A.p, min(i + R + RR, last));     d[7] = ld_vol<kF16>(A.p, min(i + 1 + R + RR, last));
}

__device__ __forceinline__ float tri_blend(const SdfVol &A, const TriPoint &t, const float *d) {
    return clampf(cell_blend(d, t.x, t.y, t.z), A.lo, A.hi);  // :223-227
}

template <int FMT>
__device__ __forceinline__ float trilinear(const SdfVol &A, float vx, float vy, float vz) {
    const TriPoint t = tri_setup(A, vx, vy, vz);
    float d[8];
    tri_gather<FMT>(A, t, d);
    return tri_blend(A, t, d);
}

__device__ __forceinline__ float block_sum_256(float v, float *sm) {  // sm: >= 4 floats of LDS; all threads get the sum
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

template <int FMT>
__global__ void __launch_bounds__(256) sdf_trilinear_kernel(int m, const float *__restrict__ V, SdfVol A, float *__restrict__ out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256)
        out[i] = trilinear<FMT>(A, V[3 * i], V[3 * i + 1], V[3 * i + 2]);
}

// mean_j |Distance((pcld_j - t) @ R)| for the calling block's particle; every thread returns the value.
template <int FMT>
__device__ __forceinline__ float particle_sdf_energy(int n, const float *__restrict__ pcld, const float *R, const float *t,
                                                     const SdfVol &A, float *sm) {
    constexpr int U = SDF_U;  // points per thread whose gathers are all issued before any blend
    float acc = 0.0f;
    for (int j0 = threadIdx.x; j0 < n; j0 += 256 * U) {
        TriPoint tp[U];
        float d[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = min(j0 + 256 * u, n - 1);  // out-of-range slots re-read the last point and are masked below
            float ox, oy, oz;
            to_object_frame(pcld[3 * j], pcld[3 * j + 1], pcld[3 * j + 2], t, R, ox, oy, oz);
            tp[u] = tri_setup(A, ox, oy, oz);
            tri_gather<FMT>(A, tp[u], d[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float v = fabsf(tri_blend(A, tp[u], d[u]));
            acc += (j0 + 256 * u < n) ? v : 0.0f;
        }
    }
    return block_sum_256(acc, sm) / (float)n;
}

template <int FMT>
__global__ void __launch_bounds__(256)
sdf_particle_energy_kernel(int n, const float *__restrict__ pcld, const float *__restrict__ rot, const float *__restrict__ trans,
                           SdfVol A, float *__restrict__ sdf_energy) {
    __shared__ float sm[4];
    const int i = blockIdx.x;
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rot[9 * i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = trans[3 * i + k];
    const float e = particle_sdf_energy<FMT>(n, pcld, R, t, A, sm);
    if (threadIdx.x == 0) sdf_energy[i] = e;
}

// ---- gf_optimize_obj.optimize's particle loop (optimization_obj.py:253-301) ----------------------------------------
// work layout (floats): [0..5] search size, [6..11] previous search size, [12] previous-success flag,
// [13] "previous search size is still the Python scalar c1" flag, [14] ticket counter (u32), [15] pad,
// [16 .. 16+p) per-particle sdf_energy.
constexpr int W_SEARCH = 0, W_PREV = 6, W_PREV_OK = 12, W_PREV_SCALAR = 13, W_TICKET = 14, W_ENERGY = 16;

// sample = [qw, pre*search] (:259-261)
__device__ __forceinline__ void particle_sample(const float *__restrict__ pre, int i, const float *search, float *s) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[1 + k] = pre[6 * i + k] * search[k];
    s[0] = sqrtf(1.0f - s[1] * s[1] - s[2] * s[2] - s[3] * s[3]);
}

// Grid (p, problems): workgroup (i, k) is particle i of problem k.  Problem k owns the work record at work + k * work_stride (the
// layout above; a batch pads it to a multiple of 16 floats), poses[12k .. 12k+12) and -- in a batch -- its slice of the packed cloud
// and vols[k] (problem_slice, sdf_device.h).  Nothing is shared between problems but read-only inputs, and the last workgroup of
// problem k is decided by problem k's own ticket: no workgroup ever waits for another, of its own problem or of any other.
struct OptArgs {
    int p, n, work_stride;     // n: the single entry's cloud
    const float *pcld, *pre;
    const int *cloud_off;      // batch: (problems + 1) offsets in points; NULL for the single entry
    const void *const *vols;   // batch; the single entry's volume is V.p
    SdfVol V;
    float c2, beta, one_minus_beta, carry0;
    float *poses, *work;
};

constexpr int opt_work_stride(int p) { return (W_ENERGY + p + 15) / 16 * 16; }

__global__ void opt_init_kernel(float *work, int work_stride, float c1) {
    float *w = work + (size_t)blockIdx.x * work_stride;
    const int t = threadIdx.x;
    if (t < 12) w[t] = c1;  // W_SEARCH, W_PREV
    if (t == 12) w[W_PREV_OK] = 1.0f;
    if (t == 13) w[W_PREV_SCALAR] = 1.0f;
    if (t == 14) reinterpret_cast<unsigned *>(w)[W_TICKET] = 0u;
}

// One workgroup's share of one iteration of one problem (its n points at pcld, its volume V.p, its pose and work records):
// particle i's evaluation, then -- in the workgroup that draws the problem's last ticket -- the pose / search-size update.  The one
// body of both entries, so a problem of a batch accumulates in the single entry's order and agrees with it in every bit.
template <int FMT>
__device__ __forceinline__ void obj_optimize_block(const OptArgs &A, const int n, const float *__restrict__ pcld, const SdfVol &V,
                                                   float *pose, float *__restrict__ work, const int i) {
    __shared__ float sm[4];
    __shared__ float red[9 * 4 + 4];
    __shared__ int is_last;
    const int tid = threadIdx.x;
    float *__restrict__ energy = work + W_ENERGY;

    float search[6], R0[9], t0[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) search[k] = work[W_SEARCH + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) R0[k] = pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t0[k] = pose[9 + k];
    {
        float s[7], S[9], R[9], t[3];
        particle_sample(A.pre, i, search, s);
        quat_to_matrix(s[0], s[1], s[2], s[3], S);
        mat3_mul(R0, S, R);  // :263
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = t0[k] + s[4 + k];  // :264
        const float e = particle_sdf_energy<FMT>(n, pcld, R, t, V, sm);
        // agent-scope (write-through) store: visible to every XCD without an L2 write-back
        if (tid == 0) __hip_atomic_store(&energy[i], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- the last workgroup to finish performs the pose / search-size update of this iteration --------------------
    // No fences: a release/acquire pair at agent scope costs an L2 write-back / invalidate per workgroup on this
    // multi-XCD part (measured: 163 us per iteration instead of ~40, the shared volume keeps being evicted).
    // Instead energy[] is written and read with agent-scope atomics (coherent per location), and the store is
    // complete (vmcnt(0)) before this workgroup takes its ticket, so whoever draws the last ticket sees them all.
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(reinterpret_cast<unsigned *>(work) + W_TICKET, 1u, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        is_last = (ticket == (unsigned)A.p - 1u);
    }
    __syncthreads();
    if (!is_last) return;

    const float origin_sdf = __hip_atomic_load(&energy[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float origin = origin_sdf * 500.0f;  // :236
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
    int any = 0;
    // one workgroup walks all p energies: issue 8 independent loads per thread before using any (a dependent
    // load-use chain per particle made this tail ~15 us of a ~40 us iteration)
    constexpr int UQ = 8;
    for (int q0 = tid; q0 < A.p; q0 += 256 * UQ) {
        float se[UQ], pr[UQ][6];
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
            const int q = min(q0 + 256 * u, A.p - 1);
            se[u] = __hip_atomic_load(&energy[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 6; ++k) pr[u][k] = A.pre[6 * q + k];
        }
#pragma unroll
        for (int u = 0; u < UQ; ++u) {
            if (q0 + 256 * u >= A.p) continue;
            const float en = se[u] * 500.0f;
            const bool better = en < origin;  // :271
            const float w = better ? origin - en : 0.0f;
            any |= better;
            float s[7];
#pragma unroll
            for (int k = 0; k < 6; ++k) s[1 + k] = pr[u][k] * search[k];  // == particle_sample
            s[0] = sqrtf(1.0f - s[1] * s[1] - s[2] * s[2] - s[3] * s[3]);
            acc[0] += w;
            acc[1] += se[u] * w;
#pragma unroll
            for (int k = 0; k < 7; ++k) acc[2 + k] += s[k] * w;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
        if ((tid & 63) == 0) red[k * 4 + (tid >> 6)] = v;
    }
    const unsigned long long any_b = __ballot(any);
    if ((tid & 63) == 0) red[36 + (tid >> 6)] = any_b ? 1.0f : 0.0f;
    __syncthreads();
    if (tid != 0) return;

    float sum[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = (red[k * 4] + red[k * 4 + 1]) + (red[k * 4 + 2] + red[k * 4 + 3]);
    const bool success = (red[36] + red[37] + red[38] + red[39]) > 0.0f;
    const float wsum = sum[0] + 1e-5f;  // :273
    float mean_sdf, mt[7];
    if (success) {
        mean_sdf = sum[1] / wsum;  // :275
#pragma unroll
        for (int k = 0; k < 7; ++k) mt[k] = sum[2 + k] / wsum;  // :283
        const float qn = sqrtf(mt[0] * mt[0] + mt[1] * mt[1] + mt[2] * mt[2] + mt[3] * mt[3]) + 1e-8f;
#pragma unroll
        for (int k = 0; k < 4; ++k) mt[k] /= qn;  // :284
        float S[9], Rn[9];
        quat_to_matrix(mt[0], mt[1], mt[2], mt[3], S);
        mat3_mul(R0, S, Rn);  // :285
        // SO(3) re-projection: Gram-Schmidt on the first two ROWS (:287, rotations.py:356-369 + transpose)
        float x[3] = {Rn[0], Rn[1], Rn[2]}, yr[3] = {Rn[3], Rn[4], Rn[5]}, z[3], y[3];
        normalize3(x);
        z[0] = x[1] * yr[2] - x[2] * yr[1]; z[1] = x[2] * yr[0] - x[0] * yr[2]; z[2] = x[0] * yr[1] - x[1] * yr[0];
        normalize3(z);
        y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pose[k] = x[k];
            pose[3 + k] = y[k];
            pose[6 + k] = z[k];
            pose[9 + k] = t0[k] + mt[4 + k];  // :288
        }
    } else {
        mean_sdf = origin_sdf;  // :278
#pragma unroll
        for (int k = 0; k < 7; ++k) mt[k] = 0.0f;
    }
    // update_seach_size (:239-242) and its smoothing (:293-299)
    float s[6], nrm = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        s[k] = fabsf(mt[1 + k]) + 1e-3f;
        nrm += s[k] * s[k];
    }
    nrm = sqrtf(nrm);
    const bool prev_ok = work[W_PREV_OK] != 0.0f, prev_scalar = work[W_PREV_SCALAR] != 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float ns = mean_sdf * A.c2 * s[k] / nrm + 1e-3f;
        if (prev_ok && success) {
            const float carry = prev_scalar ? A.carry0 : A.one_minus_beta * work[W_PREV + k];
            ns = A.beta * ns + carry;
        }
        work[W_SEARCH + k] = ns;
        if (success) work[W_PREV + k] = ns;
    }
    if (success) work[W_PREV_SCALAR] = 0.0f;
    work[W_PREV_OK] = success ? 1.0f : 0.0f;
    reinterpret_cast<unsigned *>(work)[W_TICKET] = 0u;
}

template <int FMT>
__global__ void __launch_bounds__(256) obj_optimize_kernel(const OptArgs A) {
    const int k = blockIdx.y;
    int n = A.n;
    const float *pcld = A.pcld;
    SdfVol V = A.V;
    if (A.cloud_off && !problem_slice(A.cloud_off, A.vols, k, pcld, n, V.p)) return;
    obj_optimize_block<FMT>(A, n, pcld, V, A.poses + 12 * (size_t)k, A.work + (size_t)k * A.work_stride, blockIdx.x);
}

// ---- gf_optimize_hand_pose.query_sdf (+ get_penetration_loss) (optimization_hand.py:252-268) -----------------------
// (index arithmetic: div_floor / nearest_voxel in sdf_device.h, shared with hand_pose.hip)
template <bool F16>
__global__ void __launch_bounds__(256)
sdf_nearest_kernel(int n, const float *__restrict__ hand, const float *__restrict__ obj_r, const float *__restrict__ obj_t,
                   const void *__restrict__ vol, int res, float voxel_scale, int *__restrict__ out_idx,
                   void *__restrict__ out_sdf, void *__restrict__ out_pen) {
    __shared__ float sm[4];
    const int b = blockIdx.x;
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = obj_r[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = obj_t[k];
    float pen = 0.0f;
    constexpr int U = 4;
    for (int j0 = threadIdx.x; j0 < n; j0 += 256 * U) {
        int flat[U];
        float v[U];
        __half h[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t e = (size_t)b * n + min(j0 + 256 * u, n - 1);
            float ox, oy, oz;
            to_object_frame(hand[3 * e], hand[3 * e + 1], hand[3 * e + 2], t, R, ox, oy, oz);
            flat[u] = nearest_voxel(ox, oy, oz, voxel_scale, res);
            if constexpr (F16) h[u] = reinterpret_cast<const __half *>(vol)[flat[u]];
            else v[u] = reinterpret_cast<const float *>(vol)[flat[u]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (j0 + 256 * u >= n) continue;
            const size_t e = (size_t)b * n + j0 + 256 * u;
            if (out_idx) out_idx[e] = flat[u];
            if constexpr (F16) {
                if (out_sdf) reinterpret_cast<__half *>(out_sdf)[e] = h[u];
                v[u] = __half2float(h[u]);
            } else {
                if (out_sdf) reinterpret_cast<float *>(out_sdf)[e] = v[u];
            }
            if (v[u] < 0.0f) pen = fmaxf(pen, -v[u]);
        }
    }
    if (!out_pen) return;
#pragma unroll
    for (int o = 32; o; o >>= 1) pen = fmaxf(pen, __shfl_down(pen, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = pen;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        if constexpr (F16) reinterpret_cast<__half *>(out_pen)[b] = __float2half(m);  // exact: m is a half value
        else reinterpret_cast<float *>(out_pen)[b] = m;
    }
}

// Corner layout: cell i = the eight corner values the reference's Distance() fetches when i000 == i, with ITS index
// arithmetic (flat +1 / +R / +R^2 offsets, each clamped to the last element, optimization_obj.py:206-222), so a
// lookup through this layout is bit-identical to one through the linear volume for every input.
template <bool F16>
__global__ void __launch_bounds__(256) corner_volume_kernel(const void *__restrict__ vol, int res, void *__restrict__ out) {
    const int R = res, RR = R * R, last = RR * R - 1;
    for (int i = blockIdx.x * 256 + threadIdx.x; i <= last; i += gridDim.x * 256) {
        const int id[8] = {i, min(i + 1, last), min(i + R, last), min(i + 1 + R, last),
                           min(i + RR, last), min(i + 1 + RR, last), min(i + R + RR, last), min(i + 1 + R + RR, last)};
        if constexpr (F16) {
            const unsigned short *v = reinterpret_cast<const unsigned short *>(vol);
            uint4 w;
            w.x = v[id[0]] | ((unsigned)v[id[1]] << 16);
            w.y = v[id[2]] | ((unsigned)v[id[3]] << 16);
            w.z = v[id[4]] | ((unsigned)v[id[5]] << 16);
            w.w = v[id[6]] | ((unsigned)v[id[7]] << 16);
            reinterpret_cast<uint4 *>(out)[i] = w;
        } else {
            const float *v = reinterpret_cast<const float *>(vol);
            reinterpret_cast<float4 *>(out)[2 * (size_t)i] = make_float4(v[id[0]], v[id[1]], v[id[2]], v[id[3]]);
            reinterpret_cast<float4 *>(out)[2 * (size_t)i + 1] = make_float4(v[id[4]], v[id[5]], v[id[6]], v[id[7]]);
        }
    }
}

// the trilinear entries' grid: res in [2, 1024] (res^3 fits an int), a finite stride > 0
inline bool grid_inval(int res, float stride) { return res < 2 || res > 1024 || !finite_positive(stride); }

}  // namespace pn2

using namespace pn2;

#define SDF_FMT_DISPATCH(fmt, CALL)                   \
    switch (fmt) {                                    \
        case 0: { constexpr int FMT = 0; CALL; } break; \
        case 1: { constexpr int FMT = 1; CALL; } break; \
        case 2: { constexpr int FMT = 2; CALL; } break; \
        case 3: { constexpr int FMT = 3; CALL; } break; \
        default: return PN2_EINVAL;                   \
    }

extern "C" long pn2s_corner_volume_elems(int res) { return (res < 2 || res > 1024) ? (long)PN2_EINVAL : 8L * res * res * res; }

extern "C" int pn2s_build_corner_volume(const void *vol, int vol_f16, int res, void *out, void *stream) {
    if (res < 2 || res > 1024 || (vol_f16 != 0 && vol_f16 != 1)) return PN2_EINVAL;
    if (!vol || !out) return PN2_ENULL;
    const long cells = (long)res * res * res;
    const unsigned blocks = (unsigned)min((cells + 255) / 256, 65536L);
    hipStream_t st = (hipStream_t)stream;
    if (vol_f16) hipLaunchKernelGGL(corner_volume_kernel<true>, dim3(blocks), dim3(256), 0, st, vol, res, out);
    else hipLaunchKernelGGL(corner_volume_kernel<false>, dim3(blocks), dim3(256), 0, st, vol, res, out);
    return check_launch();
}

extern "C" int pn2s_trilinear(int m, const float *V, const void *vol, int vol_fmt, int res, float bbox_min, float stride,
                              float clamp_lo, float clamp_hi, float *out, void *stream) {
    if (m < 0 || grid_inval(res, stride)) return PN2_EINVAL;
    if (m == 0) return (vol_fmt < 0 || vol_fmt > 3) ? PN2_EINVAL : PN2_OK;
    if (!V || !vol || !out) return PN2_ENULL;
    const SdfVol A{vol, res, bbox_min, stride, clamp_lo, clamp_hi};
    const unsigned blocks = (unsigned)min((m + 255) / 256, 16384);
    hipStream_t st = (hipStream_t)stream;
    SDF_FMT_DISPATCH(vol_fmt, hipLaunchKernelGGL(sdf_trilinear_kernel<FMT>, dim3(blocks), dim3(256), 0, st, m, V, A, out))
    return check_launch();
}

extern "C" int pn2s_particle_energy(int p, int n, const float *pcld, const float *rot, const float *trans, const void *vol,
                                    int vol_fmt, int res, float bbox_min, float stride, float clamp_lo, float clamp_hi,
                                    float *sdf_energy, void *stream) {
    if (p < 0 || n < 1 || grid_inval(res, stride)) return PN2_EINVAL;
    if (p == 0) return (vol_fmt < 0 || vol_fmt > 3) ? PN2_EINVAL : PN2_OK;
    if (!pcld || !rot || !trans || !vol || !sdf_energy) return PN2_ENULL;
    const SdfVol A{vol, res, bbox_min, stride, clamp_lo, clamp_hi};
    hipStream_t st = (hipStream_t)stream;
    SDF_FMT_DISPATCH(vol_fmt, hipLaunchKernelGGL(sdf_particle_energy_kernel<FMT>, dim3(p), dim3(256), 0, st, n, pcld, rot, trans, A, sdf_energy))
    return check_launch();
}

extern "C" int pn2s_obj_optimize_work_floats(int p) { return p < 0 ? PN2_EINVAL : W_ENERGY + p; }

extern "C" long pn2s_obj_optimize_batch_work_floats(int s, int p) {
    return (s < 0 || p < 0) ? (long)PN2_EINVAL : (long)s * opt_work_stride(p);
}

static_assert(sizeof(pn2s_obj_opt) == 120, "record layout (pn2_sdf.h)");

// A record pointer is read only if a process can own the address: nothing is mapped below 64 KiB, and the upper half of the
// address space is the kernel's.  A caller built against the positional entries passes its problem or particle count where the
// record is now, and is refused (PN2_EINVAL) instead of read (as hand_check.h's is_record).
static int opt_launch(const pn2s_obj_opt *opt, bool batch, void *stream) {
    if (!opt) return PN2_ENULL;
    if ((intptr_t)opt < 65536) return PN2_EINVAL;
    const pn2s_obj_opt &r = *opt;
    Faults f;
    f.inval = r.problems < 0 || (!batch && (r.problems != 1 || r.n < 1)) || r.p < 1 || r.iterations < 0 || grid_inval(r.res, r.stride);
    f.inval |= r.vol_fmt < 0 || r.vol_fmt > 3;
    f.range = r.problems > PN2S_OPT_BATCH_MAX || r.p > (1 << 20) || (long)r.problems * r.p > (1L << 22);
    if (f.code() != PN2_OK) return f.code();
    if (r.problems == 0) return PN2_OK;
    f.null = !r.pcld || !r.pre_sampled || !r.poses || !r.work || (batch ? (!r.cloud_off || !r.vols) : !r.volume);
    if (f.code() != PN2_OK) return f.code();
    if (r.work_floats < (batch ? pn2s_obj_optimize_batch_work_floats(r.problems, r.p) : (long)pn2s_obj_optimize_work_floats(r.p)))
        return PN2_ESCRATCH;
    OptArgs A;
    A.p = r.p; A.n = r.n; A.work_stride = batch ? opt_work_stride(r.p) : 0;
    A.pcld = r.pcld; A.pre = r.pre_sampled; A.cloud_off = batch ? r.cloud_off : nullptr; A.vols = batch ? r.vols : nullptr;
    A.V = SdfVol{batch ? nullptr : r.volume, r.res, r.bbox_min, r.stride, r.clamp_lo, r.clamp_hi};
    A.c2 = r.c2; A.beta = r.beta;
    // the reference mixes a Python double scalar into fp32 tensors here (:295): (1-beta) is rounded to fp32 when it
    // multiplies a tensor, but (1-beta)*c1 is a double product rounded once while prev_search_size is still c1
    A.one_minus_beta = (float)(1.0 - (double)r.beta);
    A.carry0 = (float)((1.0 - (double)r.beta) * (double)r.c1);
    A.poses = r.poses; A.work = r.work;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(opt_init_kernel, dim3(r.problems), dim3(64), 0, st, r.work, A.work_stride, r.c1);
    for (int it = 0; it < r.iterations; ++it) {
        SDF_FMT_DISPATCH(r.vol_fmt, hipLaunchKernelGGL(obj_optimize_kernel<FMT>, dim3(r.p, r.problems), dim3(256), 0, st, A))
    }
    return check_launch();
}

extern "C" int pn2s_obj_optimize(const pn2s_obj_opt *opt, void *stream) { return opt_launch(opt, false, stream); }

extern "C" int pn2s_obj_optimize_batch(const pn2s_obj_opt *opt, void *stream) { return opt_launch(opt, true, stream); }

extern "C" int pn2s_nearest(int b, int n, const float *hand, const float *obj_r, const float *obj_t, const void *vol,
                            int vol_f16, int res, float voxel_scale, int *out_idx, void *out_sdf, void *out_pen, void *stream) {
    if (b < 0 || n < 1 || res < 1 || res > 1024 || (res & 1) == 0 || !(voxel_scale > 0.0f)) return PN2_EINVAL;
    if (b == 0) return PN2_OK;
    if (!hand || !obj_r || !obj_t || !vol) return PN2_ENULL;
    hipStream_t st = (hipStream_t)stream;
    if (vol_f16) hipLaunchKernelGGL(sdf_nearest_kernel<true>, dim3(b), dim3(256), 0, st, n, hand, obj_r, obj_t, vol, res, voxel_scale, out_idx, out_sdf, out_pen);
    else hipLaunchKernelGGL(sdf_nearest_kernel<false>, dim3(b), dim3(256), 0, st, n, hand, obj_r, obj_t, vol, res, voxel_scale, out_idx, out_sdf, out_pen);
    return check_launch();
}
