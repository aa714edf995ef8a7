// row_chain.hip -- the per-point layers between feature propagation and the keypoint queries, run only over the points
// that a keypoint's kNN list names (eval fast path, network/models/fast_eval.py).
//
// The keypoint branches q1 / q2 read the backbone's per-point features only through the rows their kNN lists name: the
// union of the 21 keypoints' K = 64 lists covers about two thirds of a 1024-point cloud, the K = 16 lists about a quarter.
// Everything from fp1's MLP to the layer-1 feature product of the four q scales is per point, so it runs over those rows
// only, in one launch:
//
//   x = fp1_in[r] = [interp | xyz | pad]                              (132 floats)
//   h1 = relu(Wa x[:128] + We xyz + ba), h2 = relu(Wb h1 + bb)        fp1, both layers (BatchNorm folded)
//   c  = relu(Wc h2 + bc)                                             conv1 + bn1, 128 -> 384
//   out[r, 0:512] = Wq c                                              [q1 s0 | q2 s0 | q1 s1 | q2 s1] layer-1 feature terms
//
// Rows named by a small-K list get all 512 columns, rows named only by a large-K list the last 256 (the large-K scale);
// no other row or column is written.  pn2x_row_lists builds the per-cloud row lists and counts on the device, so the
// row count never reaches the host (graph capture).
//
// Work split: the persistent grid divides the GLOBAL row work (both lists of all clouds, small-K rows weighted 31 : 20 by
// their FLOPs) into equal contiguous shares of 16-row groups; a workgroup runs its share as tiles of up to 64 rows.
// Per tile, all four layers on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32) with the activations in LDS
// and the weights streamed from L2 straight into registers (the shared core and its layouts: mfma_rows.h).
#include "pn2_common.h"
#include "mfma_rows.h"
#include "../../include/pn2_ext.h"

namespace pn2 {
namespace rchain {

using mrows::f32x4;
using mrows::init_bias;
using mrows::mm;
using mrows::relu_to_lds;

constexpr int CH = 128, CC = 384, CQ = 512;  // fp1 width, conv1 width, the four scales' layer-1 width
constexpr int KX = 144;                      // fp1 layer 1: 128 features + 3 coordinates, zero-padded to 9 k-groups of 16
constexpr int XQ = 33;                       // 16-byte quads of an input row that hold data (132 floats)
// LDS row strides: = 8 (mod 64) floats keeps the 16-byte operand reads (16 rows x 4 k-quads per lane group) conflict-free
constexpr int LDX = 152, LDH = 136, LDC = 392;
constexpr int MAXB = 1024;
constexpr int GROUP_COST_SMALL = 31, GROUP_COST_LARGE = 20;  // 557 vs 361 kFLOP per row

struct ChainArgs {
    int B, N, ldx, ldo;
    const float *x;
    const int *list, *counts;
    const float *wa, *ba, *wb, *bb, *wc, *bc, *wq;
    float *out;
};

struct Smem {
    int *rows;       // [64] global row (b * N + point) of each tile row, -1 past the end
    int *p_small;    // [B + 1] prefix sums of the per-cloud small-K row counts
    int *p_large;    // [B + 1] ... of the large-K-only row counts
    float *r1;       // input rows (LDX), later h2 (LDH)
    float *r2;       // h1 (LDH), later conv1's output (LDC)
};

// dynamic LDS of a launch over `clouds` clouds: r1, r2, rows, both prefix arrays, the scan's [2][256]
constexpr size_t lds_bytes(int clouds) {
    return (size_t)64 * (LDX + LDC) * sizeof(float) + (size_t)(64 + 2 * (clouds + 1) + 512) * sizeof(int);
}

// row e of list `seq` (0 = small-K rows, 1 = large-K-only rows) -> global row index
__device__ __forceinline__ int lookup(const ChainArgs &A, const Smem &S, int seq, int e) {
    const int *P = seq ? S.p_large : S.p_small;
    int lo = 0, hi = A.B;  // largest b with P[b] <= e
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P[mid] <= e) lo = mid; else hi = mid;
    }
    const int off = seq ? (S.p_small[lo + 1] - S.p_small[lo]) : 0;
    return lo * A.N + A.list[(size_t)lo * A.N + off + (e - P[lo])];
}

// one tile: rows e0 .. e0 + cnt - 1 (cnt <= 16 MT) of list `seq`.  H1IN: the input rows are h1 itself (CH floats, already
// activated: pn2x_row_chain3) and the tile starts at fp1's second layer.
template <int MT, bool H1IN>
__device__ void tile(const ChainArgs &A, const Smem &S, int seq, int e0, int cnt) {
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int R = MT * 16;
    if (tid < R) S.rows[tid] = tid < cnt ? lookup(A, S, seq, e0 + tid) : -1;
    __syncthreads();
    if constexpr (H1IN) {
        // h1 rows -> LDS where layer 1 would have left them, zero for rows past the end (those read row 0: no load in a branch)
        for (int i = tid; i < R * (CH / 4); i += 256) {
            const int r = i / (CH / 4), q = i - r * (CH / 4);
            const int g = S.rows[r];
            const f32x4 v = *reinterpret_cast<const f32x4 *>(A.x + (size_t)(g < 0 ? 0 : g) * A.ldx + 4 * q);
            *reinterpret_cast<f32x4 *>(S.r2 + r * LDH + 4 * q) = g < 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : v;
        }
    } else {
        // input rows -> LDS, zero past column 131 (the row's pad float may hold anything) and for rows past the end
        for (int i = tid; i < R * (KX / 4); i += 256) {
            const int r = i / (KX / 4), q = i - r * (KX / 4);
            const int g = S.rows[r];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (g >= 0 && q < XQ) {
                v = *reinterpret_cast<const f32x4 *>(A.x + (size_t)g * A.ldx + 4 * q);
                if (q == XQ - 1) v.w = 0.f;
            }
            *reinterpret_cast<f32x4 *>(S.r1 + r * LDX + 4 * q) = v;
        }
        __syncthreads();
        // fp1 layer 1: 144 -> 128, two n-tiles per wave
        f32x4 acc[2][MT];
        init_bias(acc, A.ba, 2 * w, lane);
        mm<2, MT, KX / 16, LDX>(acc, A.wa + (size_t)(2 * w) * (KX / 16) * 256, S.r1, lane);
        relu_to_lds(acc, S.r2, LDH, 2 * w, lane);
    }
    __syncthreads();
    {  // fp1 layer 2: 128 -> 128 (h2 over the input rows)
        f32x4 acc[2][MT];
        init_bias(acc, A.bb, 2 * w, lane);
        mm<2, MT, CH / 16, LDH>(acc, A.wb + (size_t)(2 * w) * (CH / 16) * 256, S.r2, lane);
        relu_to_lds(acc, S.r1, LDH, 2 * w, lane);
    }
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {  // conv1: 128 -> 384, 24 n-tiles = 2 passes x 4 waves x 3
        const int nt0 = (p * 4 + w) * 3;
        f32x4 acc[3][MT];
        init_bias(acc, A.bc, nt0, lane);
        mm<3, MT, CH / 16, LDH>(acc, A.wc + (size_t)nt0 * (CH / 16) * 256, S.r1, lane);
        relu_to_lds(acc, S.r2, LDC, nt0, lane);
    }
    __syncthreads();
    // layer-1 feature product of the four scales: 384 -> 512 (small-K rows) or the last 256 columns (large-K-only rows)
    const int np = seq ? 1 : 2;
#pragma unroll 1
    for (int p = 0; p < np; ++p) {
        const int nt0 = (seq ? 16 : 0) + (p * 4 + w) * 4;
        f32x4 acc[4][MT];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mm<4, MT, CC / 16, LDC>(acc, A.wq + (size_t)nt0 * (CC / 16) * 256, S.r2, lane);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int g = S.rows[mt * 16 + (lane & 15)];
            if (g < 0) continue;
            float *o = A.out + (size_t)g * A.ldo + nt0 * 16 + 4 * (lane >> 4);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<f32x4 *>(o + nt * 16) = acc[nt][mt];
        }
    }
    __syncthreads();  // rows[] and the LDS images are rewritten by the next tile
}

// run rows [e_lo, e_hi) of list `seq` as tiles of up to 64 rows
template <bool H1IN>
__device__ void run_rows(const ChainArgs &A, const Smem &S, int seq, int e_lo, int e_hi) {
    for (int e0 = e_lo; e0 < e_hi; e0 += 64) {
        const int cnt = e_hi - e0 < 64 ? e_hi - e0 : 64;
        switch ((cnt + 15) >> 4) {
            case 1: tile<1, H1IN>(A, S, seq, e0, cnt); break;
            case 2: tile<2, H1IN>(A, S, seq, e0, cnt); break;
            case 3: tile<3, H1IN>(A, S, seq, e0, cnt); break;
            default: tile<4, H1IN>(A, S, seq, e0, cnt); break;
        }
    }
}

// the launch: the counts' prefix sums, this workgroup's share of both lists, its tiles
template <bool H1IN>
__device__ __forceinline__ void chain(const ChainArgs &A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = (int)threadIdx.x;
    Smem S;
    S.r1 = smem;
    S.r2 = smem + 64 * LDX;
    S.rows = reinterpret_cast<int *>(S.r2 + 64 * LDC);
    S.p_small = S.rows + 64;
    S.p_large = S.p_small + (A.B + 1);
    int *scan = S.p_large + (A.B + 1);  // [2][256]
    // prefix sums of the per-cloud counts, 256 clouds at a time (Hillis-Steele in LDS)
    int carry_s = 0, carry_l = 0;
    if (tid == 0) { S.p_small[0] = 0; S.p_large[0] = 0; }
    for (int base = 0; base < A.B; base += 256) {
        const int b = base + tid;
        int cs = 0, cl = 0;
        if (b < A.B) {
            cs = A.counts[2 * b];
            cl = A.counts[2 * b + 1] - cs;
        }
        for (int d = 1; d < 256; d <<= 1) {
            scan[tid] = cs; scan[256 + tid] = cl;
            __syncthreads();
            if (tid >= d) { cs += scan[tid - d]; cl += scan[256 + tid - d]; }
            __syncthreads();
        }
        if (b < A.B) { S.p_small[b + 1] = carry_s + cs; S.p_large[b + 1] = carry_l + cl; }
        scan[tid] = cs; scan[256 + tid] = cl;
        __syncthreads();
        carry_s += scan[255]; carry_l += scan[511];
        __syncthreads();
    }
    const int n_small = carry_s, n_large = carry_l;
    // this workgroup's share of the weighted 16-row groups
    const long g_small = (n_small + 15) / 16, g_large = (n_large + 15) / 16;
    const long total = GROUP_COST_SMALL * g_small + GROUP_COST_LARGE * g_large;
    const long lo = total * blockIdx.x / gridDim.x, hi = total * (blockIdx.x + 1) / gridDim.x;
    auto first_at = [](long c, long cost) { return c <= 0 ? 0L : (c + cost - 1) / cost; };  // first group starting at >= c
    long s0 = first_at(lo, GROUP_COST_SMALL), s1 = first_at(hi, GROUP_COST_SMALL);
    s0 = s0 < g_small ? s0 : g_small; s1 = s1 < g_small ? s1 : g_small;
    const long cs_end = GROUP_COST_SMALL * g_small;
    long l0 = first_at(lo - cs_end, GROUP_COST_LARGE), l1 = first_at(hi - cs_end, GROUP_COST_LARGE);
    l0 = l0 < g_large ? l0 : g_large; l1 = l1 < g_large ? l1 : g_large;
    auto clip = [](long e, int n) { return (int)(e < n ? e : n); };
    run_rows<H1IN>(A, S, 0, clip(16 * s0, n_small), clip(16 * s1, n_small));
    run_rows<H1IN>(A, S, 1, clip(16 * l0, n_large), clip(16 * l1, n_large));
}

__global__ __launch_bounds__(256, 1) void row_chain_kernel(ChainArgs A) { chain<false>(A); }

// pn2x_row_chain3: the same lists, shares, tiles and layers from fp1's second layer on, over rows that already hold h1
__global__ __launch_bounds__(256, 1) void row_chain3_kernel(ChainArgs A) { chain<true>(A); }

// ---- per-cloud row lists -------------------------------------------------------------------------------------------------
// One workgroup per cloud: bitmaps of the points named by the small-K lists and by either list (LDS, one bit per point),
// then a block scan of the per-thread popcounts places every point: small-K rows ascending, then the other rows ascending.
constexpr int RL_MAXN = 16384;

__global__ __launch_bounds__(256) void row_lists_kernel(int N, int J, int KL, int KS, const int *__restrict__ gi,
                                                        const int *__restrict__ gis, int *__restrict__ list, int *__restrict__ counts) {
    __shared__ unsigned small[RL_MAXN / 32], any[RL_MAXN / 32];
    __shared__ int scan[2][256];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int NW = (N + 31) >> 5;
    for (int i = tid; i < NW; i += 256) { small[i] = 0u; any[i] = 0u; }
    __syncthreads();
    const int *gl = gi + (size_t)b * J * KL;
    for (int i = tid; i < J * KL; i += 256) {
        const int p = gl[i];
        if (gis == nullptr && (i % KL) < KS && (unsigned)p < (unsigned)N) atomicOr(&small[p >> 5], 1u << (p & 31));
        if ((unsigned)p < (unsigned)N) atomicOr(&any[p >> 5], 1u << (p & 31));
    }
    if (gis != nullptr) {
        const int *gs = gis + (size_t)b * J * KS;
        for (int i = tid; i < J * KS; i += 256) {
            const int p = gs[i];
            if ((unsigned)p < (unsigned)N) {
                atomicOr(&small[p >> 5], 1u << (p & 31));
                atomicOr(&any[p >> 5], 1u << (p & 31));
            }
        }
    }
    __syncthreads();
    // thread t owns the words [t * WPT, (t + 1) * WPT): ascending points per thread, threads in order
    const int WPT = (NW + 255) >> 8;
    const int w0 = tid * WPT, w1 = w0 + WPT < NW ? w0 + WPT : NW;
    int cs = 0, co = 0;
    for (int i = w0; i < w1; ++i) {
        cs += __builtin_popcount(small[i]);
        co += __builtin_popcount(any[i] & ~small[i]);
    }
    int is = cs, io = co;  // inclusive scan
    for (int d = 1; d < 256; d <<= 1) {
        scan[0][tid] = is; scan[1][tid] = io;
        __syncthreads();
        if (tid >= d) { is += scan[0][tid - d]; io += scan[1][tid - d]; }
        __syncthreads();
    }
    scan[0][tid] = is; scan[1][tid] = io;
    __syncthreads();
    const int tot_s = scan[0][255], tot_o = scan[1][255];
    int *dst = list + (size_t)b * N;
    int ps = is - cs, po = tot_s + io - co;
    for (int i = w0; i < w1; ++i) {
        unsigned ms = small[i], mo = any[i] & ~small[i];
        while (ms) { const int k = __builtin_ctz(ms); ms &= ms - 1; dst[ps++] = 32 * i + k; }
        while (mo) { const int k = __builtin_ctz(mo); mo &= mo - 1; dst[po++] = 32 * i + k; }
    }
    if (tid == 0) { counts[2 * b] = tot_s; counts[2 * b + 1] = tot_s + tot_o; }
}

}  // namespace rchain
}  // namespace pn2

extern "C" int pn2x_row_lists(int b, int n, int j, int k_large, int k_small, const int *gi, const int *gi_small, int *list,
                              int *counts, void *stream) {
    using namespace pn2;
    if (b < 0 || n < 1 || j < 1 || k_large < 1 || k_small < 1 || k_small > k_large) return PN2_EINVAL;
    if (n > rchain::RL_MAXN || (long)j * k_large > (1L << 24)) return PN2_ERANGE;
    if (b == 0) return PN2_OK;
    if (!gi || !list || !counts) return PN2_ENULL;
    hipLaunchKernelGGL(rchain::row_lists_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, n, j, k_large, k_small, gi, gi_small,
                       list, counts);
    return check_launch();
}

extern "C" int pn2x_row_chain_supported(int c_in, int c_h, int c_conv, int c_q) {
    return (c_in == 128 && c_h == 128 && c_conv == 384 && c_q == 512) ? 1 : 0;
}

// the checks and the launch both entries share; h1in: the three-layer kernel (rows of CH floats, no wa / ba)
static int launch_chain(void (*kernel)(pn2::rchain::ChainArgs), pn2::PerDeviceOnce &raised, bool h1in, int b, int n, const float *x,
                        int ldx, const int *list, const int *counts, const float *wa, const float *ba, const float *wb,
                        const float *bb, const float *wc, const float *bc, const float *wq, float *out, int ldo, int grid,
                        void *stream) {
    using namespace pn2;
    using namespace pn2::rchain;
    if (b < 0 || n < 1 || ldx < (h1in ? CH : 132) || ldo < CQ || ldx % 4 || ldo % 4 || grid < 0) return PN2_EINVAL;
    if (b > MAXB || (long)b * n >= (1L << 31) / 2) return PN2_ERANGE;
    if (b == 0) return PN2_OK;
    if (!x || !list || !counts || (!h1in && (!wa || !ba)) || !wb || !bb || !wc || !bc || !wq || !out) return PN2_ENULL;
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)wa | (uintptr_t)ba | (uintptr_t)wb | (uintptr_t)bb | (uintptr_t)wc |
         (uintptr_t)bc | (uintptr_t)wq) % 16 != 0)
        return PN2_EINVAL;
    ChainArgs a;
    a.B = b; a.N = n; a.ldx = ldx; a.ldo = ldo; a.x = x; a.list = list; a.counts = counts;
    a.wa = wa; a.ba = ba; a.wb = wb; a.bb = bb; a.wc = wc; a.bc = bc; a.wq = wq; a.out = out;
    const size_t lds = lds_bytes(b);
    // the opt-in is made once per device, so it covers the largest batch the entry accepts, not the first call's
    static_assert(lds_bytes(MAXB) <= 160 * 1024, "row_chain's LDS at MAXB clouds exceeds a compute unit's 160 KB");
    if (raised.first_use())
        (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(MAXB));
    const int cus = num_compute_units();
    if (grid == 0 || grid > cus) grid = cus;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch();
}

extern "C" int pn2x_row_chain(int b, int n, const float *x, int ldx, const int *list, const int *counts, const float *wa,
                              const float *ba, const float *wb, const float *bb, const float *wc, const float *bc, const float *wq,
                              float *out, int ldo, int grid, void *stream) {
    static pn2::PerDeviceOnce raised;
    return launch_chain(pn2::rchain::row_chain_kernel, raised, false, b, n, x, ldx, list, counts, wa, ba, wb, bb, wc, bc, wq, out, ldo,
                        grid, stream);
}

extern "C" int pn2x_row_chain3_supported(int c_h, int c_conv, int c_q) {
    return (c_h == 128 && c_conv == 384 && c_q == 512) ? 1 : 0;
}

extern "C" int pn2x_row_chain3(int b, int n, const float *h1, int ldh, const int *list, const int *counts, const float *wb,
                               const float *bb, const float *wc, const float *bc, const float *wq, float *out, int ldo, int grid,
                               void *stream) {
    static pn2::PerDeviceOnce raised;
    return launch_chain(pn2::rchain::row_chain3_kernel, raised, true, b, n, h1, ldh, list, counts, nullptr, nullptr, wb, bb,
                        wc, bc, wq, out, ldo, grid, stream);
}
