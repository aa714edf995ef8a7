// sdf_mesh.hip -- SDF volume -> triangle mesh (include/pn2_sdf.h: pn2s_volume_mesh_count, pn2s_volume_mesh_emit): the way back
// from the volume the trackers look up to a surface.  Reference: gf_optimize_obj.sdf2mesh (optimization_obj.py:399-405), which
// samples its decoder on a grid and runs marching cubes (third_party/DeepSDF/mesh.py:76-140); here the volume the tracker used
// is extracted, by marching TETRAHEDRA, so that the output is fixed index for index.
//
// Algorithm.  Grid vertex v = (ix,iy,iz), linear (ix*res + iy)*res + iz, is INSIDE iff value(v) < level (fp32).  A cell's corner
// c + o is named by the bits of o: x = 1, y = 2, z = 4.  Every cell is split into six tetrahedra round its body diagonal (Kuhn):
// tetrahedron k belongs to the k-th permutation (a,b,c) of the axes in lexicographic order
//     k = 0 xyz, 1 xzy, 2 yxz, 3 yzx, 4 zxy, 5 zyx
// and has the vertices  t0 = c, t1 = c + e_a, t2 = c + e_a + e_b, t3 = c + e_x + e_y + e_z; det(t1-t0, t2-t0, t3-t0) is the
// permutation's sign, so k = 0, 3, 4 are positively oriented and k = 1, 2, 5 negatively.  Every edge of this grid runs from a
// vertex to that vertex plus an offset o != 0 and belongs to its lower endpoint with the class
//     0 +x (o = 1), 1 +y (2), 2 +z (4), 3 +xy (3), 4 +xz (5), 5 +yz (6), 6 +xyz (7).
// An edge whose endpoints differ in the inside flag carries one mesh vertex, key 7 * linear(lower) + class, at
//     p_a + t (p_b - p_a),  t = (level - s_a) / (s_b - s_a)   (a = the lower endpoint; fp32: a subtraction, a subtraction, a division)
// per axis  p = (i - res/2) * stride  where the offset has no bit, and  fma(t, stride, p)  where it has one.
// Triangles of a tetrahedron with inside set m (bit i: t_i inside), for a POSITIVELY oriented one -- a negatively oriented one
// swaps the last two corners of every triangle; edge (p,q) stands for the mesh vertex on t_p t_q:
//   one inside or one outside vertex i, the others j < k < l:  ((i,j), (i,k), (i,l)), last two swapped if that faces inwards;
//   two inside i < j, two outside k < l:  the quad (i,k) (i,l) (j,l) (j,k) split along (i,k)-(j,l) into
//     ((i,k), (i,l), (j,l)) and ((i,k), (j,l), (j,k)), both reversed as ((i,k), (j,l), (i,l)), ((i,k), (j,k), (j,l)) if they face inwards.
// "Faces inwards" is decided by vm_make_table() below at compile time, on the tetrahedron (0,0,0) (1,0,0) (1,1,0) (1,1,1) with
// the mesh vertices at the edges' midpoints: the normal must point from the inside vertices' centroid to the outside ones'.
// Output order: vertices by ascending key, triangles by ascending (cell linear index, k, triangle).
//
// Launches (no atomics, no workgroup waits for another; two runs are bitwise equal):
//   count   one lane per grid vertex, 256 consecutive vertices per workgroup: the 7-bit mask of owned crossing edges (one byte
//           per voxel), the cell's triangle count, and the workgroup's sums of both;
//   scan    ONE workgroup walks the workgroup sums in chunks of 1024 with a running carry: exclusive prefixes in place, totals
//           into the header;
//   apply   per voxel: the exclusive prefix of the vertex counts (workgroup prefix + scan inside the workgroup);
//   emit    vertices at prefix[v] + popcount(mask[v] & ((1 << class) - 1)); triangles at the workgroup's triangle prefix + a
//           scan of the cells' counts inside the workgroup, their corners looked up the same way.
// A lane reads the four rows (its own, +y, +x, +x+y) once each; the +z neighbours come from the next lane of the wave (the
// last lane of a wave reads them itself).
#include <cmath>

#include "pn2_common.h"
#include "sdf_device.h"
#include "../../include/pn2_sdf.h"

namespace pn2 {

constexpr int kVmThreads = 256;
constexpr int kVmScanThreads = 1024;
constexpr int kVmMaxRes = 512;     // 7 res^3 keys need 64 bits from res = 675; 12 res^3 triangles fit an int32 up to res = 563
constexpr long kVmHeader = 16;     // bytes: ints {vertices, triangles, 0, 0}

struct VmTable {
    unsigned tri[16];  // per inside set: six 3-bit edge ids, corners 0..2 of triangle 0 then of triangle 1
};

constexpr int vm_edge_id(int p, int q) {  // edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of a tetrahedron, p != q in any order
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    return lo == 0 ? hi - 1 : lo == 1 ? hi + 1 : 5;
}

// twice the midpoint of edge e of the model tetrahedron (0,0,0) (1,0,0) (1,1,0) (1,1,1), axis d
constexpr int vm_model_mid2(int e, int d) {
    const int P[6] = {0, 0, 0, 1, 1, 2}, Q[6] = {1, 2, 3, 2, 3, 3};
    return (P[e] > d ? 1 : 0) + (Q[e] > d ? 1 : 0);  // vertex i has coordinate d set iff i > d
}

constexpr VmTable vm_make_table() {
    VmTable t = {};
    for (int m = 1; m < 15; ++m) {
        int in[4] = {}, nin = 0, out[4] = {}, nout = 0;
        for (int i = 0; i < 4; ++i) {
            if ((m >> i) & 1) in[nin++] = i;
            else out[nout++] = i;
        }
        int e[6] = {};
        if (nin == 2) {
            e[0] = vm_edge_id(in[0], out[0]);
            e[1] = vm_edge_id(in[0], out[1]);
            e[2] = vm_edge_id(in[1], out[1]);
            e[3] = e[0];
            e[4] = e[2];
            e[5] = vm_edge_id(in[1], out[0]);
        } else {
            const int lone = nin == 1 ? in[0] : out[0];
            const int *rest = nin == 1 ? out : in;
            for (int j = 0; j < 3; ++j) e[j] = vm_edge_id(lone, rest[j]);
        }
        // normal of triangle 0 against (outside centroid - inside centroid), both scaled to integers
        int a[3] = {}, b[3] = {}, dir[3] = {};
        for (int d = 0; d < 3; ++d) {
            a[d] = vm_model_mid2(e[1], d) - vm_model_mid2(e[0], d);
            b[d] = vm_model_mid2(e[2], d) - vm_model_mid2(e[0], d);
            int so = 0, si = 0;
            for (int i = 0; i < nout; ++i) so += out[i] > d ? 1 : 0;
            for (int i = 0; i < nin; ++i) si += in[i] > d ? 1 : 0;
            dir[d] = nin * so - nout * si;
        }
        const int dot = (a[1] * b[2] - a[2] * b[1]) * dir[0] + (a[2] * b[0] - a[0] * b[2]) * dir[1] + (a[0] * b[1] - a[1] * b[0]) * dir[2];
        if (dot < 0) {
            int s = e[1]; e[1] = e[2]; e[2] = s;
            s = e[4]; e[4] = e[5]; e[5] = s;
        }
        for (int j = 0; j < 6; ++j) t.tri[m] |= (unsigned)e[j] << (3 * j);
    }
    return t;
}

__constant__ VmTable kVmTable = vm_make_table();

// tetrahedron k: the offset bits of t1 and t2 (t0 = 0, t3 = 7), 3 bits each, and the negatively oriented ones
constexpr unsigned kVmT1 = 1u | 1u << 3 | 2u << 6 | 2u << 9 | 4u << 12 | 4u << 15;
constexpr unsigned kVmT2 = 3u | 5u << 3 | 3u << 6 | 6u << 9 | 5u << 12 | 6u << 15;
constexpr unsigned kVmOdd = 0x26;  // k = 1, 2, 5
// offset bits -> edge class, 3 bits each (index 0 unused): 1 -> 0, 2 -> 1, 3 -> 3, 4 -> 2, 5 -> 4, 6 -> 5, 7 -> 6
constexpr unsigned kVmClassOfBits = 0u << 3 | 1u << 6 | 3u << 9 | 2u << 12 | 4u << 15 | 5u << 18 | 6u << 21;
constexpr unsigned kVmBitsOfClass = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;
constexpr unsigned kVmEdgeP = 0u | 0u << 2 | 0u << 4 | 1u << 6 | 1u << 8 | 2u << 10;
constexpr unsigned kVmEdgeQ = 1u | 2u << 2 | 3u << 4 | 2u << 6 | 3u << 8 | 3u << 10;

// What a lane knows of the cell whose lower corner is its grid vertex.
struct VmCell {
    float s[8];      // corner values by offset bits; a corner outside the grid reads as s[0]
    unsigned in;     // bit o: corner o is inside
    unsigned mask;   // bit c: the owned edge of class c carries a mesh vertex
    int ntri;        // triangles of the cell (0 where the vertex has no cell)
    int ix, iy, iz;
};

// Must be reached by every lane of the wave (the +z neighbours come from the next lane).  n = res^3; lin >= n: an idle lane.
template <bool F16>
__device__ __forceinline__ void vm_cell(const void *vol, int res, int n, int lin, float level, VmCell &c) {
    const bool live = lin < n;
    const int l = live ? lin : 0;
    c.ix = l / (res * res);
    c.iy = (l / res) % res;
    c.iz = l % res;
    const bool vx = live && c.ix < res - 1, vy = live && c.iy < res - 1, vz = live && c.iz < res - 1;
    float r[4];  // the rows: this vertex, +x, +y, +x+y
    r[0] = live ? ld_vol<F16>(vol, l) : 0.f;
    r[1] = vx ? ld_vol<F16>(vol, l + res * res) : 0.f;
    r[2] = vy ? ld_vol<F16>(vol, l + res) : 0.f;
    r[3] = vx && vy ? ld_vol<F16>(vol, l + res * res + res) : 0.f;
    const bool own = (threadIdx.x & (kWave - 1)) == kWave - 1;  // no next lane
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const bool have = (!(o & 1) || vx) && (!(o & 2) || vy);
        float z = __shfl_down(r[o], 1);  // lane + 1 holds vertex lin + 1 = this vertex + e_z where vz
        if (own) z = have && vz ? ld_vol<F16>(vol, l + (o & 1) * res * res + (o >> 1) * res + 1) : 0.f;
        c.s[o] = have ? r[o] : r[0];
        c.s[o | 4] = have && vz ? z : r[0];
    }
    c.in = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) c.in |= (c.s[o] < level ? 1u : 0u) << o;
    c.mask = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const unsigned o = (kVmBitsOfClass >> (3 * k)) & 7;
        c.mask |= (((c.in >> o) ^ c.in) & 1u) << k;
    }
    c.ntri = 0;
    if (vx && vy && vz) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const unsigned t1 = (kVmT1 >> (3 * k)) & 7, t2 = (kVmT2 >> (3 * k)) & 7;
            const int cnt = (c.in & 1) + ((c.in >> t1) & 1) + ((c.in >> t2) & 1) + ((c.in >> 7) & 1);
            c.ntri += cnt == 2 ? 2 : (cnt & 1);
        }
    }
}

// Exclusive scan of x over the workgroup (WAVES waves), in thread order; total = the sum.  lds: WAVES ints.
template <int WAVES>
__device__ __forceinline__ int vm_block_scan(int x, int *lds, int &total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int inc = x;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    __syncthreads();  // (lds may still be read from the previous scan)
    if (lane == kWave - 1) lds[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int s = lds[w];
        before += w < wave ? s : 0;
        total += s;
    }
    return before + inc - x;
}

// work: header | prefix int32[n] | sums int32[2 nb] (vertices, triangles per workgroup) | mask byte[n]
struct VmWork {
    int *header, *prefix, *sums;
    unsigned char *mask;
};

__host__ __device__ inline long vm_round16(long x) { return (x + 15) & ~15L; }
static inline long vm_blocks(long n) { return (n + kVmThreads - 1) / kVmThreads; }
static inline long vm_work_bytes(long n) { return kVmHeader + vm_round16(4 * n) + vm_round16(8 * vm_blocks(n)) + vm_round16(n); }
static inline VmWork vm_work(void *work, long n) {
    char *p = reinterpret_cast<char *>(work);
    VmWork w;
    w.header = reinterpret_cast<int *>(p);
    w.prefix = reinterpret_cast<int *>(p + kVmHeader);
    w.sums = reinterpret_cast<int *>(p + kVmHeader + vm_round16(4 * n));
    w.mask = reinterpret_cast<unsigned char *>(p + kVmHeader + vm_round16(4 * n) + vm_round16(8 * vm_blocks(n)));
    return w;
}

template <bool F16>
__global__ void __launch_bounds__(kVmThreads)
volume_mesh_count_kernel(const void *__restrict__ vol, int res, int n, float level, unsigned char *__restrict__ mask, int *__restrict__ sums) {
    __shared__ int lds[kVmThreads / kWave];
    const int lin = blockIdx.x * kVmThreads + threadIdx.x;
    VmCell c;
    vm_cell<F16>(vol, res, n, lin, level, c);
    if (lin < n) mask[lin] = (unsigned char)c.mask;
    int nv, nt;
    vm_block_scan<kVmThreads / kWave>(lin < n ? __popc(c.mask) : 0, lds, nv);
    vm_block_scan<kVmThreads / kWave>(lin < n ? c.ntri : 0, lds, nt);
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = nv;
        sums[2 * blockIdx.x + 1] = nt;
    }
}

__global__ void __launch_bounds__(kVmScanThreads)
volume_mesh_scan_kernel(int nb, int *__restrict__ sums, int *__restrict__ header) {
    __shared__ int lds[kVmScanThreads / kWave];
    int carry_v = 0, carry_t = 0;
    for (int base = 0; base < nb; base += kVmScanThreads) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? sums[2 * i] : 0, t = i < nb ? sums[2 * i + 1] : 0;
        int tot_v, tot_t;
        const int ev = vm_block_scan<kVmScanThreads / kWave>(v, lds, tot_v);
        const int et = vm_block_scan<kVmScanThreads / kWave>(t, lds, tot_t);
        if (i < nb) {
            sums[2 * i] = carry_v + ev;
            sums[2 * i + 1] = carry_t + et;
        }
        carry_v += tot_v;
        carry_t += tot_t;
    }
    if (threadIdx.x == 0) {
        header[0] = carry_v;
        header[1] = carry_t;
        header[2] = header[3] = 0;
    }
}

__global__ void __launch_bounds__(kVmThreads)
volume_mesh_apply_kernel(int n, const unsigned char *__restrict__ mask, const int *__restrict__ sums, int *__restrict__ prefix) {
    __shared__ int lds[kVmThreads / kWave];
    const int lin = blockIdx.x * kVmThreads + threadIdx.x;
    int total;
    const int ex = vm_block_scan<kVmThreads / kWave>(lin < n ? __popc((unsigned)mask[lin]) : 0, lds, total);
    if (lin < n) prefix[lin] = sums[2 * blockIdx.x] + ex;
}

template <bool F16>
__global__ void __launch_bounds__(kVmThreads)
volume_mesh_emit_kernel(const void *__restrict__ vol, int res, int n, float stride, float level, const unsigned char *__restrict__ mask,
                        const int *__restrict__ sums, const int *__restrict__ prefix, int nv, int nf, float *__restrict__ verts,
                        int *__restrict__ faces) {
    __shared__ int lds[kVmThreads / kWave];
    const int lin = blockIdx.x * kVmThreads + threadIdx.x;
    VmCell c;
    vm_cell<F16>(vol, res, n, lin, level, c);
    int total;
    int tri = sums[2 * blockIdx.x + 1] + vm_block_scan<kVmThreads / kWave>(lin < n ? c.ntri : 0, lds, total);
    if (lin >= n) return;
    if (c.mask) {
        const int h = res / 2;
        const float pa[3] = {(float)(c.ix - h) * stride, (float)(c.iy - h) * stride, (float)(c.iz - h) * stride};
        int at = prefix[lin];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            if (!((c.mask >> k) & 1)) continue;
            const unsigned o = (kVmBitsOfClass >> (3 * k)) & 7;
            const float t = (level - c.s[0]) / (c.s[o] - c.s[0]);
            if (at < nv) {
#pragma unroll
                for (int d = 0; d < 3; ++d) verts[3 * (size_t)at + d] = (o >> d) & 1 ? __builtin_fmaf(t, stride, pa[d]) : pa[d];
            }
            ++at;
        }
    }
    if (c.ntri == 0) return;
    const unsigned in = c.in;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const unsigned bits = 0u | ((kVmT1 >> (3 * k)) & 7) << 3 | ((kVmT2 >> (3 * k)) & 7) << 6 | 7u << 9;  // t0..t3, 3 bits each
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m |= ((in >> ((bits >> (3 * i)) & 7)) & 1u) << i;
        const int cnt = __popc(m);
        const int ntri = cnt == 2 ? 2 : (cnt & 1);
        const unsigned row = kVmTable.tri[m];
        const bool odd = (kVmOdd >> k) & 1;
        for (int j = 0; j < ntri; ++j, ++tri) {
            int idx[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned e = (row >> (9 * j + 3 * q)) & 7;
                const unsigned lo = (bits >> (3 * ((kVmEdgeP >> (2 * e)) & 3))) & 7, hi = (bits >> (3 * ((kVmEdgeQ >> (2 * e)) & 3))) & 7;
                const unsigned cls = (kVmClassOfBits >> (3 * (hi ^ lo))) & 7;
                const int at = lin + (int)(lo & 1) * res * res + (int)((lo >> 1) & 1) * res + (int)(lo >> 2);  // inside the cell: < n
                idx[q] = prefix[at] + __popc((unsigned)mask[at] & ((1u << cls) - 1u));
            }
            if (tri < nf) {
                faces[3 * (size_t)tri] = idx[0];
                faces[3 * (size_t)tri + 1] = odd ? idx[2] : idx[1];
                faces[3 * (size_t)tri + 2] = odd ? idx[1] : idx[2];
            }
        }
    }
}

static int vm_check(const void *vol, int vol_f16, int res, float stride, float level, const void *work, long work_bytes) {
    if (res < 2 || (vol_f16 != 0 && vol_f16 != 1) || !(stride > 0.f) || !std::isfinite(stride) || !std::isfinite(level)) return PN2_EINVAL;
    if (!vol || !work) return PN2_ENULL;
    if (res > kVmMaxRes) return PN2_ERANGE;
    if (work_bytes < vm_work_bytes((long)res * res * res)) return PN2_ESCRATCH;
    if (((uintptr_t)work & 15) != 0) return PN2_EINVAL;
    return PN2_OK;
}

}  // namespace pn2

extern "C" long pn2s_volume_mesh_work_bytes(int res) {
    if (res < 2) return (long)PN2_EINVAL;
    if (res > pn2::kVmMaxRes) return (long)PN2_ERANGE;
    return pn2::vm_work_bytes((long)res * res * res);
}

extern "C" int pn2s_volume_mesh_count(const void *vol, int vol_f16, int res, float stride, float level, void *work, long work_bytes,
                                       void *stream) {
    using namespace pn2;
    const int rc = vm_check(vol, vol_f16, res, stride, level, work, work_bytes);
    if (rc != PN2_OK) return rc;
    const int n = res * res * res, nb = (int)vm_blocks(n);
    const VmWork w = vm_work(work, n);
    hipStream_t st = (hipStream_t)stream;
    if (vol_f16) hipLaunchKernelGGL(volume_mesh_count_kernel<true>, dim3(nb), dim3(kVmThreads), 0, st, vol, res, n, level, w.mask, w.sums);
    else hipLaunchKernelGGL(volume_mesh_count_kernel<false>, dim3(nb), dim3(kVmThreads), 0, st, vol, res, n, level, w.mask, w.sums);
    hipLaunchKernelGGL(volume_mesh_scan_kernel, dim3(1), dim3(kVmScanThreads), 0, st, nb, w.sums, w.header);
    hipLaunchKernelGGL(volume_mesh_apply_kernel, dim3(nb), dim3(kVmThreads), 0, st, n, (const unsigned char *)w.mask, (const int *)w.sums,
                       w.prefix);
    return check_launch();
}

extern "C" int pn2s_volume_mesh_emit(const void *vol, int vol_f16, int res, float stride, float level, const void *work,
                                      long work_bytes, int nv, int nf, float *verts, int *faces, void *stream) {
    using namespace pn2;
    const int rc = vm_check(vol, vol_f16, res, stride, level, work, work_bytes);
    if (rc != PN2_OK) return rc;
    if (nv < 0 || nf < 0) return PN2_EINVAL;
    if (nv == 0 && nf == 0) return PN2_OK;
    if ((nv > 0 && !verts) || (nf > 0 && !faces)) return PN2_ENULL;
    const int n = res * res * res, nb = (int)vm_blocks(n);
    const VmWork w = vm_work(const_cast<void *>(work), n);
    hipStream_t st = (hipStream_t)stream;
    if (vol_f16)
        hipLaunchKernelGGL(volume_mesh_emit_kernel<true>, dim3(nb), dim3(kVmThreads), 0, st, vol, res, n, stride, level,
                           (const unsigned char *)w.mask, (const int *)w.sums, (const int *)w.prefix, nv, nf, verts, faces);
    else
        hipLaunchKernelGGL(volume_mesh_emit_kernel<false>, dim3(nb), dim3(kVmThreads), 0, st, vol, res, n, stride, level,
                           (const unsigned char *)w.mask, (const int *)w.sums, (const int *)w.prefix, nv, nf, verts, faces);
    return check_launch();
}
