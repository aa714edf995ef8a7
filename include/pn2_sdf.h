/*
 * pn2_sdf.h -- C ABI of the particle optimisers' signed-distance-volume lookups.
 *
 * The reference evaluates thousands of candidate poses ("particles") per tracking step by transforming the
 * observed cloud into each candidate's object frame and looking every point up in a voxelised SDF:
 *   - gf_optimize_obj.Distance / evaluate / optimize   network/models/optimization_obj.py:184-237, :244-301
 *     (2048 particles x N points, trilinear interpolation in a 201^3 fp16 volume, 10 iterations per frame)
 *   - gf_optimize_hand_pose.query_sdf / get_penetration_loss   network/models/optimization_hand.py:252-268
 *     (5120 particles x 778 MANO vertices, nearest-voxel read from a 151^3 fp16 volume)
 * as ~60 elementwise torch kernels over (P*N)-element temporaries per evaluation.  Each entry below is one
 * launch with no temporaries: transform, address arithmetic, gathers, interpolation and the per-particle
 * reduction are fused; the volume (16 MB at 201^3 fp16) stays resident in L2 / Infinity Cache.
 *
 * Conventions as pn2_hip.h: raw device pointers, contiguous row-major arrays, caller allocates everything,
 * asynchronous on `stream` (hipStream_t as void*, NULL = default stream), returns PN2_OK or a negative PN2_E*
 * code (pn2_strerror), nothing is retained after return.  Volumes: res^3 elements, element (ix,iy,iz) at
 * (ix*res + iy)*res + iz, IEEE binary16 (`vol_f16` = 1, the reference's storage type) or fp32 (`vol_f16` = 0, the
 * type the reference's volume has after `update_shape`, optimization_obj.py:400).  The trilinear entries take a
 * `vol_fmt` instead: 0 / 1 = that linear layout in fp32 / fp16, 2 / 3 = the CORNER layout built from it by
 * pn2s_build_corner_volume (fp32 / fp16), which they read ~3x faster.  Arithmetic is fp32 and follows
 * the reference's torch expressions operation for operation (true division, same association); the 3x3
 * transforms use the fixed chain  o_j = fma(q2, R2j, fma(q1, R1j, q0*R0j)).
 */
#ifndef PN2_SDF_H
#define PN2_SDF_H

#include "pn2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Corner layout for the trilinear entries ("memory laid out for the lookup"): cell i (16 bytes in fp16, 32 in fp32)
 * holds the eight corner values d000..d111 that Distance() fetches when its base index i000 == i, gathered with the
 * reference's own index arithmetic and clamps (optimization_obj.py:206-222).  A lookup becomes ONE aligned 16-byte
 * load per point instead of eight scattered 2-byte reads in four cache lines, and is bit-identical to a lookup in
 * the linear volume for every input.  8x the memory (201^3 fp16: 130 MB of 288 GB), built once per object.
 *   out: pn2s_corner_volume_elems(res) elements of the volume's type (= 8 * res^3), 16-byte aligned.
 */
long pn2s_corner_volume_elems(int res);
int pn2s_build_corner_volume(const void *vol, int vol_f16, int res, void *out, void *stream);

/*
 * Distance(V)  (optimization_obj.py:184-228): trilinear SDF at m points.
 *   V (m,3) object-frame coordinates; out (m).  x = clamp((v - bbox_min)/stride, 0, res-1) per axis, the eight
 *   corner indices clamped to [0, res^3-1] exactly as the reference does, result clamped to [clamp_lo, clamp_hi]
 *   (reference constants: bbox_min -0.2, clamps -0.05 / 0.05).  res in [2, 1024]; stride finite and > 0 (PN2_EINVAL otherwise).
 */
int pn2s_trilinear(int m, const float *V, const void *vol, int vol_fmt, int res, float bbox_min, float stride,
                   float clamp_lo, float clamp_hi, float *out, void *stream);

/*
 * evaluate(pcld, r, t)  (optimization_obj.py:230-237), fused: for each of p particles
 *   sdf_energy[i] = mean_j | Distance((pcld[j] - trans[i]) @ rot[i]) |
 * pcld (n,3) is shared by all particles; rot (p,3,3) row-major; trans (p,3).  The reference's `energy` is
 * 500 * sdf_energy (left to the caller).
 */
int pn2s_particle_energy(int p, int n, const float *pcld, const float *rot, const float *trans, const void *vol,
                         int vol_fmt, int res, float bbox_min, float stride, float clamp_lo, float clamp_hi,
                         float *sdf_energy, void *stream);

/*
 * The particle loop of gf_optimize_obj.optimize (optimization_obj.py:253-301, update_shape_flag False), entirely
 * on the device: `iterations` launches, each evaluating p candidate poses
 *   sample_i = [sqrt(1-|v|^2), v = pre_sampled[i,0:3]*search[0:3], pre_sampled[i,3:6]*search[3:6]]
 *   R_i = R @ quat2mat(sample_i[0:4]),  t_i = t + sample_i[4:7]
 * and then (last workgroup to finish) the weighted-mean pose update, SO(3) re-projection and search-size update,
 * with no host synchronisation (the reference syncs on `torch.any` every iteration).
 * pn2s_obj_opt is HOST memory, read during the call; its pointers are DEVICE memory:
 *   pcld        (n,3) camera-frame points; the batch entry: the packed clouds (sum_k n_k, 3);
 *   pre_sampled (p,6) with row 0 == 0 (particle 0 is the current pose), shared by all problems;
 *   volume      of layout `vol_fmt`, with res, bbox_min, stride, clamp_lo and clamp_hi as pn2s_trilinear;
 *   poses       in/out (problems,12): rotation (3,3) row-major, then translation (3), per problem;
 *   work        scratch of work_floats floats: at least pn2s_obj_optimize_work_floats(p) (16 header floats and p energies) for the
 *               single entry, pn2s_obj_optimize_batch_work_floats(problems, p) for the batch = `problems` such records, each padded
 *               to a multiple of 16 floats.  Contents undefined on return except a record's [0..5] = final search size and its
 *               ticket, which is zero again;
 *   c1, c2, beta: scaling_coefficient1 (0.02), scaling_coefficient2 (2), beta (0.9).
 * pn2s_obj_optimize: problems == 1, n >= 1 points, `volume`; a grid of p workgroups.  cloud_off and vols are not read.
 * pn2s_obj_optimize_batch: `problems` independent problems at once (one frame step of that many object sequences tracked in
 *   lockstep): one init launch and `iterations` launches of a (p, problems) grid for all of them together, capturable in a HIP graph.
 *   Workgroup (i, k) evaluates particle i of problem k; the last workgroup of problem k to finish -- by problem k's own ticket --
 *   does problem k's update.  No workgroup waits for another, and no problem reads what another writes.  Every problem's result
 *   is bit-for-bit what pn2s_obj_optimize returns for it alone (one kernel, the same accumulation order).
 *   cloud_off   DEVICE array of problems + 1 ints, in points: problem k owns rows [cloud_off[k], cloud_off[k+1]).  The offsets must
 *               lie inside pcld (the caller's duty: they are read on the device only).  A problem with an empty slice
 *               (cloud_off[k+1] <= cloud_off[k]) is INACTIVE: its pose is left untouched; the entry vols[k] is loaded but
 *               the volume is never read, so the entry may be NULL -- how a sequence that has ended sits out the remaining
 *               frames of its group;
 *   vols        DEVICE array of `problems` volume pointers, all of one vol_fmt, res, bbox_min and stride.
 *   n and volume are not read; problems == 0 is a no-op that reads nothing.
 * Refused with nothing launched, checked in this order: a NULL record (PN2_ENULL);  a record pointer no process can own -- below
 *   64 KiB or in the upper half of the address space, which is what a caller built against the positional entries passes, its
 *   count -- is PN2_EINVAL and is not read;  PN2_EINVAL for problems < 0 (the single entry: != 1, or n < 1), p < 1, iterations < 0, res outside [2, 1024], vol_fmt outside 0..3, a stride that is not finite and > 0 (an
 *   infinite stride, which puts every point in cell 0, is refused like a NaN);  PN2_ERANGE for problems > PN2S_OPT_BATCH_MAX (the
 *   grid's second dimension), p > 2^20, problems * p > 2^22 (workgroups per launch);  PN2_ENULL for a NULL pointer the entry reads;
 *   PN2_ESCRATCH when work_floats is too small.
 */
#define PN2S_OPT_BATCH_MAX 65535
struct pn2s_obj_opt {
    const float *pcld;
    const int *cloud_off;     /* batch entry only */
    const float *pre_sampled;
    const void *volume;       /* single entry only */
    const void *const *vols;  /* batch entry only */
    float *poses;
    float *work;
    long work_floats;
    float bbox_min, stride, clamp_lo, clamp_hi;
    float c1, c2, beta;
    int problems, p, n, iterations, res, vol_fmt;
    int pad_; /* to 120 bytes; not read */
}; /* 120 bytes */
typedef struct pn2s_obj_opt pn2s_obj_opt;
int pn2s_obj_optimize(const pn2s_obj_opt *opt, void *stream);
int pn2s_obj_optimize_batch(const pn2s_obj_opt *opt, void *stream);
int pn2s_obj_optimize_work_floats(int p);
long pn2s_obj_optimize_batch_work_floats(int s, int p);

/*
 * query_sdf(hand) (+ get_penetration_loss)  (optimization_hand.py:252-268): nearest-voxel read.
 *   hand (b,n,3); obj_r (3,3); obj_t (3):  q = (hand - obj_t) @ obj_r;
 *   index per axis = clamp(q // voxel_scale, -(res/2), res/2) + res/2   (`//` = torch's floor division);
 *   res must be odd (the reference asserts the index range; its volumes are 151^3 / 201^3).
 *   out_idx (b,n) int32 flat voxel index, or NULL;
 *   out_sdf (b,n) in the volume's element type (bit copy), or NULL;
 *   out_pen (b)   max_n |sdf| * (sdf < 0) in the volume's element type, or NULL.
 */
int pn2s_nearest(int b, int n, const float *hand, const float *obj_r, const float *obj_t, const void *vol,
                 int vol_f16, int res, float voxel_scale, int *out_idx, void *out_sdf, void *out_pen, void *stream);

/*
 * Signed distance to a triangle mesh -- the producer of the volumes above (optimization_obj.py:163-182, load_obj_oracle: "directly
 * compute the SDF volume from a mesh if we assume the mesh is known"; the reference leaves it commented out because it needs
 * kaolin).  verts (nv,3) fp32; faces (nf,3) int32 vertex indices, closed and outward oriented.
 *   magnitude: the exact minimum over ALL triangles of the distance to the triangle's closest point (face, edge or vertex);
 *              no triangle is culled.  The face counts where the query's projection lies inside all three edges' lines,
 *              n . ((end - start) x (p - start)) >= 2^-20 |end - start| |p - start| with n the unit normal (built in fp64):
 *              well conditioned for slivers down to the degeneracy threshold below; within the margin the nearest edge stands
 *              in for the face, at most 2^-20 |p - start| farther;
 *   sign:     generalised winding number w = (1/4pi) sum_f Omega_f, Omega_f = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| +
 *              (b.c)|a| + (c.a)|b|), a, b, c = v - p (Van Oosterom-Strackee); negative (inside) iff w > 0.5.  Every query sums its
 *              angles in face order: no atomics, two runs are bitwise equal;
 *   degenerate triangles (a repeated vertex, three collinear vertices: |n|^2 <= 1e-12 |b-a|^2 |c-a|^2) contribute the distance
 *              to their segment or point and exactly zero solid angle; no input produces a NaN.
 * work: scratch of at least pn2s_mesh_sdf_work_floats(nf) floats, 16-byte aligned (the per-triangle records, built by a
 *   prepare launch).  On return -- in stream order -- the int at work[0] is 1 if a face index lies outside [0, nv) and 0
 *   otherwise.  Such a face is replaced by vertex 0, so nothing is read out of bounds, and the outputs must not be used: the caller
 *   reads that one word back.  A volume is built once per object and outside any captured graph, so the one read-back costs
 *   nothing that matters; a caller inside a capture leaves the word on the device.
 * Limits: nv, nf <= 2^24, res <= 1023 (PN2_ERANGE beyond); PN2_ESCRATCH when work_floats is too small.
 *
 * pn2s_mesh_sdf_points: pts (m,3) -> out_sdf (m) signed and unclamped; out_wn (m) the winding numbers, or NULL.  m == 0 is a
 *   no-op that reads nothing.
 * pn2s_mesh_sdf_volume: res^3 voxels, element (ix,iy,iz) at (ix*res + iy)*res + iz with centre ((ix,iy,iz) - res/2) * stride
 *   (fp32 product; res odd -- the grid pn2s_nearest indexes), the value clamped to [-clamp, clamp] (the reference: 0.1) and
 *   rounded once to the output type (out_f16 = 1: IEEE binary16, 0: fp32).  Before clamping and rounding, the value is
 *   bit-for-bit what pn2s_mesh_sdf_points returns at that centre.
 */
long pn2s_mesh_sdf_work_floats(int nf);
int pn2s_mesh_sdf_points(int m, const float *pts, int nv, const float *verts, int nf, const int *faces, float *out_sdf,
                         float *out_wn, float *work, long work_floats, void *stream);
int pn2s_mesh_sdf_volume(int nv, const float *verts, int nf, const int *faces, int res, float stride, float clamp, void *out,
                         int out_f16, float *work, long work_floats, void *stream);

/*
 * SDF volume -> triangle mesh -- the way back from the volumes above to a surface (the reference: gf_optimize_obj.sdf2mesh,
 * optimization_obj.py:399-405, marching cubes over its decoder; here marching tetrahedra over the volume itself, so that the
 * output is fixed index for index; hotrack_amd/csrc/sdf_mesh.hip states the algorithm).
 *   Grid vertex (ix,iy,iz) is inside iff its value < level (fp32; binary16 converts exactly).  Every cell is split into six
 *   tetrahedra round its body diagonal; an edge of that grid whose endpoints differ in the inside flag carries one mesh vertex,
 *   shared by every tetrahedron round it, at  p_a + t (p_b - p_a),  t = (level - s_a) / (s_b - s_a)  with a the lower endpoint and
 *   p = ((ix,iy,iz) - res/2) * stride, the grid of pn2s_mesh_sdf_volume.  Triangles face outwards (towards increasing value).
 *   Vertices come in ascending key 7 * linear(lower endpoint) + edge class, triangles in ascending (cell, tetrahedron, triangle):
 *   nothing depends on launch order, and two runs are bitwise equal.  A value exactly at `level` puts coincident vertices on
 *   the grid vertex and gives zero-area triangles; the mesh stays closed wherever the surface does not leave the volume.
 * Two calls, because the caller allocates the outputs:
 *   pn2s_volume_mesh_count  three launches (count, scan of the workgroup sums by ONE workgroup, apply); on return -- in stream
 *                           order -- the ints at work[0] and work[1] are the numbers of vertices and of triangles.  The caller
 *                           reads those two words back (its one synchronisation) and allocates verts (nv,3) and faces (nf,3);
 *   pn2s_volume_mesh_emit   one launch, with the SAME vol, vol_f16, res, level and the work buffer as pn2s_volume_mesh_count
 *                           left it.  Nothing is written past nv vertices or nf triangles whatever the buffer holds.
 *                           nv == nf == 0 is a no-op.
 * work: at least pn2s_volume_mesh_work_bytes(res) bytes, 16-byte aligned: an int32 prefix and a mask byte per voxel and two
 *   ints per 256 voxels (201^3: 40.7 MB).
 * Refused with nothing launched: res < 2, stride not finite or <= 0, level not finite, vol_f16 not 0 / 1 (PN2_EINVAL);
 *   res > 512 (PN2_ERANGE: beyond it 12 res^3 triangle slots leave an int32; keys 7 res^3 are never formed on the device);
 *   work_bytes too small (PN2_ESCRATCH).
 */
long pn2s_volume_mesh_work_bytes(int res);
int pn2s_volume_mesh_count(const void *vol, int vol_f16, int res, float stride, float level, void *work, long work_bytes,
                           void *stream);
int pn2s_volume_mesh_emit(const void *vol, int vol_f16, int res, float stride, float level, const void *work, long work_bytes,
                          int nv, int nf, float *verts, int *faces, void *stream);

/*
 * Tracked depth frames fused into an SDF volume (hotrack_amd/csrc/tsdf_fuse.hip): the weighted running average of
 * truncated signed distances per voxel (KinectFusion's update) -- the online shape update of a volume that was built from a mesh or
 * handed over.  ONE launch integrates `frames` >= 1 frames, in order, into one volume in place; one lane per voxel walks the frames
 * with V and W in fp32 registers.  pn2s_tsdf_frames is HOST memory, read during the call; its pointers are DEVICE memory:
 *   volume (res^3) fp32 or, with vol_f16 = 1, binary16, element (ix,iy,iz) at (ix*res + iy)*res + iz, voxel centre
 *          p = ((ix,iy,iz) - res/2) * voxel_scale (the grid of pn2s_mesh_sdf_volume);  weight (res^3) fp32;  both in/out;
 *   depth (frames,h,w) fp32 metres, or with depth_u16 = 1 uint16 counts, D = (float)((double)raw * depth_scale);
 *   seg (frames,hs,ws,c) bytes, c 1 or 3, h = f hs and w = f ws with one integer f >= 1: pixel (v,u) reads seg[v / f, u / f]
 *          (as pn2x_depth_frame_clouds); the pixel is the object's iff its byte `channel` equals `value`;
 *   intrinsics (frames,4) fx, fy, cx, cy;  rotation (frames,3,3) row-major and translation (frames,3): the tracked pose, the
 *          object-frame cloud being (pcld - t) @ R, so that a voxel centre p is seen at q = R p + t.
 * Per voxel and frame, fp32 (the exact expressions, with their fmaf, are at the head of tsdf_fuse.hip): q = R p + t; flip_yz = 1
 * negates q_y and q_z (the front end negated them on the way in); skip unless q_z > 1e-6; u = rint(q_x / q_z fx + cx),
 * v = rint(q_y / q_z fy + cy), skip outside the image; D = depth[v,u], skip unless finite and > 0; d = D - q_z;
 *   object pixel:  skip if d < -trunc, else s = min(d, trunc), g = 1;
 *   other pixel:   free space only: d > trunc gives s = trunc, g = carve_weight, else skip;  g == 0 skips;
 *   V = (V W + s g) / (W + g),  W = min(W + g, max_weight).
 * A voxel no frame updated is not written (its bytes stay).  No atomics, two runs are bitwise equal; an fp32 volume after one
 * launch of F frames has the bits of F launches of one frame; an fp16 volume is rounded once, at the end of the launch.
 * No host sync or allocation (capturable).
 * Refused with nothing launched: PN2_EINVAL for res < 2, frames < 1, a size < 1, h / hs and w / ws not one integer factor, c not 1
 *   or 3, channel outside [0, c) or value outside [0, 255], vol_f16 / depth_u16 / flip_yz not 0 / 1, voxel_scale, trunc or
 *   max_weight not finite and > 0, carve_weight not finite or < 0, depth_u16 = 1 with a depth_scale that is not finite and > 0;
 *   PN2_ERANGE for res > 512, h w >= 2^29 or frames > 65535;  PN2_ENULL for a NULL record or pointer (checked in this order).
 */
struct pn2s_tsdf_frames {
    void *volume;
    float *weight;
    const void *depth;
    const unsigned char *seg;
    const float *intrinsics;
    const float *rotation;
    const float *translation;
    double depth_scale;
    float voxel_scale, trunc, carve_weight, max_weight;
    int res, vol_f16, frames, h, w, hs, ws, c, depth_u16, flip_yz, channel, value;
}; /* 128 bytes */
typedef struct pn2s_tsdf_frames pn2s_tsdf_frames;
int pn2s_tsdf_integrate(const pn2s_tsdf_frames *frames, void *stream);

/*
 * pn2s_tsdf_integrate for the `sequences` volumes of a group tracked in lockstep, in ONE launch.  Sequence k
 * integrates the frames [frame_off[k], frame_off[k+1]) of the group's packed frame arrays, in order, into volumes[k] / weights[k];
 * afterwards both have, bit for bit, what pn2s_tsdf_integrate gives for that volume and those frames alone (one __device__
 * function holds the rule for both entries; no workgroup reads what another writes).  pn2s_tsdf_group is HOST memory:
 *   volumes, weights  DEVICE arrays of `sequences` pointers to res^3 volumes (all of one res, vol_f16 and voxel_scale) and fp32 weights;
 *   frame_off         DEVICE array of sequences + 1 ints, in frames.  Every slice is clamped to [0, frames] on the device, so a
 *                     wrong table never indexes outside the packed arrays.  A sequence with an empty slice
 *                     (frame_off[k+1] <= frame_off[k] after clamping) is INACTIVE: its workgroups leave before its table entries,
 *                     which may be NULL, or any volume are read, and its volume and weights keep every byte -- how a
 *                     sequence that has ended, or has nothing pending, sits a flush out;
 *   depth (frames,h,w), seg (frames,hs,ws,c), intrinsics (frames,4), rotation (frames,3,3), translation (frames,3): the packed
 *                     frames of all sequences, `frames` the group's total; everything else as in pn2s_tsdf_frames, shared.
 * The three device tables cannot be checked here: that an active sequence's entries point to res^3 elements each, and that no two
 * active sequences share a volume or weights (two workgroups would then write one voxel), is the caller's duty -- the Python
 * binding (hotrack_amd.sdf.tsdf_integrate_batch) is the checked boundary.
 * Grid (z tiles x y blocks, res, sequences): the voxel and the sequence come from block and thread indices; the third grid
 * dimension gives the limit sequences <= PN2S_TSDF_BATCH_MAX.  sequences == 0 or frames == 0 is a no-op that reads and launches
 * nothing (with every slice empty and frames > 0 the launch's workgroups all leave at once).
 * Refused with nothing launched, checked in this order: a NULL record (PN2_ENULL); sequences < 0, frames < 0 and every
 *   PN2_EINVAL of pn2s_tsdf_integrate; PN2_ERANGE for res > 512, h w >= 2^29, frames > 65535 or sequences > PN2S_TSDF_BATCH_MAX;
 *   PN2_ENULL for a NULL table or frame array when there is something to integrate.
 */
#define PN2S_TSDF_BATCH_MAX 65535
struct pn2s_tsdf_group {
    void *const *volumes;
    float *const *weights;
    const int *frame_off;
    const void *depth;
    const unsigned char *seg;
    const float *intrinsics;
    const float *rotation;
    const float *translation;
    double depth_scale;
    float voxel_scale, trunc, carve_weight, max_weight;
    int res, vol_f16, sequences, frames, h, w, hs, ws, c, depth_u16, flip_yz, channel, value;
    int pad_; /* to 144 bytes; not read */
}; /* 144 bytes */
typedef struct pn2s_tsdf_group pn2s_tsdf_group;
int pn2s_tsdf_integrate_batch(const pn2s_tsdf_group *group, void *stream);

/*
 * An SDF volume rendered to depth and normal maps at tracked poses (hotrack_amd/csrc/sdf_raycast.hip): the raycast, the
 * image the model predicts.  The geometry is the inverse of pn2s_tsdf_integrate's, so a raycast of a volume at a pose lands on the
 * pixels pn2s_tsdf_integrate writes that pose's voxels from.  ONE launch renders `frames` >= 1 frames of one volume, one lane per
 * pixel, a wave per 8 x 8 tile.  pn2s_raycast is HOST memory, read during the call; its pointers are DEVICE memory:
 *   volume (res^3) fp32 or, with vol_f16 = 1, binary16, the linear layout (ix*res + iy)*res + iz (not the corner layout);
 *   intrinsics (frames,4) fx, fy, cx, cy;  rotation (frames,3,3) row-major and translation (frames,3): q = R p + t, as pn2s_tsdf_integrate;
 *   depth (frames,h,w) fp32 out: the hit's depth z, 0 where there is none (the hit mask is depth > 0);
 *   normal (frames,h,w,3) fp32 out, unit, camera frame, (0,0,0) where there is no hit or no gradient; NULL skips its six samples.
 * Per pixel (u,v), fp32 (the exact expressions, with their fmaf, are at the head of sdf_raycast.hip):
 *   ray     c = ((u - cx) / fx, (v - cy) / fy, 1), flip_yz = 1 negates c_y and c_z;  o = -R^T t,  d = R^T c,  speed = |d|.  The ray
 *           parameter is the DEPTH z (the projective distance of pn2s_tsdf_integrate), the point o + z d;
 *   box     the trilinear domain [lo, hi]^3, lo = -(res / 2) voxel_scale, hi = lo + (res - 1) voxel_scale: a slab test gives
 *           [z_in, z_out], z_in = max(z_in, 1e-3); no ray unless z_out > z_in (a NaN gives no ray);
 *   sample  s(z): the trilinear value at o + z d, grid coordinate (p - lo) / voxel_scale clamped to [0, res - 1], cell
 *           min((int)g, res - 2), blended in the order of the reference's Distance (optimization_obj.py:223-226), NOT clamped to +-0.05;
 *   march   z = z_in; no hit unless s(z_in) > 0.  At most max_steps times: dz = max(s step_scale, min_step voxel_scale) / speed,
 *           z' = min(z + dz, z_out), s' = s(z'); s' <= 0 brackets the surface in [z, z']; otherwise z' >= z_out is no hit.  Out of
 *           steps is no hit: the loop is bounded by the count, not by convergence, and a NaN sample never hits and never stalls it;
 *   refine  `refine` bisections keeping s > 0 at the near end and s <= 0 at the far end, then one linear interpolation
 *           z_hit = z_a + (z_b - z_a) s_a / (s_a - s_b);
 *   normal  central differences of s at p_hit +- 0.5 voxel_scale per axis, normalised (a zero gradient stays (0,0,0)), n = R g,
 *           flip_yz applied.
 * No atomics, no scratch; every pixel is written once; two runs are bitwise equal, `frames` frames in one launch equal `frames`
 * launches of one, and the depth does not depend on whether normals are asked for.  No host sync or allocation (capturable).
 * Refused with nothing launched, checked in this order: a NULL record (PN2_ENULL);  PN2_EINVAL for res < 2, frames < 1, h or w < 1,
 *   vol_f16 / flip_yz not 0 / 1, voxel_scale, step_scale or min_step not finite and > 0, refine outside [0, 16], max_steps < 1;
 *   PN2_ERANGE for res > 512, h w >= 2^29, frames > 65535 or h > 8 * 65535 (the grid's second dimension);  PN2_ENULL for a NULL
 *   pointer other than `normal`.
 */
struct pn2s_raycast {
    const void *volume;
    const float *intrinsics;
    const float *rotation;
    const float *translation;
    float *depth;
    float *normal; /* may be NULL */
    float voxel_scale, step_scale, min_step;
    int res, vol_f16, frames, h, w, flip_yz, refine, max_steps;
    int pad_; /* to 96 bytes; not read */
}; /* 96 bytes */
typedef struct pn2s_raycast pn2s_raycast;
int pn2s_volume_raycast(const pn2s_raycast *raycast, void *stream);

/*
 * Rendered frames compared with the observed ones (sdf_raycast.hip: sdf_raycast_compare_kernel), one workgroup per frame.
 *   rendered (frames,h,w) fp32: Z, what pn2s_volume_raycast wrote (a hit: Z > 0);
 *   depth (frames,h,w) and seg (frames,hs,ws,c), depth_u16 / depth_scale, channel / value: the observed frames, decoded and
 *          addressed exactly as pn2s_tsdf_integrate does (D valid: finite and > 0; pixel (v,u) reads seg[v / f, u / f]);
 *   out (frames,4) fp32.
 * With  A = the object's pixels with valid depth,  Occ = the other pixels with valid depth where the model hits and
 * D < Z - occl_margin (something -- the hand -- is in front of the model),  B = the hit pixels outside Occ:
 *   out[k] = ( |A n B|,  |A u B|,  sum over A n B of |D - Z|,  |Occ| )
 * counted in integers and converted once; the sum in fp32 in a fixed order.  No atomics: two runs are bitwise equal.
 * Refused with nothing launched, checked in this order: a NULL record (PN2_ENULL);  PN2_EINVAL for frames < 1, a size < 1, h / hs and
 *   w / ws not one integer factor, c not 1 or 3, channel outside [0, c), value outside [0, 255], depth_u16 not 0 / 1, depth_u16 = 1
 *   with a depth_scale that is not finite and > 0, occl_margin not finite or < 0;  PN2_ERANGE for h w >= 2^29 or frames > 65535;
 *   PN2_ENULL for a NULL pointer.
 */
struct pn2s_raycast_frames {
    const float *rendered;
    const void *depth;
    const unsigned char *seg;
    float *out;
    double depth_scale;
    float occl_margin;
    int frames, h, w, hs, ws, c, depth_u16, channel, value;
}; /* 80 bytes */
typedef struct pn2s_raycast_frames pn2s_raycast_frames;
int pn2s_raycast_compare(const pn2s_raycast_frames *frames, void *stream);

/*
 * The tracked object pose refined by damped Gauss-Newton on the SDF volume (hotrack_amd/csrc/sdf_refine.hip): `iters`
 * Levenberg-Marquardt steps on  sum_j w_j phi(R^T (p_j - t))^2  from the pose handed in (the particle optimum of pn2s_obj_optimize),
 * ONE launch, one workgroup of 256 lanes per problem, no host synchronisation.  The reference has no such step.  pn2s_refine is HOST
 * memory, read during the call; its pointers are DEVICE memory:
 *   pcld    (n,3) camera-frame points; the batch entry: the packed clouds (sum_k n_k, 3);
 *   volume  the CORNER layout of pn2s_build_corner_volume, vol_fmt 2 (fp32) or 3 (fp16); res, bbox_min and stride as pn2s_trilinear;
 *   poses   in/out (problems,12): rotation (3,3) row-major, then translation (3); the object-frame point is q = R^T (p - t);
 *   stats   out (problems,8): initial cost, final cost, initial and final count of weighted points, accepted steps, final lambda, 0, 0;
 *   trace   out (problems, iters + 1, PN2S_REFINE_TRACE_ROW) or NULL: the state after every pass (layout: head of sdf_refine.hip).
 * The rule, fp32 (every expression, with its fmaf, is at the head of sdf_refine.hip):
 *   residual  r = the trilinear value at q in Distance's operation order (optimization_obj.py:223-226), NOT clamped to +-0.05;
 *   gradient  g = the exact derivative of that interpolant inside its cell, from the same eight corner values, divided by stride;
 *   Jacobian  for  R <- R exp([omega]x),  t <- t + dt:   d r / d omega = g x q,   d r / d dt = -R g;
 *   weight    0 unless |r| < band, the grid coordinate lies strictly inside (0, res - 1) on every axis (the cell is not on the
 *             volume's clamped border) and the sample is finite; else Huber's with the knee at band / 2: min(1, (band / 2) / |r|);
 *   pass      A = sum w J J^T (21 values), b = sum w J r (6), E = sum w r^2, n = the number of weighted points: per lane in point
 *             order, per wave by xor butterfly, the four waves in order;  cost C = E / max(n, 1);
 *   decision  a step is accepted when C <= the accepted cost and n >= half the accepted count: lambda = max(lambda / 3, 1e-7);
 *             otherwise the accepted pose stays and lambda = min(10 lambda, 1e7).  lambda starts at 1e-3;
 *   step      (A + lambda diag(A) + 1e-5 max(n, 1) I) delta = -b of the ACCEPTED pose by an unrolled 6 x 6 Cholesky;  fewer than 6
 *             weighted points, a pivot that is not positive, a delta that is not finite or whose predicted gain -b . delta is below
 *             1e-3 of the accepted E (converged): no step this pass, lambda x 10;
 *             R' = R exp([omega]x) re-projected by pn2s_obj_optimize's ortho6d rule, t' = t + dt.
 *   iters steps are iters + 1 passes (the last one evaluates and decides); the result is the accepted pose, so the final cost
 *   is never above the initial one.  No atomics, no scratch; two runs are bitwise equal; nothing is allocated (capturable).
 * pn2s_obj_refine: problems == 1, n >= 1 points, `volume`; cloud_off and vols are not read.
 * pn2s_obj_refine_batch: a grid of `problems` workgroups; cloud_off is a DEVICE array of problems + 1 ints, in points, problem k
 *   owning rows [cloud_off[k], cloud_off[k+1]) of pcld (inside it: the caller's duty), vols a DEVICE array of `problems` volume
 *   pointers of one vol_fmt, res, bbox_min and stride: pn2s_obj_optimize_batch's conventions (one slice rule on the device).  A problem with an empty slice is
 *   INACTIVE: its pose, stats and trace keep every byte and its table entry, which may be NULL, is never dereferenced.  Every
 *   problem's outputs are bit for bit the single entry's (the same device code).  n and volume are not read; problems == 0 is a
 *   no-op.
 * Refused with nothing launched, checked in this order: a NULL record (PN2_ENULL);  PN2_EINVAL for problems < 0 (the single entry:
 *   != 1, or n < 1), iters < 0, res < 2, vol_fmt not 2 / 3, stride or band not finite and > 0, bbox_min not finite;  PN2_ERANGE for
 *   iters > PN2S_REFINE_MAX_ITERS, res > 1024, problems > PN2S_REFINE_BATCH_MAX;  PN2_ENULL for a NULL pointer other than `trace`.
 */
#define PN2S_REFINE_MAX_ITERS 64
#define PN2S_REFINE_TRACE_ROW 72
#define PN2S_REFINE_BATCH_MAX 65535
struct pn2s_refine {
    const float *pcld;
    const int *cloud_off;     /* batch entry only */
    const void *volume;       /* single entry only */
    const void *const *vols;  /* batch entry only */
    float *poses;
    float *stats;
    float *trace; /* may be NULL */
    float bbox_min, stride, band;
    int problems, n, res, vol_fmt, iters;
}; /* 88 bytes */
typedef struct pn2s_refine pn2s_refine;
int pn2s_obj_refine(const pn2s_refine *refine, void *stream);
int pn2s_obj_refine_batch(const pn2s_refine *refine, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PN2_SDF_H */
