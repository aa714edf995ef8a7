/*
 * pn2_ext.h -- MI355X-side extensions of libpn2_hip.so that have NO counterpart in the
 * reference's native module: work the reference does in Python/torch around the operator
 * stack, moved onto the device so a HandTrackNet forward has no host round trip and the
 * grouped tensors are never materialised.  Same conventions as pn2_hip.h (fp32/int32,
 * contiguous, caller allocates, async on `stream`, PN2_* return codes).
 */
#ifndef PN2_EXT_H
#define PN2_EXT_H

#include "pn2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Batched rigid alignment  y ~= R x + t  of `num` 3-D point pairs (Kabsch / Horn).
 *   reference: network/models/hand_utils.py:42-66 (solve_rot_and_trans: 3x3 cross-covariance,
 *   torch.svd ON THE CPU with a device->host->device hop per forward, det-corrected rotation).
 * Here: one thread per batch element, Horn's unit-quaternion form (largest eigenvector of the
 * 4x4 symmetric matrix built from the cross-covariance) solved by cyclic Jacobi in fp64.
 * x: (xb, num, 3) with xb == b, or xb == 1 (one template shared by the whole batch);
 * y: (b, num, 3);  R: (b, 3, 3) row-major;  t: (b, 3, 1).
 */
int pn2x_kabsch(int b, int xb, int num, const float *x, const float *y, float *R, float *t, void *stream);
/*
 * Gradient of a loss with respect to y through the fit (R, t) = pn2x_kabsch(x, y), in closed form (no solver library, one
 * launch; what autograd computes through torch.svd in the reference's training losses, hand_network.py:186-190 via
 * hand_utils.py:42-66).  R (b,3,3) as returned by pn2x_kabsch; grad_R (b,3,3) / grad_t (b,3) may be NULL (= zero);
 * grad_y (b,num,3) is written.  x carries no gradient (the palm template).
 * A fit whose points are collinear or coincident (or whose mirrored target has two equal singular values) has no unique
 * rotation and no derivative of it: the 3x3 system K of the closed form is singular (|det K| <= 1e-12 tr(Sym)^3).  Such a
 * fit's rows receive the translation term alone, grad_y[i] = grad_t / num -- finite, zero without grad_t -- and never Inf or
 * NaN.  Every fit is computed by its own thread from its own rows: a singular fit changes no other fit's rows by a bit.
 */
int pn2x_kabsch_backward(int b, int xb, int num, const float *x, const float *y, const float *R, const float *grad_R,
                         const float *grad_t, float *grad_y, void *stream);

/*
 * Hand frame in one launch: Kabsch fit of the palm template to kp[:, palm_idx] (num <= 16 indices, device int32)
 * followed by the canonicalisation of the cloud and of the keypoints,
 *   xyz2[b,i,:] = R_b^T (points[b,i,:] - t_b) / scale      xyz1[b,k,:] = R_b^T (kp[b,k,:] - t_b) / scale
 * (reference hand_network.py:100,118-119 + hand_utils.py:30-31,42-66: ransac_rt with a CPU SVD, torch.cat,
 * transpose, matmul, divide).  points (b,n,3), kp (b,j,3), palm_template (xb,num,3) with xb in {1,b};
 * outputs R (b,3,3), t (b,3,1), xyz2 (b,n,3), xyz1 (b,j,3), all point-major.  n == 0: points and xyz2 may be NULL.
 * xyz2_copy (or NULL): a second copy of xyz2 into three columns of a wider row buffer (row stride copy_ld floats).
 * nonfinite (device int32, b entries, or NULL): per-cloud flag, 1 when the cloud, the keypoints or the fit of cloud b contain
 * a NaN / Inf.  Handed to pn2x_pose_head, it turns that frame's predicted keypoints into NaN: the fused inference kernels
 * drop NaNs in their ReLU / max-pool maxima (built -fno-honor-nans), whereas in the reference a non-finite input point
 * spreads through sampling, grouping and the global max-pool to every output of its frame.
 */
int pn2x_hand_frame(int b, int xb, int num, int n, int j, const float *palm_template, const float *kp,
                    const int *palm_idx, const float *points, float scale, float *R, float *t, float *xyz2,
                    float *xyz1, float *xyz2_copy, int copy_ld, int *nonfinite, void *stream);

/*
 * Fused grouped MLP + max of one set-abstraction scale, eval mode (BatchNorm folded into the
 * 1x1 convolutions by the caller).  Replaces, for one (radius | kNN) scale, the reference's
 *   group(points, idx) / group(xyz, idx) - centre / cat / [Conv2d 1x1 + BN2d + ReLU] x3 / max over K
 * (pointnet_utils.py:389-403 for SA-MSG, :566-581 for GivenCenterPoints) without ever
 * materialising the (B, C, S, K) grouped tensors.
 *
 * Layer 1 is linear in its input [feat_j | xyz_j - c_s | centre_feat_s], so it is split:
 *   a1f  (b, n, a1f_ld) or NULL  per-point feature term  W1[:, feat] . feat_j  (point-major rows of
 *                            a1f_ld >= c1 floats; a GEMM over the n points instead of the s*k positions)
 *   xyz  (b, n, 3)  or NULL  point coordinates; with cxyz (b, s, 3) centroids and wx (c1, 3) =
 *                            W1[:, xyz] the kernel adds  wx . (xyz_j - c_s)  itself
 *   b1   (c1)       or NULL  layer-1 bias
 *   cadd (b, s, cadd_ld) or NULL  per-centroid term  W1[:, centre] . centre_feat_s
 * and for every centroid s and neighbour j = idx[b,s,k] (idx: (b, s, k) int32) computes
 *   h1 = relu(a1f[j] + wx.(xyz_j - c_s) + b1 + cadd_s);  h2 = relu(w2 h1 + b2);  h3 = w3 h2 + b3;
 *   out[b*out_b + s*out_s + c*out_c] = relu(max_k h3[c])
 * (out strides in floats: channel-major (b,c3,s) = {c3*s, 1, s}; point-major rows of a wider
 * (b, s, ld) buffer = {s*ld, ld, 1}, which lets the caller skip the reference's torch.cat).
 * w2 (c2, c1), w3 (c3, c2) row-major, BN folded.  fp32 throughout (matrix cores:
 * v_mfma_f32_16x16x4_f32, exact fp32).  Supported: k in {16,32,64} and (c1,c2,c3) in
 * {(32,32,64), (64,64,128), (128,128,192)} -- PN2_ERANGE otherwise (query with
 * pn2x_sa_mlp_max_supported; callers keep the unfused operator path for other shapes).
 *
 * Return codes of pn2x_sa_mlp_max, pn2x_sa_mlp_max_classes and, per record, pn2x_sa_mlp_max_pair -- one shared check; a call
 * with several faults gets the first of:
 *   1. a size below its minimum (b < 0; n, k < 1; s < 0, in a pair record s < 1)            PN2_EINVAL
 *   2. an empty problem (b = 0, or s = 0 in the positional entries): nothing is done        PN2_OK
 *   3. a required pointer NULL (an operand without its companions counts: xyz needs cxyz and wx)   PN2_ENULL
 *   4. a1f_ld / cadd_ld below c1 or no multiple of 4; a1f, cadd, b1, w2, w3 (cls_list) not 16-byte aligned   PN2_EINVAL
 *   5. beyond a limit of the addressing (24-bit rows and strides, 32-bit offsets), or a k / width set / operand set without an
 *      instantiation                                                                        PN2_ERANGE
 * The pair refuses a NULL record (PN2_ENULL) before step 2 and tests pn2x_sa_mlp_max_pair_supported right after it, before it
 * reads anything else of its records.
 */
int pn2x_sa_mlp_max(int b, int n, int s, int k, int c1, int c2, int c3, const float *a1f, int a1f_ld,
                    const float *xyz, const float *cxyz, const float *wx, const float *b1, const float *cadd,
                    int cadd_ld, const int *idx,
                    const float *w2, const float *b2, const float *w3, const float *b3, float *out,
                    long out_b, int out_s, int out_c, void *stream);
int pn2x_sa_mlp_max_supported(int k, int c1, int c2, int c3);

/*
 * pn2x_sa_mlp_max on ball-query lists without their padding ("class walk", csrc/sa_fused.hip).  idx (b, s, 32) are lists
 * whose slots past counts[b, s] repeat slot 0 (pn2x_ball_query_picks_counts).  A centroid is served with its first 8, 16 or 32
 * slots -- the smallest of the three that holds its count -- so layers 2 and 3 run over about a quarter of the positions when
 * most lists are short.  The result is BIT-IDENTICAL to pn2x_sa_mlp_max on the same idx: each position's output is independent
 * of the tile it sits in, and the max over a list equals the max over the list without its duplicates.
 *
 * pn2x_sa_class_lists: counts (b*s) -> list (b*s, 4) int32 records {b*s' id = cloud * s + centroid, cloud * n, cloud, centroid},
 *   class "32" (count 17..32) first, then "16" (9..16), then "8" (<= 8), ascending id inside a class; sizes[0..2] = the three
 *   class sizes.  n: points per cloud of the level the lists index.  One launch of one workgroup, deterministic, nothing reaches
 *   the host.  list 16-byte aligned; b*s and b*n below 2^24 (PN2_ERANGE).  b = 0 writes sizes = 0, 0, 0.
 * pn2x_sa_class_lists2: two such problems (both levels of a forward: level 2's counts depend on geometry only) in ONE launch, a
 *   workgroup each; the checks of pn2x_sa_class_lists hold for either problem.
 * pn2x_sa_mlp_max_classes: the arguments of pn2x_sa_mlp_max plus list and sizes; one persistent launch whose workgroups read
 *   the class sizes on the device and each walk an equal contiguous share of the tiles, class 32 first (capturable; a replay on
 *   inputs with another class mix is correct).  Supported (pn2x_sa_mlp_max_classes_supported): k = 32 and widths (32,32,64) or
 *   (64,64,128); cadd rows and out rows of consecutive clouds must continue each other (cloud stride = s * row stride for cadd;
 *   any out_b).  Honours pn2x_sa_set_compute_units.
 */
int pn2x_sa_class_lists(int b, int s, int n, const int *counts, int *list, int *sizes, void *stream);
int pn2x_sa_class_lists2(int b0, int s0, int n0, const int *counts0, int *list0, int *sizes0, int b1, int s1, int n1,
                         const int *counts1, int *list1, int *sizes1, void *stream);
int pn2x_sa_mlp_max_classes_supported(int k, int c1, int c2, int c3);
int pn2x_sa_mlp_max_classes(int b, int n, int s, int k, int c1, int c2, int c3, const float *a1f, int a1f_ld,
                            const float *xyz, const float *cxyz, const float *wx, const float *b1, const float *cadd,
                            int cadd_ld, const int *idx, const int *cls_list, const int *cls_sizes,
                            const float *w2, const float *b2, const float *w3, const float *b3, float *out,
                            long out_b, int out_s, int out_c, void *stream);

/*
 * In-place y[b,c,n] = act(y[b,c,n] + bias[c]) (relu != 0 -> ReLU): the epilogue of an eval-mode,
 * BatchNorm-folded 1x1 convolution (reference: Conv1d + BatchNorm1d + ReLU of the feature-propagation
 * stacks, pointnet_utils.py:460-462) whose GEMM half is a library GEMM on the (b, c, n) tensor.
 */
int pn2x_bias_act(int b, int c, int n, float *y, const float *bias, int relu, void *stream);

/*
 * three_nn that returns interpolation WEIGHTS: idx (b,n,3) as pn2_three_nn, and
 *   weight[t] = (1/(sqrt(d2_t)+1e-8)) / sum_t (1/(sqrt(d2_t)+1e-8))
 * i.e. the sqrt of pointnet2_utils.py:135 plus the three torch kernels of the reference's caller
 * (pointnet_utils.py:447-449) folded into the search kernel's epilogue.  Needs m >= 3.
 */
int pn2x_three_nn_weights(int b, int n, int m, const float *unknown, const float *known, float *weight, int *idx,
                          void *stream);

/*
 * pn2x_three_nn_interpolate_pm: pn2x_three_nn_weights followed by pn2x_three_interpolate_pm in ONE launch, for callers that need
 * the (weight, index) pair for nothing else (the forward of feature propagation, pointnet_utils.py:440-453): out (b, n, ldo) rows
 * <- the inverse-distance blend of the three nearest `known` (b,m,3) points' rows of `points` (b, m, ldp), c columns.  Same floats
 * as the two calls.  PN2_ERANGE unless pn2x_three_nn_interpolate_pm_supported (2^14 <= b n < 2^18 queries, 16 <= m <= 2048 known points in
 * one LDS tile, c / ldp / ldo multiples of 4, points / out 16-byte aligned): the caller then runs the two launches.
 */
int pn2x_three_nn_interpolate_pm_supported(int b, int n, int m, int c, int ldp, int ldo);
int pn2x_three_nn_interpolate_pm(int b, int n, int m, int c, const float *unknown, const float *known, const float *points, int ldp,
                                 float *out, int ldo, void *stream);
/*
 * three_interpolate on POINT-MAJOR features: points (b, m, ldp), out (b, n, ldo), c <= ldp, ldo channels
 * per row; out[b,j,ch] = sum_t weight[b,j,t] * points[b, idx[b,j,t], ch]  (same arithmetic as
 * pn2_three_interpolate).  `out` may point at a column block of a wider row (ldo > c).
 */
int pn2x_three_interpolate_pm(int b, int c, int m, int n, const float *points, int ldp, const int *idx,
                              const float *weight, float *out, int ldo, void *stream);
/*
 * pn2x_three_nn_interpolate_pm_rows: pn2x_three_nn_interpolate_pm for the query rows a device-side list names.  For cloud b only
 * the rows row_list[b, 0 : row_counts[b, 1]] (row_list (b, n), row_counts (b, 2): the pair pn2x_row_lists writes; any order, entries
 * outside 0 .. n-1 are skipped) get their search, weights and blend, written to the same place in `out`; no other row of `out` is
 * touched.  Every listed row holds the floats the full launch writes there.  The grid covers n rows per cloud and workgroups past a
 * cloud's count leave after reading it, so the count never reaches the host (capturable; a replay on other lists is correct).
 * PN2_ERANGE unless pn2x_three_nn_interpolate_pm_rows_supported (3 <= m <= 2048, c / ldp / ldo multiples of 4, b <= 65535) and
 * points / out 16-byte aligned -- there is no other route for a listed launch.
 */
int pn2x_three_nn_interpolate_pm_rows_supported(int b, int n, int m, int c, int ldp, int ldo);
int pn2x_three_nn_interpolate_pm_rows(int b, int n, int m, int c, const float *unknown, const float *known, const float *points,
                                      int ldp, float *out, int ldo, const int *row_list, const int *row_counts, void *stream);
/*
 * pn2x_three_nn_interpolate_pm_rows_act: the listed-rows launch with an epilogue,
 *     out[r, ch] = act(blend[r, ch] + wx[ch, 0] x + wx[ch, 1] y + wx[ch, 2] z + bias[ch]),   (x, y, z) = unknown[r],
 * act = max(., 0) when relu != 0, the identity otherwise.  It is what remains of a per-point layer over [blend | xyz] rows once the
 * layer's feature half has been applied to `points` (the blend is a convex combination of rows and commutes with a linear map).
 * Order of the sum per channel: the blend as pn2x_three_nn_interpolate_pm_rows forms it, then the x, y and z terms as one fma each
 * in that order, then the bias.  wx (c, 3) and bias (c) contiguous and 16-byte aligned.  row_list and row_counts both NULL: every
 * row of every cloud gets the search, the blend and the epilogue (the floats the listed launch writes there).  Everything else as
 * pn2x_three_nn_interpolate_pm_rows; pn2x_three_nn_interpolate_pm_rows_act_supported adds c <= 1024 (wx and bias are held in LDS).
 */
int pn2x_three_nn_interpolate_pm_rows_act_supported(int b, int n, int m, int c, int ldp, int ldo);
int pn2x_three_nn_interpolate_pm_rows_act(int b, int n, int m, int c, const float *unknown, const float *known, const float *points,
                                          int ldp, float *out, int ldo, const int *row_list, const int *row_counts, const float *wx,
                                          const float *bias, int relu, void *stream);

/*
 * Two-level furthest point sampling without the second pass.  PointNet++ samples level 2 from level 1's samples
 * (reference backbones.py:98-104: FPS 1024 -> 256, then FPS 256 -> 128 over those 256).  FPS is greedy, and every
 * pick is the arg-max over ALL remaining points, so it is also the arg-max over the subset of picked points: as long
 * as no arg-max among the first m2 picks of level 1 was a tie, level 2's sample is exactly level 1's first m2 picks,
 * in order, i.e. idx2 = 0..m2-1 -- same distances, same min() chain, same floats.  With a tie the two passes may
 * break it differently (their tie keys use different point numberings), so the second pass is then really run.
 *   pn2x_furthest_point_sampling_radii : pn2_furthest_point_sampling that also records radii (b, m): radii[i] = the
 *             running-minimum distance of pick i when it was selected (the maximum of step i); radii[0] is unused.
 *   pn2x_fps_prefix_ties : given that run (xyz (b,n,3), picks idx1 (b,m1), radii (b,m1)), decide per cloud whether any
 *             arg-max of picks 1..m2-1 was tied.  With the picks known this has no dependency chain: every point
 *             replays its running minimum against the picks in order (same sqdist / min chain, same floats) and
 *             compares it with radii[i]; fully parallel (the prefix-min is also split over four threads per point), one workgroup
 *             per 64 points.
 *             flags: (b, pn2x_fps_prefix_flags(n)) ints, one per workgroup, non-zero = tie seen (conservative: a
 *             duplicate of a pick counts).
 *   pn2x_furthest_point_sampling_prefix : FPS over xyz (b, n, 3) -> idx (b, m), m <= n, really computed only for
 *             clouds with a non-zero flag; the others get idx = 0..m-1 (the launch returns at once).
 * They cover m2 <= 1024 and the register-resident sampling kernels (n <= 16384 points after padding).
 */
int pn2x_furthest_point_sampling_radii(int b, int n, int m, const float *xyz, int *idx, float *radii, void *stream);
/*
 * pn2x_fps_radii_knn: pn2x_furthest_point_sampling_radii AND pn2x_knn_indices (the nq query points per cloud `query` (b,nq,3) among
 * the same xyz; knn_idx (b,nq,k) sorted by (distance, index), knn_idx2 (b,nq,k2) its prefix when k2 > 0) in ONE launch: the first b
 * workgroups sample, the others search.  The sampling is a serial chain on one compute unit per cloud (pointnet_utils.py:368 ->
 * sampling_gpu.cu:94-209); the keypoints' neighbour lists (pointnet_utils.py:551-556) need nothing but the coordinates, so at small
 * batch (the tracking loop, track_network.py:159-217) they ride along instead of costing 21 us + a launch of their own.
 * Same results as the two calls.  PN2_ERANGE unless pn2x_fps_radii_knn_supported(n, nq, k): 512 < padded n <= 1024.
 */
int pn2x_fps_radii_knn_supported(int n, int nq, int k);
int pn2x_fps_radii_knn(int b, int n, int m, const float *xyz, int *idx, float *radii, int nq, int k, int k2, const float *query,
                       int *knn_idx, int *knn_idx2, void *stream);
int pn2x_fps_prefix_ties(int b, int n, int m1, int m2, const float *xyz, const int *idx1, const float *radii, int *flags, void *stream);
/*
 * pn2x_ball_query_picks_ties: pn2x_ball_query_picks (ball query around the picks (b, m) of a sampling run + their coordinates) AND
 * pn2x_fps_prefix_ties (was an arg-max among the first m2 picks tied?  radii (b, m) from the sampling run, flags as above) in ONE
 * launch -- both consume the picks and nothing of each other.  Same outputs as the two calls.  PN2_ERANGE unless
 * pn2x_ball_query_picks_ties_supported(b, n, m, m2): small batches (b n <= 16384, the tracking loop), m2 <= 1024.
 */
int pn2x_ball_query_picks_ties_supported(int b, int n, int m, int m2);
int pn2x_ball_query_picks_ties(int b, int n, int m, float radius, int nsample, const float *xyz, const int *picks, float *new_xyz,
                               int *idx, float *new_xyz_copy, int copy_ld, int m2, const float *radii, int *flags, void *stream);
int pn2x_fps_prefix_flags(int n);
int pn2x_furthest_point_sampling_prefix(int b, int n, int m, const float *xyz, const int *flags, int nflags, int *idx, void *stream);

/*
 * pn2_knn without the distance output, plus (k2 > 0) the first k2 indices of every list as a second contiguous
 * (b, n, k2) tensor: the k-NN list is sorted by (distance, index), so a smaller neighbourhood is its prefix -- the
 * reference searches twice (GivenCenterPoints scales 16 and 64, pointnet_utils.py:560-565).  m <= 2048.
 */
int pn2x_knn_indices(int b, int n, int m, int k, int k2, const float *unknown, const float *known, int *idx, int *idx2, void *stream);

/*
 * pn2_ball_query whose centroids are given as indices into the cloud itself (picks (b, m) int32, values in [0, n):
 * the output of FPS), which is how PointNet++ always calls it (pointnet_utils.py:379-382: sample, gather, query).
 * Also writes the centroids' coordinates new_xyz (b, m, 3) = xyz[picks], so the gather launch disappears.
 * new_xyz_copy (or NULL): a second copy of the coordinates into three columns of a wider row buffer (row stride copy_ld
 * floats; the consumer's [feat | xyz] GEMM input, so the reference's torch.cat of pointnet_utils.py:493 is not needed).
 */
int pn2x_ball_query_picks(int b, int n, int m, float radius, int nsample, const float *xyz, const int *picks, float *new_xyz,
                          int *idx, float *new_xyz_copy, int copy_ld, void *stream);
/*
 * The same launches with one more output: counts (b, m) int32 (or NULL: exactly the calls above) = min(hits, nsample) of every
 * centroid, 1 for a centroid without a hit (its list is all point 0, so its first slot alone gives the same pooled result).
 * A list's slots past its count repeat slot 0 (ball_query_gpu.cu:35-39), which is what pn2x_sa_mlp_max_classes skips.
 */
int pn2x_ball_query_picks_counts(int b, int n, int m, float radius, int nsample, const float *xyz, const int *picks, float *new_xyz,
                                 int *idx, float *new_xyz_copy, int copy_ld, int *counts, void *stream);
int pn2x_ball_query_picks_ties_counts(int b, int n, int m, float radius, int nsample, const float *xyz, const int *picks, float *new_xyz,
                                      int *idx, float *new_xyz_copy, int copy_ld, int m2, const float *radii, int *flags, int *counts,
                                      void *stream);

/*
 * pn2_ball_query through a cell grid (csrc/ball_query_grid.hip): identical output for every input -- the same hit test on
 * the same pairs, emitted in ascending index order with the reference's first-hit padding (ball_query_gpu.cu:34-43) --
 * but only the points in the 3x3x3 cells around a centroid are tested, in blocks of consecutive indices with the
 * reference's early exit after the nsample-th hit.  For clouds of n >= 2048 points (PN2_ERANGE below that and for
 * radius <= 0: callers run pn2_ball_query).  scratch: pn2x_ball_query_grid_scratch_words(b, n) 4-byte words, 16-byte
 * aligned, contents irrelevant (the per-cloud grid is rebuilt by every call).  pn2_ball_query itself takes this path for
 * large problems when it can use library-owned scratch (i.e. outside stream capture).
 */
long pn2x_ball_query_grid_scratch_words(int b, int n);
int pn2x_ball_query_grid(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                         void *scratch, long scratch_words, void *stream);

/*
 * Row gather on point-major data: out[b, j, :] = src[b, idx[b,j], :]  (src (b,n,c), idx (b,m), out (b,m,c)).
 * The point-major twin of pn2_gather_points (used for the FPS-selected centroid coordinates).
 */
int pn2x_gather_rows(int b, int n, int m, int c, const float *src, const int *idx, float *out, void *stream);

/*
 * In-place point-major epilogue: y[r, ch] = act(y[r, ch] + bias[r / rows_per_bias, ch]) for y (rows, c) with row
 * stride ldy.  rows_per_bias = rows gives an ordinary per-channel bias; rows_per_bias = points-per-cloud adds a
 * per-cloud vector (the broadcast global feature of the reference's fp3 layer, pointnet_utils.py:443-444).
 */
int pn2x_bias_act_pm(long rows, int c, float *y, int ldy, const float *bias, long rows_per_bias, int relu, void *stream);

/*
 * out[b, ch] = max over the r rows of point-major x (b, r, c): the max over N of the reference's group-all
 * set-abstraction layer (pointnet_utils.py:508, torch.max over the point axis).
 */
int pn2x_max_rows(int b, int r, int c, const float *x, float *out, void *stream);

/* n <= pn2x_copy_multi_max() device-to-device copies (dst[i] <- src[i], bytes[i] bytes, non-overlapping) as ONE launch: the batch
 * hand-over of a graph-captured training step (a few batch tensors + the geometry pack into the captured step's static buffers;
 * the reference's trainer.py:278-302 moves a batch with one .to(device) per tensor).  The table travels in the kernel arguments. */
int pn2x_copy_multi_max(void);
int pn2x_copy_multi(int n, void *const *dst, const void *const *src, const long *bytes, void *stream);

/*
 * out = LN2( LN1( x + y + bias ) ) over the last dimension of row-major (rows, c) data, c <= 1024:
 * torch.nn.functional.layer_norm semantics (biased variance, eps inside the square root), affine (g, b) each.
 * y, bias and the second LayerNorm (g2, b2 both NULL) are optional.  One launch for the reference's residual add +
 * LayerNorm runs in the attention-free transformer blocks (transformer.py:84-95 with attn=False) of the 21-token tail.
 */
int pn2x_add_layernorm(long rows, int c, const float *x, const float *y, const float *bias, const float *g1,
                       const float *b1, float eps1, const float *g2, const float *b2, float eps2, float *out, void *stream);

/*
 * rearrange_module (blocks.py) mixes each of j tokens with re - 1 neighbours: out = [f[perm[t,0]] | .. | f[perm[t,re-1]]] W^T.
 * The sum over slots commutes with the gather, so the product runs on the un-gathered tokens against the stacked slot blocks
 * (z = f [W_0 | .. | W_re-1]^T, (b*j) x (re*c), row stride ldz >= re*c floats) and these entries add the permuted slices:
 *   pn2x_perm_sum_rows      out[b,t,:] = sum_r z[b, perm[t,r], r*c : (r+1)*c]        (out (b, j, c) contiguous)
 *   pn2x_add_layernorm_perm out[b,t,:] = LN2( LN1( that sum + bias ) )               (pn2x_add_layernorm's arithmetic; c <= 1024)
 * summed in the order r = 0 .. re-1.  perm is a HOST table, (j, re) int32 row-major, j <= 256, j*re <= 512: the entry checks
 * every entry against [0, j) while it packs the table into the kernel arguments (PN2_EINVAL, nothing launched), so no launch
 * reads a table from device memory and a captured graph holds its own copy.  c % 4 == 0; pn2x_perm_sum_rows moves 16 bytes per
 * lane: z and out 16-byte aligned, ldz % 4 == 0.  bias and the second LayerNorm (g2, b2 both NULL) are optional.
 * pn2x_add_layernorm_perm launches an instance with the slot count fixed at compile time where there is one (re == 5, the
 * network's: every load of a row in flight at once); pn2x_add_layernorm_perm_any_slots always launches the run-time-slot kernel
 * that serves every other re.  Same sums in the same order: the two return the same bits.
 */
int pn2x_perm_sum_rows(int b, int j, int re, int c, const float *z, int ldz, const int *perm, float *out, void *stream);
int pn2x_add_layernorm_perm(int b, int j, int re, int c, const float *z, int ldz, const int *perm, const float *bias,
                            const float *g1, const float *b1, float eps1, const float *g2, const float *b2, float eps2,
                            float *out, void *stream);
int pn2x_add_layernorm_perm_any_slots(int b, int j, int re, int c, const float *z, int ldz, const int *perm, const float *bias,
                                      const float *g1, const float *b1, float eps1, const float *g2, const float *b2, float eps2,
                                      float *out, void *stream);

/*
 * Head of HandTrackNet (hand_network.py:141-147): delta = h W^T + bias (W (3, c): the last Conv1d), kp_hand = delta +
 * xyz1, kp_cam = (kp_hand R^T) * scale + t.  h (b*j, c) token-major; xyz1, kp_hand, kp_cam (b, j, 3); R (b,3,3); t (b,3,1).
 * nonfinite: the per-cloud flags of pn2x_hand_frame (or NULL): flagged frames get NaN keypoints in both frames.
 */
int pn2x_pose_head(int b, int j, int c, const float *h, const float *w, const float *bias, const float *xyz1,
                   const float *R, const float *t, float scale, float *kp_hand, float *kp_cam, const int *nonfinite,
                   void *stream);

/* One problem of pn2x_sa_mlp_max_pair (below) = the per-scale arguments of pn2x_sa_mlp_max, under their names there. */
typedef struct pn2x_sa_problem {
    int n, s, k;
    const float *a1f;
    int a1f_ld;
    const float *xyz, *cxyz, *wx, *b1, *cadd;
    int cadd_ld;
    const int *idx;
    const float *w2, *b2, *w3, *b3;
    float *out;
    long out_b;
    int out_s, out_c;
} pn2x_sa_problem;
/*
 * Number of compute units the persistent grids of pn2x_sa_mlp_max / _pair / pn2x_mlp2_rows may occupy (0 = all, the default;
 * also PN2_SA_CUS in the environment).  A workgroup of these kernels fills its CU, so a caller that keeps several batches in
 * flight on different streams gains by leaving a few CUs to the other stream (bench.py: 240 of 256 with two in flight).
 */
int pn2x_sa_set_compute_units(int n);
/*
 * pn2x_mlp2_rows: out[r, :] = relu(W3 relu(W2 x[r, :c1] + W2e x[r, c1:c1+3] + b2) + b3) for `rows` point-major rows (x: ldx
 * floats apart; out: ldo floats apart, c3 written; BatchNorm folded into W / b by the caller) -- two consecutive
 * [Conv1d 1x1 + BN + ReLU] layers of a feature-propagation MLP (pointnet_utils.py:504-506) in ONE launch: the tile loop of
 * pn2x_sa_mlp_max without neighbourhoods, both weight matrices register-resident, the intermediate activation never
 * written to HBM.  w2 (c2, c1), w3 (c3, c2) row-major, 16-byte aligned.  w2e (c2, 3) or NULL: weights of three more input
 * columns stored right behind the c1 features (the coordinates of an [interpolated | xyz] row; needs ldx >= c1 + 4).
 * x and out 16-byte aligned, ldx and ldo multiples of 4 floats (rows are read and written in 16-byte segments), else PN2_EINVAL.
 * PN2_ERANGE unless pn2x_mlp2_rows_supported(c1, c2, c3).
 */
int pn2x_mlp2_rows_supported(int c1, int c2, int c3);
int pn2x_mlp2_rows(long rows, int c1, int c2, int c3, const float *x, int ldx, const float *w2, const float *w2e, const float *b2,
                   const float *w3, const float *b3, float *out, int ldo, void *stream);
/*
 * Both scales of a keypoint-query module (reference PointNetSetAbstractionMsg_GivenCenterPoints, pointnet_utils.py:536-590:
 * two kNN neighbourhood sizes, same layer widths) in ONE persistent launch: every compute unit stays busy and each
 * workgroup loads only its own scale's weights (see sa_fused.hip).  Supported (pn2x_sa_mlp_max_pair_supported): widths
 * 128-128-192, k = {16, 64}, both problems with the same set of layer-1 operands (a1f + xyz, optionally + cadd); anything else
 * returns PN2_ERANGE (launch them separately).  Each record is checked as pn2x_sa_mlp_max checks its arguments.
 */
int pn2x_sa_mlp_max_pair_supported(int k0, int k1, int c1, int c2, int c3);
int pn2x_sa_mlp_max_pair(int b, int c1, int c2, int c3, const pn2x_sa_problem *p0, const pn2x_sa_problem *p1, void *stream);

/*
 * Per-point layers over the rows a kNN list names (hotrack_amd/csrc/row_chain.hip).
 *
 * pn2x_row_lists: for each cloud b, the distinct points named by gi (b, j, k_large) and gi_small (b, j, k_small) -- or, with
 * gi_small NULL, by the first k_small entries of every gi list.  list (b, n): the points named by a small list in ascending
 * order, then the points named only by a large list in ascending order (entries past the count are not written);
 * counts (b, 2): [points named by a small list, points named by any list].  One workgroup per cloud, n <= 16384.
 *
 * pn2x_row_chain: for every listed point p of cloud b (r = b * n + p),
 *     h1 = relu(Wa [x[r, 0:128] | x[r, 128:131]] + ba)   h2 = relu(Wb h1 + bb)   c = relu(Wc h2 + bc)   out[r, :] = Wq c
 * with Wa (128, 131), Wb (128, 128), Wc (384, 128), Wq (512, 384) BatchNorm-folded: columns [0, 256) of out are written for the
 * points named by a small list, columns [256, 512) for every listed point; nothing else is written.  The weights come in
 * the kernel's operand layout (hotrack_amd/ext.py: row_chain_pack: k padded to a multiple of 16, [n/16][k/16][64][4]).
 * x rows ldx >= 132 floats apart (x[r, 131] is ignored), out rows ldo >= 512 apart; both multiples of 4 floats, 16-byte
 * aligned.  The counts are read on the device (no host sync; capturable).  grid: persistent workgroups, 0 = one per compute
 * unit.  b <= 1024 (PN2_ERANGE otherwise).  Exact fp32 (v_mfma_f32_16x16x4_f32), summation order differs from a GEMM library.
 */
int pn2x_row_lists(int b, int n, int j, int k_large, int k_small, const int *gi, const int *gi_small, int *list, int *counts,
                   void *stream);
int pn2x_row_chain_supported(int c_in, int c_h, int c_conv, int c_q);
int pn2x_row_chain(int b, int n, const float *x, int ldx, const int *list, const int *counts, const float *wa, const float *ba,
                   const float *wb, const float *bb, const float *wc, const float *bc, const float *wq, float *out, int ldo,
                   int grid, void *stream);
/*
 * pn2x_row_chain3: pn2x_row_chain from its second layer on, for callers that already hold h1 (c_h = 128 floats per row, activated):
 *     h2 = relu(Wb h1[r] + bb)   c = relu(Wc h2 + bc)   out[r, :] = Wq c
 * over the same lists, with the same shares, tiles, grid rule, column rule and weight layout; h1 rows ldh >= 128 floats apart.
 * Same checks and error codes as pn2x_row_chain.
 */
int pn2x_row_chain3_supported(int c_h, int c_conv, int c_q);
int pn2x_row_chain3(int b, int n, const float *h1, int ldh, const int *list, const int *counts, const float *wb, const float *bb,
                    const float *wc, const float *bc, const float *wq, float *out, int ldo, int grid, void *stream);

/*
 * sa3 and fp3 of the backbone over the b * s level-2 rows, as row-tiled layer chains (hotrack_amd/csrc/mid_chain.hip).
 * A workgroup runs one tile of 32 rows of one cloud (r = c * s + i for cloud c, row i); s must be a multiple of 32.
 * Weights are BatchNorm-folded and come in the kernels' operand layout (hotrack_amd/ext.py: row_chain_pack: k padded to a
 * multiple of 16, [n/16][k/16][64][4]); biases plain.  Row strides are multiples of 4 floats, every pointer 16-byte aligned.
 * Exact fp32 (v_mfma_f32_16x16x4_f32); summation order differs from a GEMM library.  No atomics: results do not depend on
 * the order in which tiles run.  No host sync (capturable).  Errors: PN2_EINVAL for a bad size, stride, s % 32 != 0 or
 * a misaligned pointer, PN2_ERANGE for b * s >= 2^31, PN2_ENULL for a NULL pointer; b == 0 returns PN2_OK and touches
 * nothing.  Arguments are checked before any device work.
 *
 * pn2x_sa3_chain: for tile t (rows 32 t .. 32 t + 31),
 *     h1 = relu(W1 [x[r, 0:128] | x[r, 128:131]] + b1)   h2 = relu(W2 h1 + b2)   part[t, :] = max over the tile's rows r of
 *     relu(W3 h2 + b3)
 * with W1 (128, 131), W2 (128, 128), W3 (512, 128).  x rows ldx >= 132 floats apart (x[r, 131] is ignored); part is
 * contiguous (b * s / 32, 512) = (b, s / 32, 512): the max over a cloud's s / 32 rows of part is its sa3 output.
 *
 * pn2x_fp3_chain: for every row r of cloud c,
 *     l3 = max over part[c, :, :]   g = Wg l3 + bg   h = relu(Wa x[r, 0:128] + g)   out[r, 0:256] = relu(Wf h + bf)
 * with wgt = Wg^T (512, 256) contiguous (plain layout), Wa (256, 128) and Wf (256, 256) packed.  x rows ldx >= 128 floats
 * apart, out rows ldo >= 256 apart; columns [0, 256) of the b * s out rows are written, nothing else.  Each tile computes
 * its cloud's g itself (the two launches do not wait on each other's workgroups).
 */
int pn2x_sa3_chain_supported(int s, int c_in, int c1, int c2, int c3);
int pn2x_sa3_chain(int b, int s, const float *x, int ldx, const float *w1, const float *b1, const float *w2, const float *b2,
                   const float *w3, const float *b3, float *part, void *stream);
int pn2x_fp3_chain_supported(int s, int c_l2, int c_l3, int c1, int c2);
int pn2x_fp3_chain(int b, int s, const float *x, int ldx, const float *part, const float *wgt, const float *bg, const float *wa,
                   const float *wf, const float *bf, float *out, int ldo, void *stream);

/*
 * Hand shape-code search (reference gf_optimize_hand_shape.optimize, network/models/optimization_hand.py:74-124) in one
 * launch of one 1024-thread workgroup (hotrack_amd/csrc/hand_shape.hip).  The hand's keypoints at the fixed pose are the
 * affine function kp(beta) = k0 + sum_d beta_d k[d] (k0 (21,3), k (d,21,3): HandModel.shape_keypoint_basis).  With h = 0,
 * search = initial_scale (d), prev_search = search, prev_success = 1, each of `iterations` iterations does
 *     sample[q] = pre[q] * search                                  pre (p, d), row 0 zero (the current estimate)
 *     E[q]      = mean_t mean_b | |bone_b(h + sample[q])| - targets[t, b] |      bones / parents of kp2length, targets (t, 15)
 *     w[q]      = (E[0] - E[q]) [E[q] < E[0]]    success = any(E[q] < E[0])
 *     mean_E    = success ? sum w E / sum w : E[0]         mt = success ? sum_q w[q] sample[q] / sum w : 0      h += mt
 *     sz        = |mt| + 1e-3    search = mean_E * scaling_coefficient2 * sz / ||sz|| + 1e-3
 *     if (prev_success && success) search = beta search + (1 - beta) prev_search;  if (success) prev_search = search
 *     prev_success = success
 * and out (d) = h.  trace (iterations, 3 + d) or NULL: per iteration [E[0], mean_E, success (0/1), search after the update].
 * fp32; every sum runs in a fixed order, no atomics: two runs give bitwise-equal results.  No host sync (capturable).
 * 1 <= p <= 8192, 1 <= d <= 16, 1 <= t <= 1024 (pn2x_hand_shape_opt_supported).  Errors: PN2_EINVAL for p, d or t < 1 or
 * iterations < 0, PN2_ERANGE beyond the limits or for iterations * (3 + d) >= 2^31, PN2_ENULL for a NULL pointer other
 * than trace; iterations == 0 returns PN2_OK and touches nothing.  Arguments are checked before any device work.
 */
int pn2x_hand_shape_opt_supported(int p, int d, int t);
int pn2x_hand_shape_opt(int p, int d, int t, int iterations, const float *k0, const float *k, const float *pre,
                        const float *targets, const float *initial_scale, double scaling_coefficient2, double beta, float *out,
                        float *trace, void *stream);

/*
 * Hand-pose particle optimiser (reference gf_optimize_hand_pose.evaluate / optimize, network/models/optimization_hand.py:215-293,
 * :335-394) on the device (hotrack_amd/csrc/hand_pose.hip): hand_pose_eval_kernel evaluates all p candidate hands in one
 * launch, hand_pose_update_kernel (one workgroup) applies an iteration's update.  Two records carry the arguments.
 *
 * pn2x_hand_pose_setup: what the problems of a batch share.  HOST memory, read during the call only.  The hand model is a
 * linear-blend-skinning table (HandModel.skinning_tables):
 *   parents (j) int32, parents[i] < i, joint 0 the root;  pose_block (j) int32: the 3-vector of the 45 joint angles that rotates
 *   joint i, -1 for none;  skin_w (v,k);  skin_pack (v) int32: bits 5i..5i+4 the joint of weight i < k, bits 20..24 the tip regions
 *   (fingers 0..4 of get_attraction_loss) the vertex belongs to;  comps (45,45), rows [0,10) used;  theta_scale (30);  pre (p,16),
 *   row 0 zero: the candidates;  vol_f16 0 / 1, res (odd), voxel_scale: the SDF volumes' type, size and spacing;  w_*: the six
 *   energy weights;  reserved: not read.  Keypoints are the joint positions.
 * posedirs != NULL makes it a hand with MANO's structure (skinning_tables' optional entries; the reference's
 * OurManoLayer.forward, third_party/mano/our_mano.py:218-360); with posedirs NULL the other three fields are not read:
 *   posedirs (ceil16(3 v), 136): the pose blend shapes packed for the matrix cores -- row 3 vertex + coordinate, column
 *     9 b + 3 r + c the weight of (R_b - I)[r][c] of pose block b's own rotation, column 135 and the rows from 3 v on zero;
 *     16-byte aligned.  v_rest += posedirs . features before the skinning.
 *   pose_mean (45): added to the joint angles, theta = pose_mean + (curr_theta + (s[6:16] @ comps[:10]) * theta_scale).
 *   kp_vertex (21) int32: kp_vertex[i] >= 0 makes keypoint i that skinned vertex instead of joint i's position; joint i then has
 *     pose_block -1, is nobody's parent and no weight names it, and bits 25..29 of that vertex's skin_pack hold i (a vertex
 *     serves one keypoint at most); -1 = a joint.  kp_vertex[0] is -1.
 *   centre_root 0 / 1: keypoint 0 (= rest_joints[0]) is subtracted from vertices and keypoints before the translation is added.
 *
 * pn2x_hand_pose_problem: one problem's frame.  state (90, in/out; below);  work: pn2x_hand_pose_opt_work_floats(p) floats of
 * its own (per candidate: energy without attraction, attraction term, penetration, 0);  rest_joints (j,3), rest_verts (v,3):
 * rest + beta @ shape_* (they carry the sequence's shape code);  pred_kp (21,3);  last_kp (21,3) or NULL;  vis_mask (21 bytes);
 * obj_r (3,3), obj_t (3);  vol res^3 fp16 / fp32 (problems may share one);  mask: the h x w byte image (non-zero = background);
 * fx, fy, cx, cy;  trace (iterations, 19) or NULL;  active, reserved: read by the batched entry only.
 *
 * state, 90 floats: [0,9) curr_r row-major, [9,12) curr_t, [12,57) curr_theta, [57,73) search size, [73,89) previous search size, [89]
 * previous success (0 / 1).  Candidate q:
 *     s = pre[q] * search;  quat = [sqrt(1 - s0^2 - s1^2 - s2^2), s0, s1, s2]  (NaN for a negative argument, as the reference)
 *     root rotation = curr_r @ quat2mat(quat) (used as a matrix, not through axis-angle);  translation = curr_t + s[3:6];
 *     joint angles = curr_theta + (s[6:16] @ comps[:10]) * theta_scale;  Rodrigues, kinematic chain, skinning (fp32)
 *     per vertex: object frame and nearest voxel exactly as pn2s_nearest;  penetration = max |sdf| [sdf < 0];  per finger min of
 *       sdf [sdf > 0] over its tip region;  silhouette pixel (row, col) = trunc(y/z*fy+cy, x/z*fx+cx) clamped to the mask, count / v
 *     keypoints: visible / invisible mean distance to pred_kp under vis_mask with clamp(count, 1) denominators, mean distance
 *       to last_kp, or no temporal term when last_kp is NULL
 *     energy = sil w_sil + pen w_pen + vis w_vis + invis w_invis + temporal w_temporal + attraction w_attr, added in that order;
 *       penetration, attraction and their products with the weights are rounded to the volume's type; the attraction term
 *       counts for every candidate only if candidate 0 penetrates.
 * A MANO setup runs, before every evaluation, hand_pose_offsets_kernel (every candidate's 135 features by the evaluation's own
 * angle and Rodrigues functions, times posedirs on v_mfma_f32_16x16x4_f32, into `offsets`) and then hand_pose_mano_eval_kernel
 * (the evaluation above with the offset added to every staged v_rest - j_k, fingertip keypoints from vertices, the centring;
 * the terms, their order and rounding as in the plain kernel).  offsets: pn2x_hand_pose_mano_work_floats(p, v) = p *
 * ceil16(3 v) floats of scratch, 16-byte aligned, required exactly when posedirs is set.
 *
 * pn2x_hand_pose_energy: one evaluation at frame->state -> energy (p); out_verts (p,v,3) / out_kp (p,21,3) or NULL: the
 * candidates' vertices and keypoints as the optimiser's device function computes them (tests, diagnostics).
 * pn2x_hand_pose_opt: `iterations` x (evaluate, update).  Update (:349-386, host branches as selects):
 *     w = (E[0] - E) [E < E[0]];  success = any(E < E[0]);  mean_E = success ? sum w E / sum w : E[0];  mt = sum w [quat | s] / sum w;
 *     mt[:4] /= |mt[:4]|;  on success curr_r = gram_schmidt_rows(curr_r @ quat2mat(mt[:4])), curr_t += mt[4:7],
 *     curr_theta += (mt[7:] @ comps[:10]) * theta_scale;  sz = |success ? mt[1:] : 0| + 1e-3;
 *     search = mean_E * scaling_coefficient2 * sz / ||sz|| + 1e-3;  if (previous success && success) search = beta search +
 *     (1 - beta) previous search;  if (success) previous search = search;  previous success = success.
 *   trace row per iteration: [E[0], mean_E, success, search after the update].
 * For both, `frame` is one record in HOST memory, read during the call.
 * pn2x_hand_pose_opt_batch: pn2x_hand_pose_opt for s independent problems (hand sequences that advance one frame together) with
 * one set of launches: per iteration hand_pose_eval_batch_kernel over a (candidates, problem) grid and
 * hand_pose_update_batch_kernel with a workgroup per problem.  They run pn2x_hand_pose_opt's device functions, so a problem's
 * state and trace equal, bit for bit, what pn2x_hand_pose_opt gives for it alone.  `problems` is a DEVICE array of s records;
 * a record with active == 0 sits out -- no pointer of it is read (all may be NULL) and nothing of it is written.  `active`
 * (the argument) is the number of active records.  A setup with posedirs set is PN2_EINVAL here: it goes to
 * pn2x_hand_pose_mano_opt_batch.
 * pn2x_hand_pose_mano_opt_batch: the same for a MANO setup (posedirs set; a setup without is PN2_EINVAL, the mirror of the plain
 * entry's refusal).  Per iteration hand_pose_offsets_batch_kernel over a (groups of 64 candidates, tile strides, problem) grid,
 * hand_pose_mano_eval_batch_kernel over (candidates, problem) and the shared hand_pose_update_batch_kernel: the device functions
 * of the single MANO kernels, so a problem's state and trace equal, bit for bit, what pn2x_hand_pose_opt gives for it alone.
 * `problems` and pn2x_hand_pose_problems_fill are used as they are (a record's work stays pn2x_hand_pose_opt_work_floats(p)
 * floats).  offsets: ONE device allocation of pn2x_hand_pose_mano_batch_work_floats(p, v, s) = s * p * ceil16(3 v) floats,
 * 16-byte aligned; problem q uses slice q (a slice is a multiple of 16 floats, so the alignment carries over), and the slice of
 * a record that sits out is neither read nor written.  The pre-pass grid's y is 3 * compute units / (groups * active) clamped
 * to [1, ceil(tiles / 4)] (active = 1 for the single entries).  NULL offsets is PN2_ENULL, misaligned PN2_EINVAL; with
 * iterations == 0 or active == 0 neither the table nor offsets is looked at.
 * Every evaluation grid deals a problem's ceil(p / 4) workgroups evenly over at most max(1, 3 * compute units / active)
 * (active = 1 for the single entries), so the launch covers the device about three times.
 * pn2x_hand_pose_problems_fill writes s records from HOST memory `host` into the device array by kernel launches that carry
 * them as arguments (16 records per launch): no copy engine, no pinned memory, and a captured graph holds the records.  It
 * checks the active records as the single entries check their frame.
 * pn2x_hand_pose_opt_batch_work_floats(p, s) = s * pn2x_hand_pose_opt_work_floats(p): scratch for s problems (slice q for
 * problem q).
 *
 * Sums run in a fixed order (xor butterflies inside a wave, waves in index order), no atomics, no waits between workgroups:
 * two runs give bitwise-equal results.  No host sync or allocation (capturable).  Limits (pn2x_hand_pose_opt_supported): 1 <= p <=
 * 8192, 1 <= v <= 1024, j == 21, 1 <= k <= 4, d_pose == 10 pose components, res odd and <= 1024.  Errors, checked before any
 * device work, PN2_EINVAL before PN2_ERANGE before PN2_ENULL: PN2_EINVAL for a size < 1 (p, v, j, k, res, h, w, s), an even res,
 * voxel_scale <= 0, vol_f16 or centre_root not 0 / 1, a misaligned posedirs / offsets, iterations < 0 or active outside [0, s];
 * PN2_ERANGE beyond the limits, for h * w >= 2^31, iterations > 4096 or s > 65535; PN2_ENULL for a NULL record or a NULL
 * pointer other than last_kp, trace, out_verts, out_kp (and posedirs).  A host record pointer below 64 KiB is PN2_EINVAL and is not
 * read: it is what a caller built against ABI version 3 passes (its first argument was p), and no process owns such an address.  iterations == 0 returns PN2_OK and touches nothing --
 * the frame record or the table may then be NULL, a bad setup is still refused -- and so does active == 0 with a table.
 */
typedef struct pn2x_hand_pose_setup {
    const int *parents, *pose_block, *skin_pack;
    const float *skin_w, *comps, *pre, *posedirs, *pose_mean;
    const int *kp_vertex;
    int p, v, j, k, vol_f16, res, centre_root, reserved;
    float theta_scale, voxel_scale, w_sil, w_pen, w_vis, w_invis, w_temporal, w_attr;
} pn2x_hand_pose_setup; /* 136 bytes */
typedef struct pn2x_hand_pose_problem {
    float *state, *work;
    const float *rest_joints, *rest_verts, *pred_kp, *last_kp;
    const unsigned char *vis_mask;
    const float *obj_r, *obj_t;
    const void *vol;
    const unsigned char *mask;
    float *trace;
    int h, w;
    float fx, fy, cx, cy;
    int active, reserved;
} pn2x_hand_pose_problem; /* 128 bytes */
int pn2x_hand_pose_opt_supported(int p, int v, int j, int k, int d_pose, int res);
long pn2x_hand_pose_opt_work_floats(int p);
long pn2x_hand_pose_mano_work_floats(int p, int v);
long pn2x_hand_pose_opt_batch_work_floats(int p, int s);
int pn2x_hand_pose_energy(const pn2x_hand_pose_setup *setup, const pn2x_hand_pose_problem *frame, float *offsets, float *energy,
                          float *out_verts, float *out_kp, void *stream);
int pn2x_hand_pose_opt(const pn2x_hand_pose_setup *setup, const pn2x_hand_pose_problem *frame, float *offsets, int iterations,
                       double scaling_coefficient2, double beta, void *stream);
int pn2x_hand_pose_problems_fill(pn2x_hand_pose_problem *problems, int s, const pn2x_hand_pose_problem *host, void *stream);
int pn2x_hand_pose_opt_batch(const pn2x_hand_pose_setup *setup, int s, int active, const pn2x_hand_pose_problem *problems,
                             int iterations, double scaling_coefficient2, double beta, void *stream);
long pn2x_hand_pose_mano_batch_work_floats(int p, int v, int s);
int pn2x_hand_pose_mano_opt_batch(const pn2x_hand_pose_setup *setup, int s, int active, const pn2x_hand_pose_problem *problems,
                                  float *offsets, int iterations, double scaling_coefficient2, double beta, void *stream);

/*
 * IKNet forward in eval mode (reference hand_network.py:264-322; hotrack_amd/csrc/iknet.hip) for m <= 16 rows, fp32:
 *     kp_hf = R^T (kp - t) / 0.2  (frame 0, 'kp')   or   kp * 5  (frame 1, 'camera'; R and t are not read)
 *     x     = [kp_hf | kp_hf - kp_hf[parent]]  coordinate-major (m, 126)
 *     h     = relu(x W1^T + b1), then five times h = relu(h Wl^T + bl)      (BatchNorm folded into W / b by the caller)
 *     raw_quat = h Wo^T + bo  (m, 60);  theta (m, 45) = per joint the axis-angle of raw_quat's quaternion [w, x, y, z]:
 *                q / (|q| + 1e-8), sin = sqrt(max(1 - w^2, 0)), axis = xyz / max(sin, [sin < 1e-8]), angle = 2 acos(clamp(w))
 * kp (m, 21, 3); R (m, 3, 3); t (m, 3, 1); w1 (1024, 128) with columns 126, 127 zero; b1 (1024); wh (5, 1024, 1024); bh (5, 1024);
 * wo (60, 1024); bo (60); work: pn2x_iknet_work_floats() floats; kp_hf (m, 3, 21) or NULL; raw_quat (m, 60); theta (m, 45).
 * w1, wh, wo and work 16-byte aligned.  Seven launches (one per layer), fixed summation order, no atomics: results are bitwise
 * reproducible.  No host sync or allocation (capturable).  Errors, checked before any device work: PN2_EINVAL for m < 1, a
 * frame other than 0 / 1 or a misaligned pointer; PN2_ERANGE for m > 16; PN2_ENULL for a NULL pointer (R, t: frame 0 only;
 * kp_hf may be NULL).  pn2x_iknet_supported(m, k_in, hidden, layers, n_out): the sizes this entry covers (1..16, 126, 1024, 6,
 * 60).
 */
int pn2x_iknet_supported(int m, int k_in, int hidden, int layers, int n_out);
long pn2x_iknet_work_floats(void);
int pn2x_iknet_forward(int m, int frame, const float *kp, const float *R, const float *t, const float *w1, const float *b1,
                       const float *wh, const float *bh, const float *wo, const float *bo, float *work, float *kp_hf,
                       float *raw_quat, float *theta, void *stream);

/*
 * ---- training-mode building blocks on point-major activations (hotrack_amd/csrc/train_ops.hip) --------------------------
 * The reference trains every grouped MLP as Conv2d(1x1) + BatchNorm2d + ReLU on channel-major (B, C, S, K) tensors
 * (pointnet_utils.py:399-403, :460-462, :504-506, :577-581).  A 1x1 convolution is a GEMM over all R = B*S*K positions
 * (library GEMM on point-major rows); what sits between two GEMMs is one pair of streaming kernels per direction.
 * Rows are `c` floats wide (c % 4 == 0, c <= 1024) with a row stride `ld*` (multiple of 4), 16-byte aligned.
 *
 * pn2x_bn_stats: per-channel sum_r y[r,:] and sum_r y[r,:]^2 into `sums` -- pn2x_bn_sums_doubles(c) fp64 accumulators zeroed by
 * the caller (several interleaved copies of the 2c sums: workgroups spread their atomics over the copies).
 */
int pn2x_bn_sums_doubles(int c);
int pn2x_bn_stats(long rows, int c, const float *y, int ldy, double *sums, void *stream);
/*
 * pn2x_bn_relu_apply: batch statistics from `sums` (biased variance, eps inside the sqrt -- torch.nn.BatchNorm semantics),
 * h = relu?(gamma * (y - mean) * invstd + beta); writes save_mean / save_invstd (c floats each, for the backward) and,
 * when running_mean != NULL, the running-statistics update running = (1 - momentum) running + momentum batch (variance
 * unbiased) and num_batches_tracked += 1.  conv_bias (or NULL) is the bias of the preceding convolution: it cancels in
 * the normalisation, so y is computed without it and it is only added to the running mean.
 */
int pn2x_bn_relu_apply(long rows, int c, const float *y, int ldy, const double *sums, const float *gamma, const float *beta,
                       const float *conv_bias, float eps, float momentum, float *running_mean, float *running_var,
                       long long *num_batches_tracked, float *save_mean, float *save_invstd, float *h, int ldh, int relu,
                       void *stream);
/*
 * pn2x_bn_relu_bwd: with g = dh * [h > 0] (h recomputed from y), xhat = (y - mean) * invstd:
 *   dbeta = sum_r g, dgamma = sum_r g * xhat, dy = gamma * invstd * (g - dbeta / R - xhat * dgamma / R).
 * sums: pn2x_bn_sums_doubles(c) fp64 accumulators zeroed by the caller (two launches: reduce, apply).  dbias (or NULL): gradient of the bias of
 * the convolution in front of the BatchNorm -- sum_r dy, identically zero -- written as zeros.
 */
int pn2x_bn_relu_bwd(long rows, int c, const float *dh, int ldd, const float *y, int ldy, const float *mean,
                     const float *invstd, const float *gamma, const float *beta, int relu, double *sums, float *dy, int ldo,
                     float *dgamma, float *dbeta, float *dbias, void *stream);
/*
 * Layer 1 of a set-abstraction scale in TRAINING mode, pre-activation, without materialising the grouped input
 * [feat_j | xyz_j - c_s | centre_feat_s] (reference pointnet_utils.py:389-399, :566-577): the same linear split as
 * pn2x_sa_mlp_max (a1f / wx / cadd, each optional, see above), bias omitted because BatchNorm follows.
 *   out (b, s*k, c1) point-major; rel_out (b, s*k, 3) or NULL receives xyz_j - c_s (the backward's d(wx) operand).
 * The (c1, 3) weight block wx is read in place from a wider matrix: rows wx_ld >= 3 floats apart (a column block of the
 * layer's [feature | xyz | centre] weight; no contiguous copy per step).
 */
int pn2x_sa_layer1(int b, int n, int s, int k, int c1, const float *a1f, int a1f_ld, const float *xyz, const float *cxyz,
                   const float *wx, int wx_ld, const float *cadd, int cadd_ld, const int *idx, float *out, float *rel_out,
                   void *stream);
/* The same for `count` (1 or 2) scales of one module (pointnet_utils.py:566-581: same clouds, coordinates and centres; per scale
 * its neighbour list, weight block, per-point / per-centre terms, output and relative coordinates), also accumulating the
 * BatchNorm statistics of every `out` into its `sums` (pn2x_bn_sums_doubles(c1) doubles, zeroed by the caller, as pn2x_bn_stats
 * would): the layer that follows is a train-mode BatchNorm (pointnet_utils.py:399-401), and its separate statistics pass over
 * the (b s k, c1) tensor is saved.  Two scales share ONE launch where both can take their statistics in it (alone, the K = 16
 * scale is a 12 us launch for a quarter of the K = 64 scale's rows); a scale that cannot runs pn2x_sa_layer1 + pn2x_bn_stats. */
typedef struct pn2x_sa_layer1_stats_problem {
    const float *a1f, *wx, *cadd;
    const int *idx;
    float *out, *rel_out;
    double *sums;
    int k, c1, a1f_ld, wx_ld, cadd_ld, reserved;
} pn2x_sa_layer1_stats_problem; /* 80 bytes */
int pn2x_sa_layer1_stats(const pn2x_sa_layer1_stats_problem *problems, int count, int b, int n, int s, const float *xyz,
                         const float *cxyz, void *stream);
/*
 * Transpose of pn2x_gather_rows (group_points_grad on point-major rows, reference group_points_gpu.cu:8-25):
 *   din[b, idx[b,j], :] += dout[b, j, :]      dout (b, m, ldo), idx (b, m) int32, din (b, n, ldi) accumulated into.
 */
int pn2x_scatter_add_rows(int b, int n, int m, int c, const float *dout, int ldo, const int *idx, float *din, int ldi,
                          void *stream);
/*
 * Transpose of pn2x_three_interpolate_pm (three_interpolate_grad on rows, reference interpolate_gpu.cu:192-214):
 *   dpoints[b, idx[b,j,t], :] += weight[b,j,t] * dout[b, j, :]   dout (b, n, ldo), dpoints (b, m, ldp) accumulated into.
 */
int pn2x_three_interpolate_pm_grad(int b, int c, int m, int n, const float *dout, int ldo, const int *idx,
                                   const float *weight, float *dpoints, int ldp, void *stream);

/*
 * Atomics-free form of the two row scatters above: invert the index list of every cloud once --
 *   pn2x_inverse_index: idx (b, l) with values in [0, n_dst)  ->  offsets (b, n_dst + 1), order (b, l): entries
 *   order[offsets[i] .. offsets[i+1]) are the positions e of idx with idx[e] == i   (n_dst <= 16127) --
 * then every target row SUMS its contributions (pn2x_rows_segment_sum):
 *   t == 1:  din[b, i, :] (+)= sum_{e in list(i)} dout[b, e, :]                      (transpose of pn2x_gather_rows)
 *   t == 3:  din[b, i, :] (+)= sum_{e in list(i)} weight[b, e] * dout[b, e / 3, :]   (transpose of pn2x_three_interpolate_pm;
 *            idx / weight are the (b, m_src, 3) tensors flattened)
 * accumulate == 0 overwrites (nothing to pre-zero), != 0 adds to din.  The order inside a list is unspecified.
 */
int pn2x_inverse_index(int b, int n_dst, int l, const int *idx, int *offsets, int *order, void *stream);
/* `count` (1 or 2) index lists over the same destination rows (the two neighbourhood sizes of a module scatter into two column
 * blocks of one gradient).  Two t == 1 problems share one launch where both take the one-thread-per-(destination, quad) kernel;
 * one launch per problem otherwise.  Same results either way. */
typedef struct pn2x_rows_segment_sum_problem {
    const float *dout;
    const int *offsets, *order;
    const float *weight;
    float *din;
    int m_src, t, c, ldo, ldi, reserved;
} pn2x_rows_segment_sum_problem; /* 64 bytes */
int pn2x_rows_segment_sum(const pn2x_rows_segment_sum_problem *problems, int count, int b, int n_dst, int accumulate, void *stream);

/*
 * Backward of group_points / gather_points (t = 1) and three_interpolate (t = 3) on the reference's channel-major layout with
 * CALLER-provided scratch (pn2x_scatter_cm_scratch_ints int32 elements): same results as pn2_group_points_grad /
 * pn2_gather_points_grad / pn2_three_interpolate_grad (accumulates into grad_points), but nothing is allocated inside, so
 * the call can be captured into a HIP graph.  (The reference-signature entries use a library-owned per-stream scratch and
 * fall back to their LDS-atomic kernels when that scratch would have to grow during a capture.)
 *   grad_out (b, c, m_src); idx (b, m_src) [t = 1] or (b, m_src, 3) with weight (b, m_src, 3) [t = 3]; grad_points (b, c, n_dst).
 * PN2_ERANGE: shape not covered (n_dst > 16127 or lists longer than 64 KiB of LDS) -- use the pn2_* entry.
 */
long pn2x_scatter_cm_scratch_ints(int t, int b, int n_dst, int m_src);
int pn2x_scatter_cm(int t, int b, int c, int n_dst, int m_src, const float *grad_out, const int *idx, const float *weight,
                    float *grad_points, int *scratch, long scratch_ints, void *stream);

/*
 * relu(BatchNorm_train(y)) followed by the max over the k rows of every group (the neighbourhood reduction that ends a
 * set-abstraction scale, reference pointnet_utils.py:403,581), without writing the (groups*k, c) activations:
 *   out (groups, c) = max_k relu(bn(y[g*k + kk, :]));  arg (groups, c) int32 = the first arg-max row kk.
 * Statistics / running-statistics semantics as pn2x_bn_relu_apply (sums from pn2x_bn_stats over all groups*k rows).
 * pn2x_bn_relu_max_bwd: backward through max + ReLU + BatchNorm given dout (groups, c): only the arg-max row of a group
 * receives dout (times the ReLU mask); dy (groups*k, ldo), dgamma, dbeta, dbias as pn2x_bn_relu_bwd.
 */
/* `count` (1 or 2) problems.  The output rows are ldo floats apart: `out` may be a column block of a wider buffer (the scales of
 * a multi-scale module, reference pointnet_utils.py:405-409 / :583-590 `torch.cat(new_points_list, dim=1)`, write the halves of
 * one tensor).  Two problems (the two neighbourhood sizes of a module) share ONE launch where both take the few-groups kernel. */
typedef struct pn2x_bn_relu_max_problem {
    const float *y;
    const double *sums;
    const float *gamma, *beta, *conv_bias;
    float *running_mean, *running_var;
    long long *num_batches_tracked;
    float *save_mean, *save_invstd, *out;
    int *arg;
    long groups;
    int k, c, ldy, ldo;
    float eps, momentum;
} pn2x_bn_relu_max_problem; /* 128 bytes */
int pn2x_bn_relu_max(const pn2x_bn_relu_max_problem *problems, int count, void *stream);
int pn2x_bn_relu_max_bwd(long groups, int k, int c, const float *dout, const int *arg, const float *y, int ldy, const float *mean,
                         const float *invstd, const float *gamma, const float *beta, double *sums, float *dy, int ldo, float *dgamma,
                         float *dbeta, float *dbias, void *stream);

/*
 * The two launches of pn2x_bn_relu_bwd / pn2x_bn_relu_max_bwd as separate entries (used by the fused training stacks below).
 * pn2x_bn_bwd_reduce: sums += [sum_r g, sum_r g xhat] with g = dh . [relu(bn(y)) > 0] (relu != 0) -- or, with arg != NULL,
 *   dh = d(max over k consecutive rows) (rows / k x c, row stride ldd, arg (rows / k, c) with the same row stride c) routed
 *   to the recorded arg-max row and ReLU-masked; for this max-routed form the routed + masked gradient itself is also written
 *   densely to g_out (rows x c, row stride ldg) unless g_out is NULL: the fused GEMMs of the layer below then read a plain
 *   gradient instead of routing it on every load.
 * pn2x_bn_bwd_apply: dy = gamma invstd (g' - sum(g)/R - xhat sum(g xhat)/R) with g' = g . mask when relu != 0, g as given
 *   (already masked) when relu == 0; also writes dgamma, dbeta (and zeros to dbias) from the sums.
 */
int pn2x_bn_bwd_reduce(long rows, int c, const float *dh, int ldd, const int *arg, int k, const float *y, int ldy, const float *mean,
                       const float *invstd, const float *gamma, const float *beta, int relu, double *sums, float *g_out, int ldg,
                       void *stream);
/* The same sums for a max-routed top layer from its arg-max rows only (groups x c gathered reads of y instead of rows x c):
 * dout (groups x c, row stride ldd: may be a column block of a wider gradient), arg (groups x c, row stride lda), y ((groups * k) x c).  The layer below then routes on load (pn2x_tg_bwd_slice, gmode 2). */
/* `count` (1 or 2) problems; two whose channel counts fill the same number of 64-channel tiles share one launch. */
typedef struct pn2x_bn_bwd_reduce_routed_problem {
    const float *dout;
    const int *arg;
    const float *y, *mean, *invstd, *gamma, *beta;
    double *sums;
    long groups;
    int k, c, ldd, lda, ldy, reserved;
} pn2x_bn_bwd_reduce_routed_problem; /* 96 bytes */
int pn2x_bn_bwd_reduce_routed(const pn2x_bn_bwd_reduce_routed_problem *problems, int count, void *stream);
/* out (c x 3) = dy^T rel: dy (rows x c, row stride ldy), rel (rows x 3) -- the gradient of the three xyz columns of a grouped
 * layer-1 weight.  c / 4 must divide 256; scratch of pn2x_rows_outer3_scratch_floats(rows, c) floats (per-workgroup partials). */
long pn2x_rows_outer3_scratch_floats(long rows, int c);
int pn2x_rows_outer3(long rows, int c, const float *dy, int ldy, const float *rel, float *out, float *scratch, long scratch_floats,
                     void *stream);
int pn2x_bn_bwd_apply(long rows, int c, const float *g, int ldg, const float *y, int ldy, const float *mean, const float *invstd,
                      const float *gamma, const float *beta, int relu, const double *sums, float *dy, int ldo, float *dgamma,
                      float *dbeta, float *dbias, void *stream);

/* pn2x_bn_bwd_apply for the first layer of a set-abstraction scale, also forming dwx (c x 3) = dy^T rel from the dy it has in
 * registers (rel (rows x 3): the relative coordinates pn2x_sa_layer1 wrote) -- the separate pn2x_rows_outer3 pass disappears.
 * c <= 256; scratch: pn2x_bn_bwd_apply_rel_scratch_floats(rows, c) floats. */
long pn2x_bn_bwd_apply_rel_scratch_floats(long rows, int c);
/* `count` (1 or 2) problems; two (the two neighbourhood sizes of a module) run in one launch each of the two kernels. */
typedef struct pn2x_bn_bwd_apply_rel_problem {
    const float *g, *y, *mean, *invstd, *gamma, *beta;
    const double *sums;
    float *dy, *dgamma, *dbeta, *dbias;
    const float *rel;
    float *scratch, *dwx;
    long rows, scratch_floats;
    int c, ldg, ldy, relu, ldo, reserved;
} pn2x_bn_bwd_apply_rel_problem; /* 152 bytes */
int pn2x_bn_bwd_apply_rel(const pn2x_bn_bwd_apply_rel_problem *problems, int count, void *stream);

/*
 * Train-mode [Conv 1x1 + BatchNorm + ReLU] layers with the BatchNorm folded into fp32-MFMA GEMMs (csrc/train_gemm.hip;
 * reference composition: pointnet_utils.py:399-403, :460-462, :504-506, :577-581 as Conv2d/Conv1d + BatchNorm + ReLU modules).
 * Layer i >= 2 of a stack, point-major rows; `p` = layer i-1, `i` = layer i; sums_* = pn2x_bn_sums_doubles(c) fp64
 * accumulators (forward: [sum y | sum y^2], backward: [sum g | sum g xhat]) zeroed by the caller.
 *
 * pn2x_tg_fwd    y_i (rows x n) = relu(BN_p(x)) w^T with x = y_p (rows x k) and w (n x k); BN_p's batch statistics come from
 *                sums_in (filled by the producer of x); workgroup 0 writes save_mean / save_invstd of layer p and its
 *                running-statistics update (semantics of pn2x_bn_relu_apply); sums_out (or NULL) receives the statistics of y_i.
 * pn2x_tg_dgrad  g_p (rows x n) = (dY_i w) . [relu(BN_p(y_p)) > 0] and sums_bwd_p, where dY_i (rows x kd) =
 *                gamma_i invstd_i (g - sum(g)/R - xhat_i sum(g xhat_i)/R) is computed on load from
 *                  gmode 0: g = the stored, already masked g_i (rows x kd, row stride ldg);
 *                  gmode 1: g = dh_i . [relu(BN_i(y_i)) > 0] with dh_i stored (rows x kd);
 *                  gmode 2: dh = d(max over kmax consecutive rows) (rows / kmax x kd, row stride ldg; arg likewise) routed to
 *                           the arg-max row and masked;
 *                and sums_bwd_i (complete: from pn2x_bn_bwd_reduce for the top layer, from the dgrad of layer i+1 otherwise).
 * pn2x_tg_wgrad  dw (n x k) = dY_i^T relu(BN_p(y_p)) (both operands computed on load), reduced over row splits through
 *                `partial` (>= pn2x_tg_wgrad_partial_floats(rows, n, k) floats); also dgamma_i, dbeta_i (and zeros to dbias_i).
 *                n_partials != NULL: the reduction is deferred -- only the partial tiles are written (dw zeroed) and their
 *                count returned in *n_partials; pn2x_tg_reduce_multi then sums the partial tiles of SEVERAL layers in one
 *                launch (the weight gradients are not needed before the optimiser step).
 * pn2x_tg_supported(c_in, c_out): c_in % 4 == 0, c_in <= 512, c_out a multiple of 32 (for wgrad also c_in % 32 == 0).
 */
int pn2x_tg_supported(int c_in, int c_out);
int pn2x_tg_fwd(long rows, int k, int n, const float *x, int ldx, const float *w, int ldw, float *y, int ldy, const double *sums_in,
                const float *gamma, const float *beta, const float *conv_bias, float eps, float momentum, float *running_mean,
                float *running_var, long long *num_batches_tracked, float *save_mean, float *save_invstd, double *sums_out,
                void *stream);
int pn2x_tg_dgrad(long rows, int kd, int n, int gmode, const float *g, int ldg, const int *arg, int kmax, const float *yi, int ldyi,
                  const float *mean_i, const float *invstd_i, const float *gamma_i, const float *beta_i, const double *sums_bwd_i,
                  const float *w, int ldw, const float *yp, int ldyp, const float *mean_p, const float *invstd_p,
                  const float *gamma_p, const float *beta_p, float *gp, int ldgp, double *sums_bwd_p, void *stream);
long pn2x_tg_wgrad_partial_floats(long rows, int n, int k);
int pn2x_tg_wgrad(long rows, int n, int k, int gmode, const float *g, int ldg, const int *arg, int kmax, const float *yi, int ldyi,
                  const float *mean_i, const float *invstd_i, const float *gamma_i, const float *beta_i, const double *sums_bwd_i,
                  const float *yp, int ldyp, const float *mean_p, const float *invstd_p, const float *gamma_p, const float *beta_p,
                  float *partial, long partial_floats, float *dw, float *dgamma, float *dbeta, float *dbias, int *n_partials,
                  void *stream);

/*
 * The loss / metric dictionary of HandTrackNet.compute_loss (reference hand_network.py:159-221, training mode without MANO
 * terms) in one launch, and its gradient with respect to the predicted hand-frame keypoints in another (csrc/kabsch.hip).
 * pred_hf / init_hf (b,3,21) channel-major hand-frame keypoints, gt_kp / pred_kp (b,21,3) camera frame, R (b,3,3) / t (b,3) /
 * scale: the canonical pose, palm (pb,6,3) with pb in {1,b}: the palm template.  out[9] =
 *   {hand_pred_kp_loss, hand_pred_r_loss, hand_pred_t_loss, hand_pred_kp_diff, hand_init_kp_diff, hand_init_r_diff,
 *    hand_init_t_diff, hand_pred_r_diff, hand_pred_t_diff};  saved (b, 87) floats for the backward.  weights (9, or NULL): the
 * caller's weighted total folded in -- out then has ten entries, out[9] = sum_i weights[i] out[i].
 * backward: d_pred_hf (b,3,21) = d(grad3[0] out[0] + grad3[1] out[1] + grad3[2] out[2] + grad_total[0] out[9]) / d pred_hf;
 * grad3 (3) and grad_total (1) on the device, either may be NULL (not both); weights as given to the forward.
 */
int pn2x_hand_losses(int b, int pb, const float *pred_hf, const float *init_hf, const float *gt_kp, const float *pred_kp, const float *R,
                     const float *t, float scale, const float *palm, float *out, float *saved, const float *weights, void *stream);
int pn2x_hand_losses_backward(int b, int pb, const float *pred_hf, float scale, const float *palm, const float *saved, const float *grad3,
                              const float *grad_total, const float *weights, float *d_pred_hf, void *stream);

/*
 * The 21-token tail in TRAINING mode (csrc/tail_train.hip; reference transformer.py:65-67, hand_network.py:139-147 with
 * attn=False): every element-wise run between two GEMMs as one launch per direction.  Rows are tokens (rows x c, contiguous).
 *   pn2x_tail_ln_fwd   u = x + dropout(y + bias) (y, bias optional), out = LN_b(LN_a(u)) (LN_b optional: gb = bb = NULL);
 *                      stats (rows, 4) = mean_a, rstd_a, mean_b, rstd_b for the backward.  seed_dev != NULL: this launch
 *                      advances the device seed counter and writes the new value to seed_out (it must have no dropout itself);
 *                      otherwise seed_in is the per-forward seed the dropout mask is hashed from (site: which dropout).
 *   pn2x_tail_ln_bwd   dx (= du), dy (if y), and -- ATOMICALLY ADDED onto zero-initialised c-float buffers -- dga, dba, dgb,
 *                      dbb, dbias.  c <= 512.
 *   pn2x_tail_relu_drop_fwd / _bwd   h = dropout(relu(z + bias)); dz, dbias (atomically added).  c % 4 == 0.
 * Dropout: kept elements scaled by 1 / (1 - p); the mask is regenerated in the backward from (seed, site, index).
 */
int pn2x_tail_ln_fwd(long rows, int c, const float *x, const float *y, const float *bias, float p, int site, const long long *seed_in,
                     long long *seed_dev, long long *seed_out, const float *ga, const float *ba, float eps_a, const float *gb,
                     const float *bb, float eps_b, float *out, float *stats, void *stream);
int pn2x_tail_ln_bwd(long rows, int c, const float *x, const float *y, const float *bias, float p, int site, const long long *seed_in,
                     const float *ga, const float *ba, float eps_a, const float *gb, const float *bb, float eps_b, const float *stats,
                     const float *dout, float *dx, float *dy, float *dga, float *dba, float *dgb, float *dbb, float *dbias,
                     void *stream);
int pn2x_tail_relu_drop_fwd(long rows, int c, const float *z, const float *bias, float p, int site, const long long *seed_in,
                            float *out, void *stream);
int pn2x_tail_relu_drop_bwd(long rows, int c, const float *z, const float *bias, float p, int site, const long long *seed_in,
                            const float *dh, float *dz, float *dbias, void *stream);
/* The last layer of final_mlp + residual on the initial keypoints + de-canonicalisation, in training (hand_network.py:141-147):
 * h (b*j, c) rows, w (3, c), bias (3), xyz1 (b, 3, j), R (b, 3, 3), t (b, 3), scale (b; scale_stride 0: one value for all) ->
 * kp_hand (b, 3, j) = h w^T + bias + xyz1, kp_cam (b, j, 3) = scale R kp_hand + t.  Backward: g_hand (b, 3, j) and / or g_cam (b, j, 3)
 * -> dh (b*j, c); dw (3, c) and dbias (3) are ADDED to (zero-filled accumulators). */
int pn2x_tail_pose_head_fwd(int b, int j, int c, const float *h, const float *w, const float *bias, const float *xyz1, const float *R,
                            const float *t, const float *scale, int scale_stride, float *kp_hand, float *kp_cam, void *stream);
int pn2x_tail_pose_head_bwd(int b, int j, int c, const float *h, const float *w, const float *g_hand, const float *g_cam, const float *R,
                            const float *scale, int scale_stride, float *dh, float *dw, float *dbias, void *stream);

/*
 * One Adam step over n fp32 tensors (csrc/adam.hip): torch.optim.Adam semantics (L2 weight decay added to the gradient, bias
 * corrections from the per-tensor `step` counters, no amsgrad -- reference trainer.py:49-52), the arithmetic of torch's fused
 * kernel.  p / g / m / v / step: HOST arrays of n device pointers (m = exp_avg, v = exp_avg_sq, step = one fp32 counter per
 * tensor); numel: host array of n element counts.  The tensor table travels in the kernel arguments.  advance != 0: this call
 * advances the counters; advance = 0: they are left alone (the caller keeps them in one contiguous buffer and advances them all
 * with pn2x_adam_advance AFTER every pn2x_adam_multi of the step: the update kernels read the old values).
 */
int pn2x_adam_multi(int n, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *step, const long *numel,
                    double lr, double beta1, double beta2, double eps, double weight_decay, int advance, void *stream);
int pn2x_adam_advance(float *steps, int n, void *stream);
/* The deferred reduction of pn2x_tg_wgrad (n_partials != NULL) for SEVERAL layers (host arrays of `count` entries): sums their
 * partial tiles and emits their dgamma / dbeta (/ zero dbias) in one launch.  Entries may be column slices of a wider layer:
 * sums_ld[j] = channels of the whole layer (sums_ld NULL: = channels[j]). */
int pn2x_tg_reduce_multi(int count, const float *const *partial, const int *n_partials, const int *numel, float *const *dw,
                         const double *const *sums_bwd, const int *channels, const int *sums_ld, float *const *dgamma,
                         float *const *dbeta, float *const *dbias, void *stream);
/* pn2x_tg_fwd with a different schedule for 64- / 128-channel inputs (csrc/train_fwd.hip: W_i resident in LDS, 64-row tiles whose
 * normalised operand is built once, one 32 x 32 output block per wave).  Same arguments (as a record) and results (up to
 * summation order), for `count` (1 or 2) problems: two must have the same k and n (else PN2_EINVAL) and share ONE launch where
 * pn2x_tg_fwd2_pair_supported(k, n) -- the two neighbourhood sizes of a keypoint-query module: same widths, different weights and
 * row counts (reference pointnet_utils.py:566-581 runs them as separate Conv2d stacks); the persistent workgroups are split in
 * proportion to the tile counts. */
typedef struct pn2x_tg_fwd2_problem {
    const float *x, *w;
    float *y;
    const double *sums_in;
    const float *gamma, *beta, *conv_bias;
    float *running_mean, *running_var;
    long long *num_batches_tracked;
    float *save_mean, *save_invstd;
    double *sums_out;
    long rows;
    int k, n, ldx, ldw, ldy;
    float eps, momentum;
    int reserved;
} pn2x_tg_fwd2_problem; /* 144 bytes */
int pn2x_tg_fwd2_supported(int c_in, int c_out);
int pn2x_tg_fwd2_pair_supported(int c_in, int c_out);
int pn2x_tg_fwd2(const pn2x_tg_fwd2_problem *problems, int count, void *stream);

/* The whole backward of fused layer i in one kernel (csrc/train_bwd.hip): g_{i-1} (gp, with the ReLU mask and the
 * BatchNorm-backward sums of layer i-1, as pn2x_tg_dgrad) AND the weight-gradient partial tiles (as pn2x_tg_wgrad with
 * n_partials) from one pass over g_i, Y_i and Y_{i-1}.  gmode 0: g pre-masked (rows x n); gmode 1: g dense, ReLU-masked from Y_i on load; gmode 2: g = d(max over kmax
 * rows) ((rows / kmax) x n) routed on load through arg (same shape / stride) and ReLU-masked from Y_i.  n = channels of layer i, k = channels of layer
 * i-1; w (n x k).  pn2x_tg_bwd_supported(k, n): k in {32, 64, 128} and the instantiated n; pn2x_tg_bwd_partials = the number
 * of (n x k) partial tiles written (partial_floats >= that * n * k), to be summed by pn2x_tg_reduce_multi.  dw is zeroed.
 * pn2x_tg_bwd_slice runs one column slice [c0, c0 + n) of a layer with sums_ld channels (all layer-i pointers offset to the slice by the
 * caller; a whole layer is the one slice c0 = 0, sums_ld = n, ldarg = ldg, g_add = NULL, raw_out = 0).  A wider layer runs as consecutive slices: raw_out = 1 leaves the unmasked partial data gradient in gp, the next slice
 * passes it as g_add (may alias gp) and the last one applies the mask and accumulates the sums.  gmode 1: dense g, masked from Y_i.
 * `count` (1 or 2) problems.  Two must have the same n, k and gmode (else PN2_EINVAL) and share ONE launch where
 * pn2x_tg_bwd_pair_supported(k, n) (the two neighbourhood sizes of a keypoint-query module), the persistent workgroups split in
 * proportion to the tile counts.  n_partials (`count` ints; may be NULL when count == 1) receives the number of weight-gradient
 * partial tiles each problem wrote: in a shared launch a problem gets a share of the grid, so fewer than pn2x_tg_bwd_partials
 * reports for it alone (which its partial buffer must hold all the same). */
typedef struct pn2x_tg_bwd_slice_problem {
    const float *g;
    const int *arg;
    const float *yi, *mean_i, *invstd_i, *gamma_i, *beta_i;
    const double *sums_bwd_i;
    const float *w, *yp, *mean_p, *invstd_p, *gamma_p, *beta_p;
    float *gp;
    double *sums_bwd_p;
    float *partial, *dw;
    const float *g_add;
    long rows, partial_floats;
    int n, k, gmode, ldg, ldarg, kmax, ldyi, sums_ld, ldw, ldyp, ldgp, ldga, raw_out, reserved;
} pn2x_tg_bwd_slice_problem; /* 224 bytes */
int pn2x_tg_bwd_pair_supported(int c_in, int c_out);
int pn2x_tg_bwd_slice(const pn2x_tg_bwd_slice_problem *problems, int count, int *n_partials, void *stream);
int pn2x_tg_bwd_supported(int c_in, int c_out);
int pn2x_tg_bwd_partials(long rows, int c_out, int c_in);
/* Round 5: for c_in in {64, 128} the kernel keeps W_i in registers as the B operand of v_mfma_f32_16x16x4_f32 (16-column slices
 * per wave; csrc/train_bwd.hip, tg_bwd2).  pn2x_tg_bwd_set_variant(0) selects the round-4 kernel (W_i streamed from L2 / LDS) for
 * every shape, 1 (default, or HOTRACK_TGB2) the new one where instantiated.  Process-wide: switch between whole backward passes
 * only (tests, A/B benches) -- the number of partial tiles a launch writes depends on it. */
int pn2x_tg_bwd_set_variant(int v2);

/* The weight gradients of `count` plain linear layers in one grouped launch (csrc/train_wgrad.hip):
 *   dw[p] (n[p] x k[p], row stride lddw[p]) = g[p]^T (rows[p] x n[p], row stride ldg[p]) . x[p] (rows[p] x k[p], row stride ldx[p])
 * -- what autograd computes as `grad_out.t() @ input` per torch.nn.functional.linear call (layer 1 of every stack over the
 * un-grouped points, the rearrange linears, the 21-token tail: reference pointnet_utils.py:399-403,460-462,504-506,577-581,
 * blocks.py:226-239, transformer.py:72-82).  Host arrays of `count` <= pn2x_wgrad_multi_max() entries; any n / k / strides
 * (16-byte loads where an operand allows them); dw[p] is overwritten (a column block of a wider weight when lddw[p] > k[p]).
 * Work is cut into (128 x 128 tile, row split) units of equal length over all problems; split problems go through `scratch`
 * (>= pn2x_wgrad_multi_scratch_floats floats, 16-byte aligned) and are summed in a fixed order by a second launch:
 * deterministic, no atomics.  PN2_ESCRATCH when the scratch is too small. */
int pn2x_wgrad_multi_max(void);
long pn2x_wgrad_multi_scratch_floats(int count, const int *rows, const int *n, const int *k);
int pn2x_wgrad_multi(int count, const float *const *g, const int *ldg, const float *const *x, const int *ldx, const int *rows,
                     const int *n, const int *k, float *const *dw, const int *lddw, float *scratch, long scratch_floats, void *stream);

/* y (m x n, row stride ldy) = act(x (m x k) . w^T (w: n x k) + bias (n | NULL)), relu != 0: ReLU -- a dense layer over FEW rows
 * (the B = 1 tracking loop: 21 ... 1024 rows; csrc/linear_small.hip): one workgroup per 32 x 32 output block, its four waves
 * splitting the reduction.  Same result as the BLAS library up to summation order. */
int pn2x_linear_small(int m, int k, int n, const float *x, int ldx, const float *w, int ldw, const float *bias, int relu, float *y,
                      int ldy, void *stream);

/* y (m x n) = act(LN2(LN1(xa + ya + ybias)) . w^T + bias): pn2x_add_layernorm followed by pn2x_linear_small as ONE launch for the
 * 21-token tail at small batch (reference transformer.py:65-67,72-82 with attn = False: norm -> linear1 -> ReLU -> linear2 ->
 * residual + norm; hand_network.py:139-141).  xa, ya (m x k, contiguous rows; ya / ybias may be NULL), LayerNorm 1 (g1, b1, eps1),
 * optional LayerNorm 2 (g2, b2, eps2; g2 NULL: none), k <= 384.  xout (m x k | NULL) receives the normalised rows (the next
 * residual's input).  The LayerNorm arithmetic is pn2x_add_layernorm's, the product pn2x_linear_small's: same bits as the pair. */
int pn2x_ln_linear_small(int m, int k, int n, const float *xa, const float *ya, const float *ybias, const float *g1, const float *b1,
                         float eps1, const float *g2, const float *b2, float eps2, float *xout, const float *w, int ldw,
                         const float *bias, int relu, float *y, int ldy, void *stream);

/*
 * Per-sequence evaluation of the object trackers (csrc/seq_eval.hip): all t frames of a sequence per call, no host sync.
 *
 * pn2x_posed_chamfer: the reference's compute_chamfer (track_network.py:91-94) on the two clouds after its per-frame
 * `matmul(cloud, R^T) + t` transforms (:431-433), for every frame at once.  a (n, 3) and b (m, 3) in their model frames;
 * ra, rb (t, 3, 3) row-major and ta, tb (t, 3) the per-frame poses;
 *   out[f] = mean_i min_j |(ra_f a_i + ta_f) - (rb_f b_j + tb_f)| + mean_j min_i |...|        (f < t; metres).
 * The un-posed chamfer is the same call with t = 1 and identity poses.  Squared distances in the difference form, one square
 * root per point; the (n x m) distance matrix is never stored.  partial: device scratch of at least
 * pn2x_posed_chamfer_partial_floats(n, m, t) floats (PN2_ESCRATCH when smaller; -1 for a negative size): the per-workgroup
 * sums, added in index order by a second launch -- no atomics, two calls give the same bits.  PN2_EINVAL for n, m or t < 0 and
 * for an empty cloud with t > 0; t = 0 is a no-op; PN2_ERANGE beyond 65535 tiles of 512 points (n + m > ~33 million).
 *
 * pn2x_obj_pose_metrics: eval_part_full's per-frame terms (pose_utils/part_dof_utils.py:54-78, metrics.py:6-143) for t pose
 * pairs: gt_r, pred_r (t, 3, 3), gt_t, pred_t (t, 3) -> out (t, 4) = {tdiff [m], rdiff [degrees], 5deg5cm, 10deg10cm}.
 * axis / up_and_down_sym select rot_diff_rad's branch: axis 0..2 the angle between those columns (|cos| when up_and_down_sym),
 * 3 the minimum over the identity and the three 180-degree flips, -1 over the identity and the xz flip, any other value the
 * geodesic angle.  Cosines clamped to [-1, 1], thresholds inclusive (<=), as in the reference.
 */
long pn2x_posed_chamfer_partial_floats(int n, int m, int t);
int pn2x_posed_chamfer(int n, int m, int t, const float *a, const float *b, const float *ra, const float *ta, const float *rb,
                       const float *tb, float *partial, long partial_floats, float *out, void *stream);
int pn2x_obj_pose_metrics(int t, const float *gt_r, const float *gt_t, const float *pred_r, const float *pred_t, int axis,
                          int up_and_down_sym, float *out, void *stream);

/*
 * Evaluation of tracked hand sequences (csrc/kabsch.hip): HandTrackNet.compute_loss's dictionary with track_flag set (reference
 * hand_network.py:159-221) for every frame of s sequences, and the reference's sequence rule (track_network.py:300-306), in two
 * launches without a host sync.  The f frames are those of all sequences packed one sequence after the other; seq_off (s + 1)
 * int32 on the device, non-decreasing, seq_off[0] = 0, seq_off[s] = f, gives each sequence's frames.  j: keypoints per hand (21).
 * pred_hf / init_hf (f,3,21) channel-major hand-frame keypoints, gt_kp / pred_kp (f,21,3) camera frame, rc (f,3,3) / tc (f,3) /
 * scale (f): each frame's hand frame.  rows (f,12) and seq (s,12), columns
 *   {hand_pred_kp_loss, hand_pred_kp_diff, hand_init_kp_diff, hand_pred_r_loss, hand_pred_t_loss, hand_init_r_diff,
 *    hand_init_t_diff, hand_pred_r_diff, hand_pred_t_diff, hand_canon_r_diff, hand_canon_t_diff, MANO_theta_diff}.
 * mode 0: (R, t) / (R_gt, t_gt) are the rigid fits of the sequence's palm template (palm (s,6,3)) onto the palm keypoints of the
 * scaled predicted / ground-truth keypoints; pose_r / pose_t are not read.  mode 1: (R, t) = (pose_r (f,3,3), pose_t (f,3)),
 * (R_gt, t_gt) = (gt_r, gt_t); columns 5 and 6 are not produced and palm is not read.  gt_r (f,3,3) / gt_t (f,3): the
 * ground-truth hand pose, optional in mode 0 (columns 9, 10); theta / theta_gt (f,45) optional (column 11).  A column that is not
 * produced is written as 0.  seq: columns 2, 5, 6 are the row of the sequence's first frame, every other column the mean of the
 * sequence's rows summed in frame order; a sequence without frames gets zeros.  Run-to-run bitwise equal, and a sequence's
 * values do not depend on the other sequences of the call.
 * Returns the mask of valid columns (bit c = column c; >= 0) or PN2_EINVAL (f < 0, s < 0, j != 21, mode not 0 / 1) / PN2_ENULL (a
 * required pointer is NULL with f > 0 and s > 0) / PN2_ELAUNCH.  f = 0 or s = 0: the mask, no launch.
 */
int pn2x_hand_seq_metrics(int f, int s, int j, int mode, const float *pred_hf, const float *init_hf, const float *gt_kp,
                          const float *pred_kp, const float *rc, const float *tc, const float *scale, const float *palm,
                          const int *seq_off, const float *pose_r, const float *pose_t, const float *gt_r, const float *gt_t,
                          const float *theta, const float *theta_gt, float *rows, float *seq, void *stream);

/*
 * Hand-object penetration and contact of tracked hand sequences (hotrack_amd/csrc/hand_interact.hip): the quantities the hand-pose
 * optimiser minimises (reference optimization_hand.py:264-293) for the hands the tracker ended up with, per frame and per sequence,
 * in two launches without a host sync.  The definitions are this project's (the reference has no such evaluation).  The f frames
 * are those of s sequences packed one sequence after the other; seq_off (s + 1) int32 on the device as for pn2x_hand_seq_metrics.
 * model: the pn2x_hand_pose_setup record (HOST memory, read during the call).  Read: parents, pose_block, skin_pack, skin_w,
 * posedirs, pose_mean, kp_vertex, v, j, k, vol_f16, res, centre_root, voxel_scale.  Not read: p, pre, comps, theta_scale, the
 * weights.  Per frame (DEVICE memory): global_r (f,3,3) the root rotation, used as a matrix as the optimiser uses it; global_t
 * (f,3); theta (f,45) the joint angles (a MANO setup adds pose_mean); obj_r (f,3,3), obj_t (f,3) the object pose; pred_kp (f,21,3)
 * or NULL; rest_of (f) int32: the shape table the frame is posed with, rest_joints (g,21,3) / rest_verts (g,v,3) being g tables of
 * rest + beta @ shape_* (a tracker that re-estimates the shape has several per sequence).  vols (s): a device array of the
 * sequences' volume pointers (res^3 fp16 / fp32, sequences may share one; the entry of a sequence without frames is not read).
 * hand_interact_rows_kernel, a workgroup per frame, poses the hand with HandModel.lbs_forward_from_tables' semantics (kinematic
 * chain over parents / pose_block, k <= 4 skinning weights; with posedirs set: pose_mean, the pose blend shapes -- 3 v x 135
 * multiply-adds on the vector ALUs, column order, no workspace --, kp_vertex fingertips and centre_root), takes every vertex
 * into the object frame and reads its voxel exactly as pn2s_nearest, the value as fp32, and reduces to rows (f,8):
 *   0  penetration depth [m]: max of -sdf over the vertices with sdf < 0, else 0
 *   1  share of vertices with sdf < 0: (float)count / (float)v
 *   2  1 if column 0 > 0, else 0
 *   3  number of fingers (0..5) in contact: min of sdf over the finger's tip region <= contact_threshold; the tip regions are
 *      bits 20..24 of skin_pack (fingers 0..4 of get_attraction_loss); an empty region is not in contact
 *   4  tip gap [m]: mean over the fingers with a non-empty tip region of max(min sdf over the region, 0), summed in finger
 *      order; 0 if no finger has one
 *   5  signed minimum of sdf over all vertices [m]
 *   6  mean over the 21 keypoints of |posed model keypoint - pred_kp[f]| [m]; 0 and not valid when pred_kp is NULL
 *   7  1 if column 3 > 0, else 0
 * hand_interact_reduce_kernel, a workgroup per sequence: seq (s,8) = the mean of the sequence's rows, added in frame order
 * (fp64); a sequence without frames gets zeros.  out_verts (f,v,3) / out_kp (f,21,3) or NULL: the posed vertices and keypoints
 * (tests, diagnostics).  No atomics, fixed summation order: run-to-run bitwise equal, and a sequence's values do not depend on
 * the other sequences of the call.  No host sync or allocation (capturable).
 * Returns the mask of valid columns (bit c = column c: 0xbf, or 0xff with pred_kp) or a negative code.  Limits as
 * pn2x_hand_pose_opt_supported for v, j, k, res.  Errors, checked before any device work, PN2_EINVAL before PN2_ERANGE before
 * PN2_ENULL: PN2_EINVAL for f < 0, s < 0, g < 0 (g < 1 with frames to evaluate), contact_threshold < 0 or NaN, a size of the
 * record < 1, an even res, voxel_scale <= 0, vol_f16 or centre_root not 0 / 1, a misaligned posedirs (16-byte loads), a record
 * pointer below 64 KiB (not read); PN2_ERANGE beyond the limits; PN2_ENULL for a NULL record, a NULL table of the record (with
 * posedirs set: pose_mean, kp_vertex) and, with f > 0 and s > 0, any NULL array but pred_kp, out_verts, out_kp.  f = 0 or s = 0:
 * the mask, no launch, the arrays are not looked at (a bad record is still refused).  rest_of and seq_off are device memory and
 * NOT checked: a rest_of outside [0, g) is clamped into it, offsets outside [0, f] are clamped and a non-monotone seq_off gives
 * that sequence zeros or the wrong frames' mean -- nothing outside the arrays is read; a NULL vols entry of a sequence that has
 * frames gives those frames zero rows.
 */
int pn2x_hand_interaction_metrics(const pn2x_hand_pose_setup *model, int f, int s, int g, const float *global_r, const float *global_t,
                                  const float *theta, const float *obj_r, const float *obj_t, const float *pred_kp,
                                  const float *rest_joints, const float *rest_verts, const int *rest_of, const void *const *vols,
                                  const int *seq_off, float contact_threshold, float *rows, float *seq, float *out_verts,
                                  float *out_kp, void *stream);

/*
 * Hand and object clouds from depth frames (hotrack_amd/csrc/depth_frame.hip): what the reference's dataset readers do in numpy
 * on the host in front of FPS (datasets/HO3D_dataset.py:66-112, :163-177, DexYCB_dataset.py:76-111) -- back-projection of the valid
 * pixels, the split by segment, the crop to a ball -- for b frames of one size, in two launches over a (tiles, b) grid, a tile
 * being 1024 consecutive pixels.  pn2x_depth_frame is HOST memory, read during the call; its pointers are DEVICE memory:
 *   depth (b,h,w): fp32 metres, or with depth_u16 = 1 uint16 raw counts, z = (float)((double)raw * depth_scale);
 *   seg (b,hs,ws,c) bytes, c 1 or 3, h = f hs and w = f ws with one integer f >= 1: pixel (v,u) reads seg[v / f, u / f];
 *   intrinsics (b,4): fx, fy, cx, cy of each frame;
 *   class k (0 the hand, 1 the object): seg byte channel[k] == value[k], centre[k] (b,3), radius[k].
 * Per pixel, fp32, every operation rounded once (no fused multiply-add): valid if z > 1e-6f; x = ((float)u - cx) * z / fx,
 * y = ((float)v - cy) * z / fy; flip_yz = 1 negates y and z; the pixel is of class k if it is valid, its segment byte matches and
 * sqrtf((dx dx + dy dy) + dz dz) < radius[k] for d = point - centre[k].
 * clouds (b,2,cap,3), counts (b,2) int32 = n, the pixels of the class.  With r the rank of a pixel among its class in row-major
 * pixel order:  n <= cap: the point of rank r in slot r, slots n..cap-1 copies of the point of rank 0 (at distance 0 of FPS's first
 * pick: a sample of a cloud with enough distinct points comes from the real ones);  n > cap: rank r is kept iff
 * floor((r + 1) cap / n) > floor(r cap / n), in slot floor(r cap / n) (64-bit integers) -- exactly cap points, evenly spaced in
 * rank;  n == 0: zeros.  background (b,h,w) bytes: 1 where all c segment bytes of the pixel are zero.
 * work: pn2x_depth_frame_work_ints(b, h, w) = 2 b tiles int32, the per-tile counts the first launch leaves for the second.
 * Every element of every output is written on every call by exactly one workgroup: nothing is pre-set, no atomics, no workgroup
 * waits for another, two calls give the same bits.  No host sync or allocation (capturable).
 * Errors, checked before any device work, PN2_EINVAL before PN2_ERANGE before PN2_ENULL: PN2_EINVAL for b < 0, a size < 1, h / hs
 * and w / ws not one integer factor, c not 1 or 3, a class channel outside [0, c) or value outside [0, 255], a radius that is not
 * > 0, cap < 1, depth_u16 or flip_yz not 0 / 1;  PN2_ERANGE for h w >= 2^29, cap > 16384 (the register-resident FPS range) or
 * b > 65535;  PN2_ENULL for a NULL record or pointer.  b == 0 launches nothing (pointers are then not looked at).
 * pn2x_depth_frame_supported: 1 when a frame geometry passes the checks above.
 */
struct pn2x_depth_frame {
    const void *depth;
    const unsigned char *seg;
    const float *intrinsics;
    const float *centre[2];
    float *clouds;
    int *counts;
    unsigned char *background;
    int *work;
    double depth_scale;
    int b, h, w, hs, ws, c, cap, depth_u16, flip_yz, reserved;
    int channel[2], value[2];
    float radius[2];
}; /* 144 bytes */
typedef struct pn2x_depth_frame pn2x_depth_frame;
int pn2x_depth_frame_supported(int h, int w, int hs, int ws, int c, int cap);
long pn2x_depth_frame_work_ints(int b, int h, int w);
int pn2x_depth_frame_clouds(const pn2x_depth_frame *frames, void *stream);

/*
 * Oriented normals of b point clouds (hotrack_amd/csrc/cloud_normals.hip): what the reference's estimate_normal does with open3d on
 * the host (optimization_obj.py:335-343), in one launch, one wave per query, no host sync or allocation (capturable).
 * points (b,n,3) fp32; valid (b,n) bytes or NULL (every point valid); viewpoint (b,3); normals (b,n,3), variation (b,n).
 * A point is usable when its valid byte is not 0 and its coordinates are finite.  For a usable query: its min(k, usable points)
 * nearest usable points of its own cloud, itself included, by the key (fp32 squared distance bits, index), the lower index on
 * a tie (the order of pn2_knn); their covariance about their mean in two fp32 passes; the unit eigenvector of its smallest
 * eigenvalue from five cyclic Jacobi sweeps on the covariance divided by its trace; variation = lambda0 / (lambda0 + lambda1 +
 * lambda2), lambda0 not below 0.  Zeros for both outputs: a query that is not usable, fewer than 3 usable points, a
 * covariance whose trace is 0 (all neighbours coincide: the farthest neighbour at
 * squared distance 0).
 * orient 0: the component of largest magnitude is positive (the lower index on a tie);  1: n . (viewpoint - p) >= 0;  2: the
 * reference's rule (2 (n (viewpoint - p) > 0) - 1) n, a sign per COMPONENT -- not a geometric orientation, kept because it is
 * what the reference hands to its shape refit.  orient 0 does not read viewpoint (it must still be given).
 * PN2_EINVAL unless b >= 1, 3 <= n <= PN2X_CLOUD_NORMALS_MAX_N (the register-resident selection of knn_wave.h, 32 keys per
 * lane), 3 <= k <= PN2X_CLOUD_NORMALS_MAX_K (one lane per neighbour) and orient in 0..2; PN2_ERANGE for b > PN2X_CLOUD_NORMALS_MAX_B (the launch grid); PN2_ENULL
 * for a NULL points, viewpoint, normals or variation.  Run-to-run bitwise equal.
 */
#define PN2X_CLOUD_NORMALS_MAX_B 65535
#define PN2X_CLOUD_NORMALS_MAX_N 2048
#define PN2X_CLOUD_NORMALS_MAX_K 64
/* the three limits above, for a binding that cannot read this header (NULL: that one is not wanted) */
void pn2x_cloud_normals_limits(int *max_b, int *max_n, int *max_k);
int pn2x_cloud_normals(int b, int n, int k, int orient, const float *points, const unsigned char *valid, const float *viewpoint,
                       float *normals, float *variation, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PN2_EXT_H */
