"""Command-line flags of train.py / test.py (same flag names as the reference's parse_args.py)."""


def add_args(parser):
    parser.add_argument("--config", type=str, default=None)
    parser.add_argument("--track", default=None, choices=["hand", "hand_IKNet", "obj_opt", False], help="tracking for test")
    parser.add_argument("--num_workers", type=int, default=0, help="num_workers in data_loader")
    parser.add_argument("--debug", action="store_true", default=False)
    parser.add_argument("--debug_save", action="store_true", default=False)
    parser.add_argument("--save", action="store_true", default=False)
    parser.add_argument("--data_config", type=str, default=None)
    parser.add_argument("--obj_category", type=str, default=None)
    parser.add_argument("--experiment_dir", type=str, default=None)
    parser.add_argument("--batch_size", type=int, default=None)
    parser.add_argument("--cuda_id", type=int, default=None)
    parser.add_argument("--total_epoch", default=None, type=int)
    parser.add_argument("--optimizer", type=str, default=None)
    parser.add_argument("--weight_decay", type=float, default=None)
    parser.add_argument("--learning_rate", type=float, default=None)
    parser.add_argument("--lr_policy", type=str, default=None)
    parser.add_argument("--lr_gamma", type=float, default=None)
    parser.add_argument("--lr_step_size", type=int, default=None)
    parser.add_argument("--lr_clip", type=float, default=None)
    parser.add_argument("--num_points", type=int, default=None)
    parser.add_argument("--freq/save", type=int, default=None, help="ckpt saving frequency in epochs")
    parser.add_argument("--pointnet_cfg/camera", type=str, default=None)
    parser.add_argument("--network/type", type=str, default=None)
    parser.add_argument("--network/backbone_out_dim", type=int, default=None)
    # additions of this repo (synthetic runs)
    parser.add_argument("--synthetic_frames", type=int, default=None, help="length of the synthetic train set / sequences")
    parser.add_argument("--max_iters", type=int, default=None, help="stop an epoch after this many iterations (smoke runs)")
    parser.add_argument("--hand_model", type=str, default=None, choices=["synthetic", "synthetic_shaped", "synthetic_mano"],
                        help="track=hand_IKNet with use_optimization: the hand model of the pose optimiser ('synthetic' = the "
                             "linear-blend-skinning stand-in of models/hand_model.py; 'synthetic_shaped' = the same with 10 shape "
                             "dimensions, for use_pred_hand_shape; 'synthetic_mano' = a hand with MANO's structure -- pose blend shapes, mean "
                             "pose, regressed joints, vertex fingertips, root centring -- and seeded tables; a MANO layer is passed "
                             "programmatically)")
    parser.add_argument("--hand_particles", type=int, default=None, help="candidate hands per optimiser iteration (reference: 5120)")
    parser.add_argument("--fused_hand_pose", dest="opt/fused_pose", action="store_const", const=True, default=None,
                        help="use_optimization: run the hand-pose particle optimiser on the device-resident route (two kernels per "
                             "iteration, hotrack_amd/csrc/hand_pose.hip) instead of the torch route; needs a hand model with "
                             "plain skinning tables")
    parser.add_argument("--fused_hand_eval", dest="fused_hand_eval", action="store_const", const=True, default=None,
                        help="track=hand / hand_IKNet: evaluate the tracked sequences through HandTrackModel.compute_loss_batch (every "
                             "frame's metrics from two launches, hotrack_amd/csrc/kabsch.hip; adds MANO_theta_diff and the per-frame "
                             "error table; the hand_init_* keys are then the first frame's value, as in the reference, not the mean)")
    parser.add_argument("--hand_interaction_eval", dest="hand_interaction_eval", action="store_const", const=True, default=None,
                        help="track=hand_IKNet with a hand model: also report how the tracked hands sit against the object -- "
                             "hand_pen_depth(mm), hand_pen_ratio, hand_pen_frames, hand_contact_fingers, hand_tip_gap(mm), "
                             "hand_obj_min_sdf(mm), hand_model_kp_diff, hand_contact_frames -- from the tracked MANO_theta / global_pose, "
                             "the object pose the optimiser used and the sequence's SDF volume (two launches per evaluation, "
                             "hotrack_amd/csrc/hand_interact.hip; the contact distance is opt.contact_threshold, default 0.005 m)")
    parser.add_argument("--accumulate_obj_surface", dest="opt/accumulate_surface", action="store_const", const=True, default=None,
                        help="track=obj_opt: keep each sequence's observed surface -- the clouds the tracker saw, in the object "
                             "frame, filtered to 2 cm of the model and folded into a fixed-size merged cloud with oriented normals "
                             "(models/obs_surface.py, hotrack_amd/csrc/cloud_normals.hip; the bookkeeping of the reference's "
                             "opt.updateobjshape route without its DeepSDF refit) -- and report obs_surface_residual(mm) and "
                             "obs_surface_normal_agree; --save writes the surface into the sequence's pickle.  The tracked poses do "
                             "not depend on it")
    parser.add_argument("--extract_obj_mesh", dest="opt/extract_mesh", action="store_const", const=True, default=None,
                        help="track=obj_opt: at the end of a sequence extract the triangle mesh of the sequence's SDF volume "
                             "(models/mesh_sdf.volume_to_mesh, hotrack_amd/csrc/sdf_mesh.hip; the reference's sdf2mesh) into "
                             "ret_dict_lst[0]['obj_info']; --save writes it as a PLY ('recon_path').  A sequence that carries "
                             "neither obj_model_points nor a mesh samples it for the chamfer columns.  The tracked poses do not "
                             "depend on it")
    parser.add_argument("--fuse_obj_depth", dest="opt/fuse_depth", action="store_const", const=True, default=None,
                        help="track=obj_opt on frames that carry depth images (--from_depth): fuse every tracked depth frame into the "
                             "sequence's own copy of the SDF volume as a truncated signed distance, a weighted running average per "
                             "voxel (models/shape_fusion.py, hotrack_amd/csrc/tsdf_fuse.hip), reload the optimiser's volume every "
                             "opt.fuse_every frames (10) and put the fused volume into ret_dict_lst[0]['obj_fused']; with "
                             "--extract_obj_mesh the PLY is the reconstruction.  opt.fuse_trunc (5 voxels) and opt.fuse_prior_weight "
                             "(8) are read from the configuration.  With --seq_batch > 1 only together with --lockstep_fuse")
    parser.add_argument("--lockstep_fuse", dest="opt/lockstep_fuse", action="store_const", const=True, default=None,
                        help="track=obj_opt: allow --fuse_obj_depth with --seq_batch > 1.  The sequences of a group flush their pending "
                             "frames in one launch (hotrack_amd.sdf.tsdf_integrate_batch) and every sequence gets, bit for bit, the "
                             "poses and the fused volume of --seq_batch 1.  Opt-in for its memory: a fused volume cannot be shared, so "
                             "every sequence of a group owns a copy of the volume and its weights and, from its first flush on, of "
                             "the corner layout -- at 201^3 fp16 about 49 MB plus 130 MB per sequence.  Without --fuse_obj_depth "
                             "it changes nothing")
    parser.add_argument("--render_obj_model", dest="opt/render_model", action="store_const", const=True, default=None,
                        help="track=obj_opt on frames that carry depth images (--from_depth): at the end of a sequence render its SDF "
                             "volume (with --fuse_obj_depth the fused one) at every tracked pose in one launch and compare the depth "
                             "maps with the observed frames in a second (models/volume_render.py, hotrack_amd/csrc/sdf_raycast.hip); "
                             "report model_depth_residual(mm), model_silhouette_iou and model_occluded_ratio, which need no ground "
                             "truth, and put the maps into ret_dict_lst[0]['obj_render']; --save writes the last frame's depth and "
                             "normal maps as <sequence>_model_depth.png / _model_normal.png.  opt.render_occl_margin (0.01 m) is read "
                             "from the configuration.  The tracked poses do not depend on it")
    parser.add_argument("--obj_model_radius", type=float, default=None,
                        help="track=obj_opt, synthetic sequences: the radius of the capsule the handed-over SDF volume describes "
                             "(default 0.04, the true one the clouds and depth frames show): another value hands over a wrong model")
    parser.add_argument("--refine_obj_pose", dest="opt/refine_pose", action="store_const", const=True, default=None,
                        help="track=obj_opt: after every frame's particle search take opt.refine_iters (8) damped Gauss-Newton steps "
                             "on the SDF volume, over the points within opt.refine_band (0.02 m) of the surface, in one more launch "
                             "per frame or group step (gf_optimize_obj.refine, hotrack_amd/csrc/sdf_refine.hip).  The refined pose "
                             "is the frame's pose: the next frame starts from it, and fusion, rendering, the observed surface and "
                             "the mesh read it.  Reports refine_cost_drop and refine_accepted_steps; the per-frame figures go into "
                             "ret_dict_lst[0]['obj_refine'].  Off by default: the poses are then bit for bit what they were")
    parser.add_argument("--obj_mesh", type=str, default=None,
                        help="track the synthetic sequences' clouds against an SDF volume built from this triangle mesh (OBJ or "
                             "PLY, object frame, metres; models/mesh_sdf.py) instead of the analytic capsule volume")
    parser.add_argument("--obj_as_mesh", action="store_const", const=True, default=None,
                        help="the synthetic sequences carry the capsule as a triangle mesh and the tracker builds the volume")
    parser.add_argument("--from_depth", action="store_const", const=True, default=None,
                        help="the synthetic hand-object and object sequences hand over rendered depth frames (depth, seg, intrinsics, "
                             "crop centres) instead of clouds, and the trackers build hand_points / obj_points / background_mask on "
                             "the GPU (models/frame_frontend.py, hotrack_amd/csrc/depth_frame.hip)")
    parser.add_argument("--seq_batch", type=int, default=1,
                        help="test.py, track=obj_opt: track this many sequences in lockstep on one batched optimiser call per frame "
                             "step (same poses, bit for bit, as one sequence at a time); 1 = one sequence at a time")
    return parser


SEQ_BATCH_TRACKS = ("obj_opt",)


def check_seq_batch(seq_batch, track):
    """--seq_batch > 1 exists for the object tracker only: refuse anything else before any work is done."""
    if seq_batch < 1:
        raise SystemExit("--seq_batch must be >= 1, got %d" % seq_batch)
    if seq_batch > 1 and track not in SEQ_BATCH_TRACKS:
        raise SystemExit("--seq_batch %d needs track: obj_opt (the object tracker's sequences are tracked in lockstep on the batched "
                         "particle optimiser); this configuration has track: %s, which tracks one sequence at a time -- drop the flag"
                         % (seq_batch, track))
