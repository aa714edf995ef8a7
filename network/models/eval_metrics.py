"""The reference's per-sequence evaluation of the object trackers, for all frames of a sequence at once: the symmetry-aware
rotation error, the translation error and the 5 deg 5 cm / 10 deg 10 cm accuracies of `eval_part_full`
(pose_utils/part_dof_utils.py:54-78 over pose_utils/metrics.py:6-143) and the chamfer distance of the two posed clouds
(track_network.py:91-94 after the transforms of :431-432).

Every function has two routes with the same results (tests/test_eval_metrics.py, tests/test_gpu_seq_eval.py):
  * the kernel route (hotrack_amd/csrc/seq_eval.hip): fp32 tensors on the GPU.  A fixed number of launches per sequence
    (one for the pose metrics, two for a chamfer), no host sync, capturable into a HIP graph, run-to-run bitwise equal;
  * the torch route: CPU tensors, other dtypes, any device -- the reference's expressions as batched torch operations, chunked
    over the frames so that the (frames, M, N, 3) difference tensor of the chamfer stays below ~256 MB.
The route is chosen per call; the first time the torch route runs the reason is printed (once per reason).  On the GPU with
fp32 tensors a missing HIP library is an error, not a reason to fall back."""
from __future__ import annotations

import math

import torch

_said = set()
CHUNK_FLOATS = 1 << 26  # torch route: largest difference tensor of one chunk of frames (floats)

# diag(s) for the 180-degree flips rot_diff_rad minimises over (metrics.py:61-90 box, :110-123 bottle): identity, xy, xz, yz
_FLIPS = {3: ((1., 1., 1.), (-1., -1., 1.), (-1., 1., -1.), (1., -1., -1.)), -1: ((1., 1., 1.), (-1., 1., -1.))}


def _kernel_route(route, *tensors) -> bool:
    """True: the HIP kernels run.  route: None (by the tensors), 'torch' or 'kernel' (forced: tests, benchmarks)."""
    if route == "torch":
        return False
    why = None
    for t in tensors:
        if not t.is_cuda:
            why = f"the tensors are on {t.device.type}"
        elif t.dtype != torch.float32:
            why = f"the tensors are {t.dtype}"
        if why:
            break
    if why is not None:
        if route == "kernel":
            raise RuntimeError(f"sequence evaluation: the kernel route needs fp32 GPU tensors ({why})")
        if why not in _said:
            _said.add(why)
            print(f"[Sequence evaluation] the torch route runs: {why}")
        return False
    return True


def _poses(R, t):
    return R.reshape(-1, 3, 3), t.reshape(-1, 3)


def _rot_diff_deg(R1, R2, axis: int, up_and_down_sym: bool):
    """rot_diff_degree (metrics.py:6-139) for (T,3,3) batches."""
    prod = R1 * R2
    if 0 <= axis <= 2:  # angle between the chosen columns
        cos = prod[..., axis].sum(-1).clamp(-1.0, 1.0)
        if up_and_down_sym:
            cos = cos.abs()
        rad = torch.acos(cos)
    else:  # trace(R1 diag(s) R2^T) = sum_k s_k (column k of R1 . column k of R2); the minimum angle over the flips
        signs = torch.tensor(_FLIPS.get(axis, ((1., 1., 1.),)), dtype=R1.dtype, device=R1.device)  # (K,3)
        diag = (prod.unsqueeze(-3) * signs[:, None, :]).sum(-1)  # (T,K,3): the diagonal of R1 diag(s) R2^T
        trace = diag[..., 0] + diag[..., 1] + diag[..., 2]
        rad = torch.acos(((trace - 1) / 2.0).clamp(-1.0, 1.0)).min(dim=-1)[0]
    return rad / math.pi * 180.0


def obj_pose_metrics(gt, pred, axis: int = -1, up_and_down_sym: bool = False, route=None) -> torch.Tensor:
    """gt / pred: {'rotation': (T,[1,]3,3), 'translation': (T,[1,]3[,1])} -> (T,4) = [tdiff (m), rdiff (degrees), 5deg5cm,
    10deg10cm] per frame (eval_part_full's terms before its mean over the batch)."""
    gR, gt_ = _poses(gt["rotation"], gt["translation"])
    pR, pt = _poses(pred["rotation"], pred["translation"])
    pR, pt = pR.to(gR.device), pt.to(gR.device)
    axis = int(axis)
    if _kernel_route(route, gR, gt_, pR, pt):
        from hotrack_amd import ext
        return ext.obj_pose_metrics(gR.contiguous(), gt_.contiguous(), pR.contiguous(), pt.contiguous(), axis, bool(up_and_down_sym))
    tdiff = torch.norm(gt_ - pt, p=2, dim=-1)
    rdiff = _rot_diff_deg(gR, pR, axis, bool(up_and_down_sym))
    acc5 = torch.logical_and(rdiff <= 5.0, tdiff <= 0.05).to(tdiff.dtype)
    acc10 = torch.logical_and(rdiff <= 10.0, tdiff <= 0.10).to(tdiff.dtype)
    return torch.stack([tdiff, rdiff.to(tdiff.dtype), acc5, acc10], dim=-1)


METRIC_KEYS = ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")


def eval_part_full(gt, pred, axis: int = -1, up_and_down_sym: bool = False, route=None) -> dict:
    """The reference's eval_part_full for one part: {'tdiff_0', 'rdiff_0', '5deg5cm_0', '10deg10cm_0'} as means over the
    frames (0-dim tensors on the poses' device: nothing is read back here)."""
    m = obj_pose_metrics(gt, pred, axis, up_and_down_sym, route=route).mean(dim=0)
    return {k: m[i] for i, k in enumerate(METRIC_KEYS)}


def posed_chamfer(A, B, Ra, ta, Rb, tb, route=None) -> torch.Tensor:
    """Per-frame chamfer distance of cloud A (N,3) under the poses (Ra (T,3,3), ta (T,3)) to cloud B (M,3) under (Rb, tb):
    (T,) with out[f] = mean_i min_j |Ra_f a_i + ta_f - (Rb_f b_j + tb_f)| + mean_j min_i |...| (compute_chamfer of the two
    transformed clouds, track_network.py:91-94, :431-433).  Identity poses with T = 1 give the un-posed chamfer."""
    A, B = A.reshape(-1, 3), B.reshape(-1, 3)
    Ra, ta = _poses(Ra, ta)
    Rb, tb = _poses(Rb, tb)
    T = Ra.shape[0]
    if T > 0 and (A.shape[0] == 0 or B.shape[0] == 0):
        raise ValueError(f"posed_chamfer: empty cloud (N = {A.shape[0]}, M = {B.shape[0]})")
    if _kernel_route(route, A, B, Ra, ta, Rb, tb):
        from hotrack_amd import ext
        return ext.posed_chamfer(A.contiguous(), B.contiguous(), Ra.contiguous(), ta.contiguous(), Rb.contiguous(), tb.contiguous())
    out = torch.empty(T, dtype=A.dtype, device=A.device)
    step = max(1, CHUNK_FLOATS // max(A.shape[0] * B.shape[0] * 3, 1))
    for f0 in range(0, T, step):
        f1 = min(T, f0 + step)
        pa = torch.matmul(A, Ra[f0:f1].transpose(-1, -2)) + ta[f0:f1, None, :]  # (c,N,3)
        pb = torch.matmul(B, Rb[f0:f1].transpose(-1, -2)) + tb[f0:f1, None, :]  # (c,M,3)
        dist = torch.norm(pa[:, None, :, :] - pb[:, :, None, :], dim=-1)         # (c,M,N)
        out[f0:f1] = dist.min(dim=1)[0].mean(dim=-1) + dist.min(dim=2)[0].mean(dim=-1)
    return out


def to_eval_frame(pose, eval_frame):
    """The reference's change of evaluation frame for HO3D / DexYCB (track_network.py:417-425): R <- R R_c^T, then
    t <- t - R T_c with the new R.  pose {'rotation' (T,3,3), 'translation' (T,3)}; eval_frame {'rotation', 'translation'}."""
    R, t = _poses(pose["rotation"], pose["translation"])
    Rc = eval_frame["rotation"].to(R.device, R.dtype).reshape(3, 3)
    Tc = eval_frame["translation"].to(R.device, R.dtype).reshape(3, 1)
    R2 = torch.matmul(R, Rc.t())
    return {"rotation": R2, "translation": t - torch.matmul(R2, Tc).squeeze(-1)}


# ---- tracked hand sequences -----------------------------------------------------------------------------------------------
# HandTrackNet.compute_loss's dictionary with track_flag set (reference hand_network.py:159-221), in the reference's key order
HAND_METRIC_KEYS = ("hand_pred_kp_loss", "hand_pred_kp_diff", "hand_init_kp_diff", "hand_pred_r_loss", "hand_pred_t_loss",
                    "hand_init_r_diff", "hand_init_t_diff", "hand_pred_r_diff", "hand_pred_t_diff", "hand_canon_r_diff",
                    "hand_canon_t_diff", "MANO_theta_diff")
HAND_INIT_COLUMNS = tuple(i for i, k in enumerate(HAND_METRIC_KEYS) if "init" in k)  # the sequence's first frame, not its mean
_PALM = (0, 1, 5, 9, 13, 17)  # hand_utils.handkp2palmkp


def _kabsch(x, y):
    """Least-squares (R (F,3,3), t (F,3)) with y ~= R x + t for x, y (F,num,3): the reference's solve_rot_and_trans
    (hand_utils.py:42-66), in the tensors' own dtype on their own device."""
    cx, cy = x.mean(dim=1, keepdim=True), y.mean(dim=1, keepdim=True)
    w = torch.bmm((x - cx).transpose(-1, -2), y - cy)
    u, _, vh = torch.linalg.svd(w)
    v = vh.transpose(-1, -2)
    fix = torch.eye(3, dtype=y.dtype, device=y.device).repeat(y.shape[0], 1, 1)
    fix[:, 2, 2] = torch.det(torch.bmm(v, u.transpose(-1, -2)))
    R = torch.bmm(torch.bmm(v, fix), u.transpose(-1, -2))
    return R, (cy - torch.bmm(cx, R.transpose(-1, -2))).squeeze(1)


def _angle_deg(prod):
    """Rotation angle in degrees from the element-wise product of two (F,3,3) rotations (its sum is trace(A^T B))."""
    return torch.acos(((prod.sum(dim=(-1, -2)) - 1) / 2).clamp(-1.0, 1.0)) * (180.0 / math.pi)


def _check_offsets(offsets, F):
    offsets = [int(o) for o in offsets]
    if len(offsets) < 1 or offsets[0] != 0 or offsets[-1] != F or any(b < a for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"hand_sequence_metrics: offsets must be non-decreasing from 0 to the frame count {F}, got {offsets}")
    return offsets


def hand_sequence_metrics(frames: dict, offsets, palm=None, route=None, seq_off=None):
    """The evaluation of tracked hand sequences: F frames of S sequences, packed one sequence after the other.

    frames   the stacked per-frame tensors:
               'pred_kp' (F,21,3), 'pred_kp_handframe' / 'init_kp_handframe' (F,3,21), 'gt_hand_kp' (F,21,3),
               'canon_rotation' (F,3,3), 'canon_translation' (F,3), 'canon_scale' (F,);
             optional 'global_rotation' (F,3,3) + 'global_translation' (F,3): the pose mode (the reference's
               `'global_pose' in ret_dict` branch), which then needs 'gt_rotation' / 'gt_translation';
             optional 'gt_rotation' (F,3,3) + 'gt_translation' (F,3): the hand_canon_* columns;
             optional 'MANO_theta' + 'gt_MANO_theta' (F,45): MANO_theta_diff.
    offsets  the host list of S + 1 frame offsets; palm (S,6,3): the sequences' palm templates (Kabsch mode: without a global
             pose (R, t) / (R_gt, t_gt) are the rigid fits of the template onto the palm keypoints of the scaled predicted /
             ground-truth keypoints).  seq_off: the offsets as an int32 device tensor when the caller holds one (graph capture).
    Returns (rows (F,12), seq (S,12), keys): HAND_METRIC_KEYS columns per frame and per sequence -- the mean of the sequence's
    frames, except the 'init' columns, which are its first frame's (reference track_network.py:300-306); a sequence without
    frames is a row of zeros.  Columns that the inputs do not determine are 0 and missing from `keys`."""
    pose_mode = "global_rotation" in frames
    F = frames["pred_kp"].shape[0]
    offsets = _check_offsets(offsets, F)
    S = len(offsets) - 1
    if frames["pred_kp"].shape[1] != 21:
        raise ValueError(f"hand_sequence_metrics: 21 keypoints per hand, got {frames['pred_kp'].shape[1]}")
    has_gt = "gt_rotation" in frames and "gt_translation" in frames
    has_theta = "MANO_theta" in frames and "gt_MANO_theta" in frames
    if pose_mode and not (has_gt and "global_translation" in frames):
        raise ValueError("hand_sequence_metrics: a global pose needs 'global_translation' and the ground truth 'gt_rotation' / 'gt_translation'")
    if not pose_mode and (palm is None or palm.reshape(-1, 6, 3).shape[0] != S):
        raise ValueError("hand_sequence_metrics: without a global pose every sequence needs its palm template (S,6,3)")
    valid = [True] * 5 + [not pose_mode] * 2 + [True] * 2 + [has_gt] * 2 + [has_theta]
    keys = [k for k, ok in zip(HAND_METRIC_KEYS, valid) if ok]
    g = lambda name, *shape: frames[name].reshape(F, *shape)
    pred_kp, gt_kp = g("pred_kp", 21, 3), g("gt_hand_kp", 21, 3)
    pred_hf, init_hf = g("pred_kp_handframe", 3, 21), g("init_kp_handframe", 3, 21)
    Rc, tc, sc = g("canon_rotation", 3, 3), g("canon_translation", 3), g("canon_scale")
    opt = lambda name, *shape: g(name, *shape) if name in frames else None
    pR, pt = (opt("global_rotation", 3, 3), opt("global_translation", 3)) if pose_mode else (None, None)
    gR, gt_ = (opt("gt_rotation", 3, 3), opt("gt_translation", 3)) if has_gt else (None, None)
    th, thg = (opt("MANO_theta", 45), opt("gt_MANO_theta", 45)) if has_theta else (None, None)
    palm = None if pose_mode else palm.reshape(S, 6, 3)
    used = [t for t in (pred_kp, gt_kp, pred_hf, init_hf, Rc, tc, sc, pR, pt, gR, gt_, th, thg, palm) if t is not None]
    if _kernel_route(route, *used):
        from hotrack_amd import ext
        c = lambda t: None if t is None else t.contiguous()
        rows, seq, mask = ext.hand_seq_metrics(c(pred_hf), c(init_hf), c(gt_kp), c(pred_kp), c(Rc), c(tc), c(sc), offsets, palm=c(palm),
                                               pose_R=c(pR), pose_t=c(pt), gt_R=c(gR), gt_t=c(gt_), theta=c(th), theta_gt=c(thg),
                                               seq_off=seq_off)
        assert mask == sum(1 << i for i, ok in enumerate(valid) if ok), (mask, valid)
        return rows, seq, keys
    dt, dev = pred_kp.dtype, pred_kp.device
    s = sc[:, None, None]
    gt_cm = gt_kp.transpose(-1, -2)  # (F,3,21)
    gt_s = (torch.matmul(Rc.transpose(-1, -2), gt_cm - tc[:, :, None]) / s) * s  # canonicalize (hand_utils.py:30-31), then * scale
    pred_s, init_s = pred_hf * s, init_hf * s
    rows = torch.zeros((F, len(HAND_METRIC_KEYS)), dtype=dt, device=dev)
    rows[:, 0] = (pred_s - gt_s).abs().mean(dim=(1, 2))
    rows[:, 1] = (pred_kp.transpose(-1, -2) - gt_cm).norm(dim=1).mean(dim=-1)
    rows[:, 2] = (init_s - gt_s).norm(dim=1).mean(dim=-1)
    if pose_mode:
        R, t, R_gt, t_gt = pR, pt, gR, gt_
    else:
        lengths = torch.tensor([b - a for a, b in zip(offsets, offsets[1:])], device=dev)
        x = palm.to(dt)[torch.repeat_interleave(torch.arange(S, device=dev), lengths)] if F else palm.to(dt)[:0]
        idx = torch.tensor(_PALM, device=dev)
        if F:
            R_gt, t_gt = _kabsch(x, gt_s.transpose(-1, -2).index_select(1, idx))
            R, t = _kabsch(x, pred_s.transpose(-1, -2).index_select(1, idx))
        else:
            R = R_gt = torch.zeros((0, 3, 3), dtype=dt, device=dev)
            t = t_gt = torch.zeros((0, 3), dtype=dt, device=dev)
        rows[:, 5] = _angle_deg(torch.eye(3, dtype=dt, device=dev) * R_gt)
        rows[:, 6] = t_gt.norm(dim=-1)
    rows[:, 3] = (R - R_gt).abs().mean(dim=(1, 2))
    rows[:, 4] = (t - t_gt).abs().mean(dim=-1)
    rows[:, 7] = _angle_deg(R * R_gt)
    rows[:, 8] = (t - t_gt).norm(dim=-1)
    if has_gt:
        rows[:, 9] = _angle_deg(Rc * gR)
        rows[:, 10] = (gt_ - tc).norm(dim=-1)
    if has_theta:
        rows[:, 11] = (th - thg).abs().mean(dim=-1)
    seq = torch.zeros((S, len(HAND_METRIC_KEYS)), dtype=dt, device=dev)
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b > a:
            seq[q] = rows[a:b].mean(dim=0)
            for col in HAND_INIT_COLUMNS:
                seq[q, col] = rows[a, col]
    return rows, seq, keys


# ---- hand-object interaction of tracked hand sequences ---------------------------------------------------------------------
# What the hand-pose optimiser works on (optimization_hand.py:264-293: penetration, fingertip attraction), measured on the hands
# the tracker ended up with.  The reference has no such evaluation: the definitions are this project's (include/pn2_ext.h:
# pn2x_hand_interaction_metrics).  Columns in millimetres are the kernel's metres times 1000.
HAND_INTERACTION_KEYS = ("hand_pen_depth(mm)", "hand_pen_ratio", "hand_pen_frames", "hand_contact_fingers", "hand_tip_gap(mm)",
                         "hand_obj_min_sdf(mm)", "hand_model_kp_diff", "hand_contact_frames")
HAND_INTERACTION_MM = (0, 4, 5)
_interaction_models = {}


def _interaction_model(tables, device):
    """ext.hand_pose_model of a skinning-table dict on a device, built once (the dict is kept: its id stays its own)."""
    key = (id(tables), str(device))
    if key not in _interaction_models:
        from hotrack_amd import ext
        _interaction_models[key] = (tables, ext.hand_pose_model(tables, device))
    return _interaction_models[key][1]


def nearest_voxel_sdf(points, obj_r, obj_t, volume, voxel_scale):
    """gf_optimize_hand_pose.query_sdf (optimization_hand.py:252-262) as torch operations: points (F,V,3) in the object frames
    (obj_r (F,3,3), obj_t (F,3)) -> the value of the voxel clamp(q // voxel_scale, -(res/2), res/2) + res/2 per axis, in the
    points' dtype."""
    half = volume.shape[0] // 2
    o = torch.matmul(points - obj_t[:, None, :], obj_r)
    idx = torch.clamp(torch.div(o, voxel_scale, rounding_mode="floor"), -half, half).long() + half
    return volume.to(points.device)[idx[..., 0], idx[..., 1], idx[..., 2]].to(points.dtype)


def hand_interaction_metrics(frames: dict, offsets, tables, volumes, voxel_scale, contact_threshold=0.005, route=None, seq_off=None):
    """How the tracked hands sit against their objects: F frames of S sequences, packed one sequence after the other.

    frames   'MANO_theta' (F,45), 'global_rotation' (F,3,3) (used as a matrix, as the optimiser uses it), 'global_translation'
             (F,3), 'obj_rotation' (F,3,3), 'obj_translation' (F,3);
             optional 'pred_kp' (F,21,3): the keypoints the tracker reported (hand_model_kp_diff);
             optional 'beta' (G,D) + 'rest_of' (F,) integer: G shape codes and the one each frame is posed with (a tracker
             that re-estimates the shape has several per sequence); without them the hand is the tables' rest hand.
    offsets  the host list of S + 1 frame offsets;  tables: HandModel.skinning_tables();  volumes: the S sequences' SDF volumes
             (res,res,res), one resolution and dtype (None for a sequence without frames);  voxel_scale: their spacing.
    Every vertex of the posed hand reads the nearest voxel of its sequence's volume in the frame's object frame -- the
    optimiser's own lookup -- and a frame's row is
      hand_pen_depth(mm)    max of -sdf over the vertices inside (sdf < 0), else 0;      hand_pen_ratio  their share;
      hand_pen_frames       1 if any vertex is inside;       hand_contact_fingers  fingers whose tip region (contact zone) comes
      within contact_threshold of the surface (min sdf <= threshold);      hand_tip_gap(mm)  mean over the fingers of
      max(min sdf over the tip region, 0);      hand_obj_min_sdf(mm)  the signed minimum over all vertices;
      hand_model_kp_diff    mean distance of the posed model's keypoints to 'pred_kp' (metres; absent without it);
      hand_contact_frames   1 if any finger is in contact.
    Returns (rows (F,8), seq (S,8), keys): HAND_INTERACTION_KEYS columns per frame and their mean per sequence (zeros for a
    sequence without frames); `keys` lists the valid columns.  The kernel route (fp32 GPU tensors, a GPU volume; two launches,
    hotrack_amd/csrc/hand_interact.hip) and the torch route (lbs_forward_from_tables + nearest_voxel_sdf, chunked over the
    frames, any device and dtype) are chosen as for the other functions.  seq_off: the offsets as an int32 device tensor when
    the caller holds one."""
    theta = frames["MANO_theta"]
    F = theta.shape[0]
    offsets = _check_offsets(offsets, F)
    S = len(offsets) - 1
    if len(volumes) != S:
        raise ValueError(f"hand_interaction_metrics: {len(volumes)} volumes for {S} sequences")
    g = lambda name, *shape: frames[name].reshape(F, *shape)
    theta, R, t, oR, ot = g("MANO_theta", 45), g("global_rotation", 3, 3), g("global_translation", 3), g("obj_rotation", 3, 3), g("obj_translation", 3)
    pred_kp = g("pred_kp", 21, 3) if "pred_kp" in frames else None
    has_shape = "beta" in frames and "shape_joints" in tables
    beta = frames["beta"].reshape(-1, tables["shape_joints"].shape[0]) if has_shape else None
    rest_of = frames["rest_of"].reshape(F).long() if has_shape and "rest_of" in frames else torch.zeros(F, dtype=torch.long, device=theta.device)
    keys = [k for i, k in enumerate(HAND_INTERACTION_KEYS) if i != 6 or pred_kp is not None]
    unit = torch.ones(len(HAND_INTERACTION_KEYS), dtype=theta.dtype, device=theta.device)
    unit[list(HAND_INTERACTION_MM)] = 1000.0
    used = [x for x in (theta, R, t, oR, ot, pred_kp, beta) if x is not None]
    vols_gpu = all(v is None or (v.is_cuda and v.dtype in (torch.float16, torch.float32)) for v in volumes)
    if not vols_gpu and route == "kernel":
        raise RuntimeError("sequence evaluation: the kernel route needs fp16 / fp32 GPU volumes")
    if not vols_gpu and route is None and "volumes" not in _said:
        _said.add("volumes")
        print("[Sequence evaluation] the torch route runs: the SDF volumes are not fp16 / fp32 GPU tensors")
    if _kernel_route(route if vols_gpu else "torch", *used):
        from hotrack_amd import ext
        dev = theta.device
        model = _interaction_model(tables, dev)
        c = lambda x: None if x is None else x.contiguous()
        if beta is None:
            rest = (model["rest_joints"][None].contiguous(), model["rest_verts"][None].contiguous())
        else:
            G = beta.shape[0]
            rest = ((model["rest_joints"][None] + (beta @ model["shape_joints"]).view(G, -1, 3)).contiguous(),
                    (model["rest_verts"][None] + (beta @ model["shape_verts"]).view(G, -1, 3)).contiguous())
        rows, seq, mask, _, _ = ext.hand_interaction_metrics(model, c(R), c(t), c(theta), c(oR), c(ot), rest, rest_of.to(torch.int32).contiguous(),
                                                             [None if v is None else v.contiguous() for v in volumes], float(voxel_scale),
                                                             offsets, float(contact_threshold), pred_kp=c(pred_kp), seq_off=seq_off)
        assert mask == (0xff if pred_kp is not None else 0xbf), mask
        return rows * unit, seq * unit, keys
    from .hand_model import lbs_forward_from_tables
    dt, dev = theta.dtype, theta.device
    V = tables["rest_verts"].shape[0]
    offs = [int(o) for o in tables["finger_offsets"]]
    regions = [tables["tips"][offs[i]:offs[i + 1]].long().unique().to(dev) for i in range(5)]
    thr = torch.tensor(float(contact_threshold), dtype=dt, device=dev)
    rows = torch.zeros((F, len(HAND_INTERACTION_KEYS)), dtype=dt, device=dev)
    step = max(1, CHUNK_FLOATS // max(V * 3 * 135, 1))
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b > a and volumes[q] is None:
            raise ValueError(f"hand_interaction_metrics: sequence {q} has frames and no volume")
        for f0 in range(a, b, step):
            f1 = min(b, f0 + step)
            n = f1 - f0
            pose = torch.cat([torch.zeros((n, 3), dtype=dt, device=dev), theta[f0:f1]], dim=1)
            verts, kp = lbs_forward_from_tables(tables, pose, t[f0:f1], None if beta is None else beta[rest_of[f0:f1]], root_R=R[f0:f1])
            sdf = nearest_voxel_sdf(verts, oR[f0:f1], ot[f0:f1], volumes[q], float(voxel_scale))  # (n,V)
            inside = sdf < 0
            r = rows[f0:f1]
            r[:, 0] = torch.where(inside, -sdf, torch.zeros_like(sdf)).max(dim=1)[0]
            r[:, 1] = inside.sum(dim=1).to(dt) / V
            r[:, 2] = (r[:, 0] > 0).to(dt)
            fingers = 0
            for idx in regions:
                if idx.numel():
                    m = sdf[:, idx].min(dim=1)[0]
                    r[:, 3] += (m <= thr).to(dt)
                    r[:, 4] += m.clamp_min(0)
                    fingers += 1
            if fingers:
                r[:, 4] /= fingers
            r[:, 5] = sdf.min(dim=1)[0]
            if pred_kp is not None:
                r[:, 6] = (kp - pred_kp[f0:f1]).norm(dim=-1).mean(dim=1)
            r[:, 7] = (r[:, 3] > 0).to(dt)
    seq = torch.zeros((S, len(HAND_INTERACTION_KEYS)), dtype=dt, device=dev)
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b > a:
            seq[q] = rows[a:b].mean(dim=0)
    return rows * unit, seq * unit, keys
