"""Inputs of the tracked-hand evaluation tests (test_hand_seq_eval.py, test_gpu_hand_seq_eval.py): the golden fixture
(tests/golden/hand_eval.npz, make_golden_hand_eval.py) as `hand_sequence_metrics` inputs and as tracker dictionaries, and seeded
synthetic sequences with the edge frames the kernels must get right."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PALM = [0, 1, 5, 9, 13, 17]
ANGLE_COLS = (5, 7, 9)
FRAME_KEYS = ("pred_kp", "pred_kp_handframe", "init_kp_handframe", "gt_hand_kp", "canon_rotation", "canon_translation", "canon_scale",
              "global_rotation", "global_translation", "gt_rotation", "gt_translation", "MANO_theta")


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "hand_eval.npz"))


def fixture_frames(G, q, dtype=torch.float32, device="cpu"):
    """Sequence q of the fixture -> (frames, palm (1,6,3) or None, keys, per-frame values (T,K), per-sequence values (K,))."""
    frames = {k: torch.from_numpy(G[f"s{q}_{k}"]).to(device, dtype) for k in FRAME_KEYS if f"s{q}_{k}" in G.files}
    if "MANO_theta" in frames:
        frames["gt_MANO_theta"] = torch.from_numpy(G[f"s{q}_gt_mano_pose"][:, 3:]).to(device, dtype)
    palm = None if "global_rotation" in frames else torch.from_numpy(G[f"s{q}_palm_template"]).to(device, dtype)[None]
    return frames, palm, [str(k) for k in G[f"s{q}_keys"]], G[f"s{q}_frames"], G[f"s{q}_seq"]


def tracker_io(frames, palm_template, device="cpu", gt_theta=None):
    """One sequence's stacked `frames` as what HandTrackModel.compute_loss takes: (input, ret_dict_lst), batch 1 per frame."""
    T = frames["pred_kp"].shape[0]
    dev = lambda t: t.to(device)
    data, rets = [], []
    for k in range(T):
        d = {"gt_hand_kp": frames["gt_hand_kp"][k][None], "gt_hand_pose": {"palm_template": palm_template.reshape(1, 6, 3)}}
        if "gt_rotation" in frames:
            d["gt_hand_pose"]["rotation"] = frames["gt_rotation"][k].reshape(1, 3, 3)
            d["gt_hand_pose"]["translation"] = frames["gt_translation"][k].reshape(1, 3, 1)
        r = {"pred_kp": dev(frames["pred_kp"][k][None]), "pred_kp_handframe": dev(frames["pred_kp_handframe"][k][None]),
             "init_kp_handframe": dev(frames["init_kp_handframe"][k][None]),
             "canon_pose": {"rotation": dev(frames["canon_rotation"][k].reshape(1, 3, 3)),
                            "translation": dev(frames["canon_translation"][k].reshape(1, 3, 1)),
                            "scale": dev(frames["canon_scale"][k].reshape(1))}}
        if "global_rotation" in frames:
            r["global_pose"] = {"rotation": dev(frames["global_rotation"][k].reshape(1, 3, 3)),
                                "translation": dev(frames["global_translation"][k].reshape(1, 3, 1))}
        if "MANO_theta" in frames:
            r["MANO_theta"] = dev(frames["MANO_theta"][k][None])
            d["gt_hand_pose"]["mano_pose"] = gt_theta[k][None] if gt_theta is not None else torch.cat([torch.zeros(1, 3), frames["gt_MANO_theta"][k][None].cpu()], 1)
        data.append(d)
        rets.append(r)
    return data, rets


def rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_case(lengths, pose_mode, with_gt=True, with_theta=True, seed=0):
    """Seeded sequences of the given lengths, packed: (frames (fp32, CPU), offsets, palm (S,6,3) or None).

    A frame is a 21-keypoint rest hand (sigma 4 cm, per sequence) under a rigid pose about 0.45 m in front of the camera with
    4 mm of articulation noise: every coordinate stays within 1 m.  Hand frame: the true pose off by 2-8 degrees and 5 mm;
    prediction: ground truth + 3 mm (Kabsch mode: then turned about the wrist by 6-170 degrees); initial keypoints: + 1 cm;
    supplied poses 1.5-170 degrees from the truth.  Edge frames, by
    position in the packed order (when F allows; frame 0 is always one):
      f = 0   every angle column sits at 0 degrees: the hand frame IS the ground-truth pose (column 9), the supplied / fitted
              pose equals the ground-truth one (column 7: identical rotations, or the predicted palm equal to the ground-truth
              palm), and the ground-truth palm is the template moved by the hand frame alone (column 5);
      f = 1   every angle column sits at 180 degrees (the same constructions with a half turn);
      f = 2   Kabsch mode: the predicted palm is the MIRROR image of the ground-truth palm (reflected through a plane that holds
              its centroid): the best proper rotation differs from the best orthogonal map -- the determinant-sign case of
              the rigid fit."""
    rng = np.random.default_rng(9200 + seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    out = {k: [] for k in FRAME_KEYS + ("gt_MANO_theta",)}
    palms = []
    half = rot([0.2, 1.0, 0.4], np.pi)
    f = 0
    for n in lengths:
        rest = rng.normal(0, 0.04, (21, 3))
        rest -= rest[:1]
        palms.append(f32(rest[PALM]))
        R = rot(rng.standard_normal(3), rng.uniform(0.3, 2.5))
        t = np.array([0.05, -0.03, 0.45]) + rng.uniform(-0.05, 0.05, 3)
        dR, vel = rot(rng.standard_normal(3), 0.06), rng.normal(0, 0.002, 3)
        for _ in range(n):
            s = np.float32(rng.choice([0.2, 0.25, 0.17]))  # per-frame scale
            edge = f if f < 3 else -1
            Rc = f32(R @ rot(rng.standard_normal(3), np.deg2rad(rng.uniform(2, 8))))
            tc = f32(t + rng.normal(0, 0.005, 3))
            gR = f32(R)
            if edge == 0:
                gR = Rc.copy()
            elif edge == 1:
                gR = f32(Rc.astype(np.float64) @ half)
            hand = rest + rng.normal(0, 0.004, (21, 3))
            if edge in (0, 1) and not pose_mode:  # the ground-truth palm: the template under the hand frame (and a half turn)
                hand[PALM] = f32(rest[PALM]).astype(np.float64) @ (half.T if edge == 1 else np.eye(3))
                gt = f32(hand @ Rc.astype(np.float64).T + tc)
            else:
                gt = f32(hand @ R.T + t)
            canon = lambda p: f32(((f32(p) - tc) @ Rc) / s).T  # (3,21) in fp32, as the pipeline forms it
            pred_hf = canon(gt + rng.normal(0, 0.003, (21, 3)))
            if not pose_mode:  # the predicted hand turned about its wrist by 6-170 degrees: the fitted poses differ by as much
                turn = rot(rng.standard_normal(3), np.deg2rad(np.exp(rng.uniform(np.log(6.0), np.log(170.0)))))
                pred_hf = f32(turn @ (pred_hf - pred_hf[:, :1]).astype(np.float64) + pred_hf[:, :1])
            if not pose_mode and edge in (0, 1, 2):
                g_hf = canon(gt).astype(np.float64)  # (3,21)
                c = g_hf[:, PALM].mean(axis=1, keepdims=True)
                M = np.eye(3) if edge == 0 else half if edge == 1 else np.eye(3) - 2 * np.outer(*[np.array([0.6, 0.0, 0.8])] * 2)
                pred_hf[:, PALM] = f32(M @ (g_hf[:, PALM] - c) + c)
            init_hf = canon(gt + rng.normal(0, 0.01, (21, 3)))
            pred_kp = f32((s * (Rc @ pred_hf) + tc[:, None]).T)
            pR = f32(R @ rot(rng.standard_normal(3), np.deg2rad(np.exp(rng.uniform(np.log(1.5), np.log(170.0))))))
            if edge == 0:
                pR = gR.copy()
            elif edge == 1:
                pR = f32(gR.astype(np.float64) @ half)
            theta = 0.3 * np.sin(np.arange(45) * 0.7 + 0.3 * f)
            for key, v in (("pred_kp", pred_kp), ("pred_kp_handframe", pred_hf), ("init_kp_handframe", init_hf), ("gt_hand_kp", gt),
                           ("canon_rotation", Rc), ("canon_translation", tc), ("canon_scale", s), ("global_rotation", pR),
                           ("global_translation", f32(t + rng.normal(0, 0.006, 3))), ("gt_rotation", gR), ("gt_translation", f32(t)),
                           ("MANO_theta", f32(theta + rng.normal(0, 0.05, 45))), ("gt_MANO_theta", f32(theta))):
                out[key].append(v)
            R, t = R @ dR, t + vel
            f += 1
    F = offsets[-1]
    shapes = {"pred_kp": (21, 3), "pred_kp_handframe": (3, 21), "init_kp_handframe": (3, 21), "gt_hand_kp": (21, 3),
              "canon_rotation": (3, 3), "canon_translation": (3,), "canon_scale": (), "global_rotation": (3, 3),
              "global_translation": (3,), "gt_rotation": (3, 3), "gt_translation": (3,), "MANO_theta": (45,), "gt_MANO_theta": (45,)}
    frames = {k: torch.from_numpy(np.stack(v).astype(np.float32) if F else np.zeros((0,) + shapes[k], np.float32)) for k, v in out.items()}
    drop = []
    if not pose_mode:
        drop += ["global_rotation", "global_translation"]
        if not with_gt:
            drop += ["gt_rotation", "gt_translation"]
    if not with_theta:
        drop += ["MANO_theta", "gt_MANO_theta"]
    for k in drop:
        del frames[k]
    palm = None if pose_mode else torch.from_numpy(np.stack(palms)) if palms else torch.zeros((0, 6, 3))
    return frames, offsets, palm


def to(frames, palm, device=None, dtype=None):
    mv = lambda t: t.to(device=device, dtype=dtype)
    return {k: mv(v) for k, v in frames.items()}, None if palm is None else mv(palm)


def angle_bounds(oracle_rows):
    """Per-entry bound (degrees) for the angle columns of `oracle_rows` (F,12), fp64: 5e-3 for a true angle in [1, 179] degrees
    (trace rounding <= 2.4e-7 on the cosine over sin 1 degree = 8e-4, palm-point rounding <= 2.4e-7 m over a lever arm >= 2 cm =
    7e-4, their sum with a 3x margin), 0.06 = sqrt(2 * 4.8e-7) rad for a frame built to sit at 0 or 180 degrees (it then lies
    within that 0.06 of either: fp32 rotations are orthogonal to ~1e-7 only).  Any other angle is a mistake of the inputs: the function refuses it, so no frame escapes a bound."""
    a = np.asarray(oracle_rows)[:, list(ANGLE_COLS)]
    mid = (a >= 1.0) & (a <= 179.0)
    end = (a <= 0.06) | (a >= 179.94)
    assert (mid | end).all(), "an input frame sits between the edge and the interior angle ranges: %s" % a[~(mid | end)]
    return np.where(mid, 5e-3, 0.06), mid, end
