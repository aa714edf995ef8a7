"""Generates tests/golden/hand_eval.npz from the IMPORTED reference's HandTrackNet.compute_loss (hand_network.py:159-221) with
track_flag set, and the sequence rule of its HandTrackModel.compute_loss (track_network.py:300-306).  RUNS ONLY WHERE THE
REFERENCE IS CHECKED OUT (make_golden_track.REF); the tests only read the .npz file.  No reference file is touched or copied.

The reference class is created with object.__new__ (its __init__ builds the whole network; compute_loss reads `device` and
`handframe` only) and called frame by frame, batch 1, over two short synthetic sequences:
  sequence 0   5 frames with a `global_pose`, `MANO_theta` and IKNet_flag: the pose branch and MANO_theta_diff;
  sequence 1   3 frames with neither: the two palm fits (ransac_rt) and the hand_init_r / hand_init_t keys.
A hand is a seeded 21-keypoint rest pose under a rigid motion plus per-joint articulation noise; the hand frame is the true pose
perturbed by a few degrees / millimetres, the prediction is the ground truth plus 3 mm of noise, the initial keypoints plus
1 cm.  Stored: every input, the reference's dictionary per frame (keys in its order) and per sequence (mean over the frames,
the `init` keys from frame 0)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_track import REF, import_reference  # noqa: E402

LENGTHS = (5, 3)
PALM = [0, 1, 5, 9, 13, 17]


def rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def sequence(q, frames, with_pose):
    rng = np.random.default_rng(7100 + q)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    rest = rng.normal(0, 0.04, (21, 3))
    rest -= rest[:1]
    R = rot(rng.standard_normal(3), rng.uniform(0.3, 2.5))
    t = np.array([0.05, -0.03, 0.45]) + rng.uniform(-0.05, 0.05, 3)
    dR, vel = rot(rng.standard_normal(3), 0.06), rng.normal(0, 0.004, 3)
    out = {k: [] for k in ("gt_hand_kp", "gt_rotation", "gt_translation", "canon_rotation", "canon_translation", "canon_scale",
                           "pred_kp", "pred_kp_handframe", "init_kp_handframe")}
    if with_pose:
        out.update({k: [] for k in ("global_rotation", "global_translation", "MANO_theta", "gt_mano_pose")})
    for k in range(frames):
        gt = (rest + rng.normal(0, 0.004, (21, 3))) @ R.T + t
        Rc = f32(R @ rot(rng.standard_normal(3), np.deg2rad(rng.uniform(2, 8))))
        tc = f32(t + rng.normal(0, 0.005, 3))
        s = np.float32(0.2)
        canon = lambda p: f32(((p - tc) @ Rc) / s).T  # (3,21): R^T (p - t) / s
        pred_hf = canon(gt + rng.normal(0, 0.003, (21, 3)))
        init_hf = canon(gt + rng.normal(0, 0.01, (21, 3)))
        pred_kp = f32((s * (Rc @ pred_hf) + tc[:, None]).T)
        for key, v in (("gt_hand_kp", f32(gt)), ("gt_rotation", f32(R)), ("gt_translation", f32(t)), ("canon_rotation", Rc),
                       ("canon_translation", tc), ("canon_scale", s), ("pred_kp", pred_kp), ("pred_kp_handframe", pred_hf),
                       ("init_kp_handframe", init_hf)):
            out[key].append(v)
        if with_pose:
            theta = 0.3 * np.sin(np.arange(45) * 0.7 + 0.3 * k)
            out["global_rotation"].append(f32(R @ rot(rng.standard_normal(3), np.deg2rad(rng.uniform(1, 12)))))
            out["global_translation"].append(f32(t + rng.normal(0, 0.006, 3)))
            out["MANO_theta"].append(f32(theta + rng.normal(0, 0.05, 45)))
            out["gt_mano_pose"].append(f32(np.concatenate([rng.normal(0, 1, 3), theta])))
        R, t = R @ dR, t + vel
    out = {k: np.stack(v) for k, v in out.items()}
    out["palm_template"] = f32(rest[PALM])
    return out


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference is checked out"
    _, ref_hn, _ = import_reference()
    net = object.__new__(ref_hn.HandTrackNet)
    torch.nn.Module.__init__(net)
    net.device, net.handframe = "cpu", "kp"
    T = torch.from_numpy
    out = {"lengths": np.array(LENGTHS, dtype=np.int32)}
    for q, frames in enumerate(LENGTHS):
        with_pose = q == 0
        d = sequence(q, frames, with_pose)
        flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": with_pose}
        per_frame, keys = [], None
        for k in range(frames):
            data = {"gt_hand_kp": T(d["gt_hand_kp"][k])[None],
                    "gt_hand_pose": {"palm_template": T(d["palm_template"])[None], "rotation": T(d["gt_rotation"][k]).reshape(1, 3, 3),
                                     "translation": T(d["gt_translation"][k]).reshape(1, 3, 1)}}
            ret = {"pred_kp": T(d["pred_kp"][k])[None], "pred_kp_handframe": T(d["pred_kp_handframe"][k])[None],
                   "init_kp_handframe": T(d["init_kp_handframe"][k])[None],
                   "canon_pose": {"rotation": T(d["canon_rotation"][k]).reshape(1, 3, 3), "translation": T(d["canon_translation"][k]).reshape(1, 3, 1),
                                  "scale": T(np.array([d["canon_scale"][k]], dtype=np.float32))}}
            if with_pose:
                data["gt_hand_pose"]["mano_pose"] = T(d["gt_mano_pose"][k])[None]
                ret["MANO_theta"] = T(d["MANO_theta"][k])[None]
                ret["global_pose"] = {"rotation": T(d["global_rotation"][k]).reshape(1, 3, 3), "translation": T(d["global_translation"][k]).reshape(1, 3, 1)}
            with torch.no_grad():
                loss, _ = net.compute_loss(data, ret, flags)
            keys = list(loss) if keys is None else keys
            assert list(loss) == keys
            per_frame.append(loss)
        # track_network.py:234-241, :300-306: the running sum over the frames / their number, 'init' keys from frame 0
        total = dict(per_frame[0])
        for fr in per_frame[1:]:
            total = {k: total[k] + fr[k] for k in keys}
        seq = [float(per_frame[0][k]) if "init" in k else float(total[k] / frames) for k in keys]
        for name, v in d.items():
            out[f"s{q}_{name}"] = v
        out[f"s{q}_keys"] = np.array(keys)
        out[f"s{q}_frames"] = np.array([[float(fr[k]) for k in keys] for fr in per_frame], dtype=np.float32)
        out[f"s{q}_seq"] = np.array(seq, dtype=np.float32)
        print(f"sequence {q}: {keys}")
        print(np.round(out[f"s{q}_frames"], 5))
        print("per sequence:", np.round(out[f"s{q}_seq"], 5))
    path = os.path.join(HERE, "hand_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
