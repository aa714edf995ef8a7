"""Generates tests/golden/iknet_reference.npz from the IMPORTED reference's IKNet (hand_network.py:246-335) and its quaternion
helpers (hand_utils.py:13-28).  RUNS ONLY IN THE BUILD CONTAINER (needs the reference checkout); tests and the GPU box only read
the .npz.

The reference class is created with object.__new__ (its __init__ builds a MANO layer: licensed assets) with its layers and
attributes set as __init__ sets them; the weights and BatchNorm statistics are the closed-form lattices of tests/_iknet_cases.py
(the tests recompute them).  forward runs in eval mode with track_flag = opt_flag = True (no MANO layer call) on CPU.

Cases: B in {1, 3, 16} x iknetframe {kp, camera} x palm template {zero shape, shaped hand}; keypoints of this repository's
SyntheticLBSHand at seeded poses, global rotations and translations, plus noise.  Helper cases: mano_quat2axisang on the identity,
w < 0, near-pi, tiny-angle and unnormalised quaternions (and, if the search finds one, a quaternion whose 1 - w^2 rounds below
zero: the reference's NaN), mano_axisang2quat on zero, tiny, near-pi and generic axis-angles."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _iknet_cases import iknet_state  # noqa: E402
from make_golden import import_reference  # noqa: E402
from make_golden_hand import _load  # noqa: E402

PALM = [0, 1, 5, 9, 13, 17]


def _rot(rng):
    a = rng.standard_normal(3)
    a = a / np.linalg.norm(a) * rng.uniform(0, np.pi)
    return a


def make_ref(ref_hn, frame):
    o = object.__new__(ref_hn.IKNet)
    nn.Module.__init__(o)
    o.device = "cpu"
    o.linear, o.bn = nn.ModuleList(), nn.ModuleList()
    last = 126
    for _ in range(6):
        o.linear.append(nn.Linear(last, 1024))
        o.bn.append(nn.BatchNorm1d(1024))
        last = 1024
    o.linear.append(nn.Linear(1024, 60))
    o.layer_num, o.iknetframe = 6, frame
    sd = o.state_dict()
    with torch.no_grad():
        for k, v in iknet_state().items():
            sd[k].copy_(torch.from_numpy(v))
    return o.eval()


def main():
    _, ref_hn = import_reference()
    SyntheticLBSHand = _load("hand_model").SyntheticLBSHand
    hand, shaped = SyntheticLBSHand(), SyntheticLBSHand(num_betas=10)
    beta = torch.linspace(-1.5, 1.5, 10)[None]
    with torch.no_grad():
        _, rest0 = hand.forward(th_pose_coeffs=torch.zeros(1, 48), th_trans=torch.zeros(1, 3))
        _, rest1 = shaped.forward(th_pose_coeffs=torch.zeros(1, 48), th_trans=torch.zeros(1, 3), th_betas=beta)
    palms = {"zero": rest0[:, PALM].float(), "shaped": rest1[:, PALM].float()}
    out = {"palm_zero": palms["zero"].numpy(), "palm_shaped": palms["shaped"].numpy()}
    refs = {f: make_ref(ref_hn, f) for f in ("kp", "camera")}
    out["state_keys"] = np.array(list(refs["kp"].state_dict().keys()))
    out["state_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in refs["kp"].state_dict().values()], np.int64)
    report = {}
    rng = np.random.default_rng(2024)
    flags = {"track_flag": True, "opt_flag": True}
    for B in (1, 3, 16):
        glob = np.stack([_rot(rng) for _ in range(B)]).astype(np.float32)
        pose = rng.uniform(-0.5, 0.5, (B, 45)).astype(np.float32)
        trans = (np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.1, 0.1, (B, 3))).astype(np.float32)
        with torch.no_grad():
            _, kp = hand.forward(th_pose_coeffs=torch.from_numpy(np.concatenate([glob, pose], 1)), th_trans=torch.from_numpy(trans))
        kp = (kp + torch.from_numpy(rng.normal(0, 0.005, kp.shape).astype(np.float32))).float()
        gt = (kp + torch.from_numpy(rng.normal(0, 0.003, kp.shape).astype(np.float32))).float()
        mano_pose = torch.from_numpy(np.concatenate([glob, pose], 1))
        out[f"B{B}_kp"], out[f"B{B}_gt_kp"], out[f"B{B}_mano_pose"] = kp.numpy(), gt.numpy(), mano_pose.numpy()
        for frame in ("kp", "camera"):
            for pname, palm in palms.items():
                data = {"gt_hand_kp": gt, "pred_palm_template": palm.expand(B, -1, -1).contiguous(), "baseline_pred_kp": kp.clone(),
                        "pred_beta": None, "gt_hand_pose": {"mano_pose": mano_pose}}
                with torch.no_grad():
                    ret = refs[frame](data, dict(flags))
                    loss, _ = refs[frame].compute_loss(data, ret, dict(flags))
                key = f"B{B}_{frame}_{pname}"
                out[f"{key}_raw_quat"] = ret["raw_quat"].numpy()
                out[f"{key}_MANO_theta"] = ret["MANO_theta"].numpy()
                out[f"{key}_R"] = ret["global_pose"]["rotation"].numpy()
                out[f"{key}_t"] = ret["global_pose"]["translation"].numpy()
                out[f"{key}_init_kp_handframe"] = ret["init_kp_handframe"].numpy()
                out[f"{key}_gt_quat"] = ret["gt_quat"].numpy()
                out[f"{key}_quat_loss"] = np.float32(loss["quat_loss"])
                out[f"{key}_init_gt_kp_diff"] = np.float32(loss["init_gt_kp_diff"])
                report[key] = {"raw_quat_absmax": float(ret["raw_quat"].abs().max()), "quat_loss": float(loss["quat_loss"]),
                               "theta_finite": bool(torch.isfinite(ret["MANO_theta"]).all())}
    # ---- quaternion helpers ---------------------------------------------------------------------------------------------
    q = [[1, 0, 0, 0], [-0.5, 0.5, 0.5, 0.5], [-1, 0, 0, 0], [1e-4, 1, 0, 0], [0.9999999, 3e-4, -2e-4, 1e-4], [2.0, 0.2, -0.4, 0.6],
         [0.3, -0.2, 0.9, 0.1], [-0.2, -0.7, 0.1, 0.6], [0, 0, 0, 1], [1, 1e-9, 0, 0]]
    quats = torch.tensor(q, dtype=torch.float32).reshape(1, -1)
    out["helper_quat"] = quats.numpy()
    out["helper_quat_axisang"] = ref_hn.mano_quat2axisang(quats).numpy()
    # a quaternion whose normalised w rounds so that 1 - w^2 < 0 (the reference: NaN) -- searched, kept if found
    g = torch.Generator().manual_seed(5)
    cand = torch.cat([1 + torch.rand(20000, 1, generator=g), torch.zeros(20000, 3)], 1)  # sqrt(w^2) may round below w
    aa = ref_hn.mano_quat2axisang(cand.reshape(1, -1)).reshape(-1, 3)
    bad = torch.nonzero(torch.isnan(aa).any(-1)).flatten()
    out["helper_nan_quat"] = cand[bad[:4]].reshape(1, -1).numpy() if len(bad) else np.zeros((1, 0), np.float32)
    report["nan_cases_found"] = int(len(bad))
    a = [[0, 0, 0], [1e-9, 0, 0], [1e-5, -2e-5, 1e-5], [3.1415, 0, 0], [0, -3.14159, 0], [0.3, -0.2, 0.5], [1.0, 2.0, -0.5], [-2.5, 1.0, 0.2]]
    aas = torch.tensor(a, dtype=torch.float32).reshape(1, -1)
    out["helper_axisang"] = aas.numpy()
    out["helper_axisang_quat"] = ref_hn.mano_axisang2quat(aas).numpy()
    np.savez_compressed(os.path.join(HERE, "iknet_reference.npz"), **out)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
