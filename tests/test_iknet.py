"""CPU: IKNet (network/models/iknet.py) against the imported reference's IKNet (tests/golden/iknet_reference.npz, written by
tests/golden/make_golden_iknet.py), its quaternion helpers and loss, checkpoint loading, SyntheticIKFrames, the C-ABI argument
checks of pn2x_iknet_forward, and the unchanged hand_IKNet path when no IKNet checkpoint exists."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
G = np.load(os.path.join(ROOT, "tests", "golden", "iknet_reference.npz"))

from _iknet_cases import iknet_state, load_into  # noqa: E402
from models.iknet import IKNet, axisang2quat, gt_quat, quat2axisang  # noqa: E402

CASES = [(B, f, p) for B in (1, 3, 16) for f in ("kp", "camera") for p in ("zero", "shaped")]


def _net(frame="kp"):
    m = IKNet({"device": "cpu", "network": {"iknetframe": frame}})
    load_into(m)
    return m.eval()


def test_state_dict_matches_the_reference():
    sd = IKNet({"device": "cpu", "network": {"iknetframe": "kp"}}).state_dict()
    assert list(sd.keys()) == [str(k) for k in G["state_keys"]]
    for (k, v), shape in zip(sd.items(), G["state_shapes"]):
        assert list(v.shape) == [int(s) for s in shape if s], k


def test_reference_checkpoint_with_mano_buffers_loads(capsys):
    from hotrack_amd import ext  # noqa: F401  (nothing GPU: the import only binds the library)
    src = {k: torch.from_numpy(v) for k, v in iknet_state().items()}
    src["mano_layer_right.th_betas"] = torch.zeros(1, 10)
    src["mano_layer_right.th_v_template"] = torch.zeros(1, 778, 3)
    m = IKNet({"device": "cpu", "network": {}}, hand_model=torch.nn.Linear(1, 1))
    m.load_state_dict(src, strict=False)
    assert "ignored 2 mano_layer_right.*" in capsys.readouterr().out
    assert torch.equal(m.linear[3].weight, src["linear.3.weight"]) and torch.equal(m.bn[5].running_var, src["bn.5.running_var"])
    assert not any(k.startswith("hand_model") for k in m.state_dict())  # the hand model is never a submodule


@pytest.mark.parametrize("B,frame,palm", CASES, ids=[f"B{c[0]}_{c[1]}_{c[2]}" for c in CASES])
def test_torch_route_matches_the_reference(B, frame, palm):
    """fp32 on the CPU, same composition as the reference: equal to 1e-5 absolute (outputs are O(1); the measured difference is 0)."""
    m = _net(frame)
    key = f"B{B}_{frame}_{palm}"
    data = {"baseline_pred_kp": torch.from_numpy(G[f"B{B}_kp"]), "pred_palm_template": torch.from_numpy(G[f"palm_{palm}"])}
    with torch.no_grad():
        r = m(data, {"track_flag": True, "opt_flag": True})
    tol = dict(rtol=0, atol=1e-5)
    np.testing.assert_allclose(r["raw_quat"].numpy(), G[f"{key}_raw_quat"], **tol)
    np.testing.assert_allclose(r["MANO_theta"].numpy(), G[f"{key}_MANO_theta"], **tol)
    np.testing.assert_allclose(r["global_pose"]["rotation"].numpy(), G[f"{key}_R"], **tol)
    np.testing.assert_allclose(r["global_pose"]["translation"].numpy(), G[f"{key}_t"], **tol)
    np.testing.assert_allclose(r["init_kp_handframe"].numpy(), G[f"{key}_init_kp_handframe"], **tol)
    assert "pred_kp" not in r and float(r["global_pose"]["scale"]) == pytest.approx(0.2)


@pytest.mark.parametrize("B", [3, 16])
def test_training_forward_and_loss_match_the_reference(B):
    m = _net("kp")
    key = f"B{B}_kp_zero"
    palm = torch.from_numpy(G["palm_zero"]).expand(B, -1, -1)
    data = {"jittered_hand_kp": torch.from_numpy(G[f"B{B}_kp"]), "gt_hand_kp": torch.from_numpy(G[f"B{B}_gt_kp"]),
            "gt_hand_pose": {"palm_template": palm, "mano_pose": torch.from_numpy(G[f"B{B}_mano_pose"])}}
    with torch.no_grad():
        r = m(data, {"track_flag": False})
        loss, _ = m.compute_loss(data, r, {})
    np.testing.assert_allclose(r["gt_quat"].numpy(), G[f"{key}_gt_quat"], rtol=0, atol=1e-6)
    assert float(loss["quat_loss"]) == pytest.approx(float(G[f"{key}_quat_loss"]), abs=1e-6)
    assert float(loss["init_gt_kp_diff"]) == pytest.approx(float(G[f"{key}_init_gt_kp_diff"]), abs=1e-7)
    assert r["gt_kp_handframe"].shape == (B, 3, 21)
    # a (B, 45) pose code gives the same target as the (B, 48) one without its global block
    assert torch.equal(gt_quat(torch.from_numpy(G[f"B{B}_mano_pose"])[:, 3:]), r["gt_quat"])


def test_quaternion_helpers_match_the_reference():
    np.testing.assert_allclose(quat2axisang(torch.from_numpy(G["helper_quat"])).numpy(), G["helper_quat_axisang"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(axisang2quat(torch.from_numpy(G["helper_axisang"])).numpy(), G["helper_axisang_quat"], rtol=0, atol=1e-6)
    # no sign flip for w < 0: q = (-0.5, 0.5, 0.5, 0.5) is a 4 pi / 3 turn (not the equivalent 2 pi / 3 one)
    aa = quat2axisang(torch.tensor([[-0.5, 0.5, 0.5, 0.5]])).reshape(3)
    assert float(aa.norm()) == pytest.approx(4 * np.pi / 3, rel=1e-6)


def test_quaternion_conversion_returns_the_limit_where_the_reference_gives_nan():
    """Documented deviation: where 1 - w^2 < 0 after normalisation the reference's sqrt is NaN; here sin = 0 (axis = xyz,
    angle = 2 acos(clamp(w)))."""
    w = torch.tensor([1.0000001, 1.0, 0.99999994]).double()
    q = torch.stack([w, 1e-9 * torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                     torch.zeros(3, dtype=torch.float64)], -1)
    import models.iknet as ik
    orig = ik.EPS_Q
    try:
        ik.EPS_Q = -1e-7  # forces |w| / (|q| + eps) > 1 for the first rows: the reference's formula is NaN there
        ref_sin = torch.sqrt(1 - (q[:, 0] / (q.norm(dim=-1) + ik.EPS_Q)) ** 2)
        assert torch.isnan(ref_sin[0])
        aa = quat2axisang(q.reshape(1, -1)).reshape(3, 3)
    finally:
        ik.EPS_Q = orig
    assert torch.isfinite(aa).all()
    assert float(aa[0].abs().max()) < 1e-6  # the limit: a zero rotation


def test_synthetic_ik_frames_are_deterministic_and_posed_by_the_hand_model():
    from datasets.synthetic import SyntheticIKFrames
    from models.hand_model import SyntheticLBSHand
    for nb in (0, 10):
        hm = SyntheticLBSHand(num_betas=nb)
        ds = SyntheticIKFrames({"hand_model": hm, "hand_jitter_cfg": {"rand_scale": 0.01}}, 8, base_seed=3)
        a, b = ds[5], SyntheticIKFrames({"hand_model": hm, "hand_jitter_cfg": {"rand_scale": 0.01}}, 8, base_seed=3)[5]
        assert torch.equal(a["gt_hand_kp"], b["gt_hand_kp"]) and torch.equal(a["jittered_hand_kp"], b["jittered_hand_kp"])
        assert not torch.equal(ds[4]["gt_hand_kp"], a["gt_hand_kp"])
        pose = a["gt_hand_pose"]
        assert pose["mano_pose"].shape == (48,) and float(pose["mano_pose"][3:].abs().max()) <= 0.5
        shape = {"th_betas": pose["mano_beta"][None]} if nb else {}
        assert ("mano_beta" in pose) == (nb > 0)
        with torch.no_grad():
            _, kp = hm.forward(th_pose_coeffs=pose["mano_pose"][None], th_trans=a["gt_hand_kp"][:1] * 0 + 0, **shape)
        # the translation is not stored: the posed keypoints equal the model's up to one rigid offset of the wrist
        np.testing.assert_allclose((a["gt_hand_kp"] - kp[0] - (a["gt_hand_kp"][0] - kp[0, 0])).numpy(), 0, atol=1e-6)
        with torch.no_grad():
            _, rest = hm.forward(th_pose_coeffs=torch.zeros(1, 48), th_trans=torch.zeros(1, 3), **shape)
        assert torch.equal(pose["palm_template"], rest[0, [0, 1, 5, 9, 13, 17]])


def test_iknet_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.pn2x_iknet_supported.argtypes = [ci] * 5
    assert lib.pn2x_iknet_supported(1, 126, 1024, 6, 60) == 1 and lib.pn2x_iknet_supported(16, 126, 1024, 6, 60) == 1
    assert lib.pn2x_iknet_supported(17, 126, 1024, 6, 60) == 0 and lib.pn2x_iknet_supported(0, 126, 1024, 6, 60) == 0
    assert lib.pn2x_iknet_supported(4, 128, 1024, 6, 60) == 0 and lib.pn2x_iknet_supported(4, 126, 512, 6, 60) == 0
    assert lib.pn2x_iknet_supported(4, 126, 1024, 5, 60) == 0 and lib.pn2x_iknet_supported(4, 126, 1024, 6, 48) == 0
    lib.pn2x_iknet_work_floats.restype = ctypes.c_long
    assert lib.pn2x_iknet_work_floats() == 2 * 16 * 1024
    lib.pn2x_iknet_forward.argtypes = [ci, ci] + [vp] * 14
    f = lib.pn2x_iknet_forward
    a = 4096  # 16-byte aligned, never dereferenced: every call below is rejected before any launch
    ok = [a] * 13
    assert f(0, 0, *ok, None) == -1                      # m < 1
    assert f(17, 0, *ok, None) == -3                     # m beyond 16
    assert f(4, 2, *ok, None) == -1                      # no such frame
    assert f(4, 0, None, *ok[1:], None) == -2            # NULL keypoints
    assert f(4, 0, a, None, a, *ok[3:], None) == -2      # NULL R in the 'kp' frame
    assert f(4, 0, *ok[:9], None, *ok[10:], None) == -2  # NULL work
    assert f(4, 0, *ok[:12], None, None) == -2           # NULL theta
    assert f(4, 0, *ok[:3], a + 4, *ok[4:], None) == -1  # misaligned w1
    assert f(4, 0, *ok[:9], a + 8, *ok[10:], None) == -1  # misaligned work


def test_hand_iknet_without_a_checkpoint_is_unchanged(tmp_path, monkeypatch, capsys):
    """handopt_test_HO3D.yml names IKNet_dir; with no checkpoint there the Trainer builds today's model and logs today's lines."""
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from configs.config import get_config
    from parse_args import add_args
    from trainer import Trainer
    p = add_args(argparse.ArgumentParser())
    for hm in (None, "synthetic"):
        args = ["--config", "handopt_test_HO3D.yml"] + (["--hand_model", hm] if hm else [])
        cfg = get_config(p.parse_args(args), save=False)
        tr = Trainer(cfg)
        tr.resume()
        out = capsys.readouterr().out
        assert "use_iknet" not in cfg and "IKNet" not in out.replace("track=hand_IKNet", "").replace("IKNet's initial pose", "") \
            .replace("IKNet / MANO assets", "")
        assert tr.model.IKnet is None and not any(k.startswith("IKnet.") for k in tr.model.state_dict())
        want = ("hand-pose particle optimisation (hand model: SyntheticLBSHand; IKNet's initial pose from the previous frame + a rigid "
                "keypoint fit)" if hm else "no hand model (IKNet / MANO assets are not available) -> HandTrackNet tracking branch only")
        assert want in out and "No HandTrackNet checkpoint found" in out
