"""CPU: the hand model's skinning tables (HandModel.skinning_tables, lbs_forward_from_tables) and the switch of the hand-pose
optimiser's device-resident route (gf_optimize_hand_pose.fused / use_kernel, opt.fused_pose, --fused_hand_pose)."""
import argparse
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from models.hand_model import SyntheticLBSHand, lbs_forward_from_tables  # noqa: E402
from models.optimization_hand import gf_optimize_hand_pose  # noqa: E402


@pytest.mark.parametrize("num_betas", [0, 10])
def test_synthetic_hand_has_tables_that_reproduce_forward(num_betas):
    hm = SyntheticLBSHand(num_betas=num_betas)
    t = hm.skinning_tables()
    assert t is not None and hm.skinning_tables() is t   # built and checked once
    assert t["parents"].numel() == 21 and t["skin_idx"].shape == (778, 2) and t["comps"].shape == (45, 45)
    assert ("shape_joints" in t) == (num_betas > 0)
    assert sorted(int(b) for b in t["pose_block"] if b >= 0) == list(range(15)) and int(t["pose_block"][0]) == -1
    g = torch.Generator().manual_seed(7)
    pose = torch.cat([torch.randn(5, 3, generator=g, dtype=torch.float64),
                      (torch.rand(5, 45, generator=g, dtype=torch.float64) * 2 - 1) * 1.5], dim=1)
    trans = torch.randn(5, 3, generator=g, dtype=torch.float64)
    beta = torch.randn(5, num_betas, generator=g, dtype=torch.float64) * 2 if num_betas else None
    want = hm(th_pose_coeffs=pose, th_trans=trans, th_betas=beta)
    got = lbs_forward_from_tables(t, pose, trans, beta)
    for a, b in zip(want, got):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-9
    v32, k32 = lbs_forward_from_tables(t, pose.float(), trans.float(), None if beta is None else beta.float())
    assert v32.dtype == torch.float32 and float((v32.double() - want[0]).abs().max()) < 1e-5


def test_a_pose_corrective_term_disqualifies_the_tables():
    class CorrectiveHand(SyntheticLBSHand):
        """A stand-in for a MANO layer with pose blend shapes: vertices move with the joint angles beyond skinning."""

        def forward(self, th_pose_coeffs, **kw):
            verts, joints = super().forward(th_pose_coeffs, **kw)
            return verts + 1e-3 * torch.sin(th_pose_coeffs[:, 3:6])[:, None, :], joints

    assert CorrectiveHand().skinning_tables() is None
    opt = gf_optimize_hand_pose({"device": "cpu", "opt": {"fused_pose": True}}, hand_model=CorrectiveHand(), particle_size=8)
    assert opt.use_kernel() is False


def test_tips_follow_the_optimisers_contact_zone_order():
    hm = SyntheticLBSHand()
    opt = gf_optimize_hand_pose({"device": "cpu"}, hand_model=hm, particle_size=8)
    t = hm.skinning_tables()
    assert t["tips"].tolist() == opt.tips_region
    offs = t["finger_offsets"].tolist()
    assert [list(range(offs[i], offs[i + 1])) for i in range(5)] == opt.finger_mask


def test_the_switch_defaults_to_off():
    opt = gf_optimize_hand_pose({"device": "cpu"}, hand_model=SyntheticLBSHand(), particle_size=8)
    assert opt.fused is False and opt.use_kernel() is False
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    assert getattr(p.parse_args([]), "opt/fused_pose") is None
    assert getattr(p.parse_args(["--fused_hand_pose"]), "opt/fused_pose") is True


def test_config_carries_the_switch(tmp_path, monkeypatch):
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    from configs.config import get_config
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    off = get_config(p.parse_args(["--config", "handopt_test_HO3D.yml"]), save=False)
    assert off["opt"]["fused_pose"] is False and off["opt"]["energy_weight"]["vis_regu_loss"] == 10
    on = get_config(p.parse_args(["--config", "handopt_test_HO3D.yml", "--fused_hand_pose"]), save=False)
    assert on["opt"]["fused_pose"] is True


def test_fused_on_a_cpu_device_runs_the_torch_route_and_says_why_once(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_hand_opt as base
    g, opt, proj, obj_pose, mask = base._setup("cpu")
    opt.fused = True
    with torch.no_grad():
        mano, pose, kp0, last, vis = base._frame_inputs(g, 0, "cpu")
        kp, theta, R, t = opt.optimize(mano, pose, kp0, last, vis, obj_pose, None, proj, mask)
        assert opt.use_kernel() is False
    out = capsys.readouterr().out
    assert out.count("fused_pose is set but the torch route runs") == 1 and "cpu" in out
    assert float((kp - torch.from_numpy(g["f0_final_kp"])).abs().max()) <= 2e-6   # the torch route's numbers
