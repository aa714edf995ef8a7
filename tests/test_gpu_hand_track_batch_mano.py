"""GPU: several sequences of a MANO-structured hand tracked in lockstep (HandTrackModel.forward_batch, Trainer.test_batch with
opt.lockstep_mano) against the same sequences tracked one at a time by `forward`, each on a tracker in its fresh state: the same
bits per sequence and frame.  tests/test_gpu_hand_track_batch.py's set-up with SyntheticManoHand(num_verts=97) (the synthetic
sequences take it, and its shape space has the affine basis the shape-search kernel needs, so use_pred_hand_shape stays on):
the pose optimiser's per-step call is ONE ext.hand_pose_mano_opt_batch.  HandTrackNet is replaced by an oracle whose noise depends
on the frame alone.  Small: a 41^3 volume, 512 points, 256 candidates, sequences of 4, 3 and 2 frames, two distinct objects."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
LENGTHS = (4, 3, 2)
FIELDS = ("pred_kp", "MANO_theta", "pred_beta")
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


class OracleNet(torch.nn.Module):
    """Ground-truth keypoints plus 2 mm of noise seeded by the frame's name: the same in whatever order frames are visited."""

    def __init__(self, cfg):
        super().__init__()
        self.device = cfg["device"]

    def forward(self, data, flags):
        s, k = data["file_name"][0].split("_")[-1].split("/")
        g = torch.Generator(device="cuda").manual_seed(1000 * int(s) + int(k))
        kp = data["gt_hand_kp"].to(self.device) + 0.002 * torch.randn(1, 21, 3, device=self.device, generator=g)
        vis = torch.ones(1, 21, dtype=torch.bool, device=self.device)
        vis[0, [8, 20]] = int(k) % 2 == 0
        return {"pred_kp": kp, "pred_kp_vis_mask": vis}

    def compute_loss(self, data, ret, flags):
        return {"hand_pred_kp_diff": (ret["pred_kp"] - data["gt_hand_kp"].to(self.device)).norm(dim=-1).mean()}, ret


def _hand():
    from models.hand_model import SyntheticManoHand
    return SyntheticManoHand(num_verts=97)


def _cfg(hm, lockstep):
    return {"device": torch.device("cuda", 0), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
            "use_optimization": True, "use_pred_hand_shape": 1, "hand_particles": 256, "shape_particles": 256, "hand_model": hm,
            "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": True, "lockstep_mano": lockstep}}


def _model(lockstep):
    from models.track_network import HandTrackModel
    hm = _hand()
    model = HandTrackModel(_cfg(hm, lockstep), handnet=OracleNet, hand_model=hm).eval()
    opt = model.optimizer
    assert opt.use_kernel() and opt._kernel_model()["mano"] and opt.lockstep_mano == lockstep   # (the config key reaches the optimiser)
    assert model.opt_shape is not None and model.opt_shape.use_kernel()
    model.use_graph = False
    return model


def _sequences():
    """Three sequences (4, 3, 2 frames) of hands with their own shapes; 0 and 2 hand over ONE volume tensor, 1 a fatter object."""
    from datasets.synthetic import SyntheticHandObjectSequences
    ds = SyntheticHandObjectSequences(_cfg(_hand(), True), 3, max(LENGTHS), res=41, stride=0.01, hand_beta=1.0)
    seqs = [ds[s][:n] for s, n in enumerate(LENGTHS)]
    seqs[1][0]["sdf_volume"] = seqs[1][0]["sdf_volume"] + 0.004
    assert seqs[0][0]["sdf_volume"] is seqs[2][0]["sdf_volume"] and seqs[1][0]["sdf_volume"] is not seqs[0][0]["sdf_volume"]
    return seqs


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _assert_same(got, ref, what):
    assert [len(r) for r in got] == [len(r) for r in ref] == list(LENGTHS)
    for s, (a_seq, b_seq) in enumerate(zip(got, ref)):
        for k, (a, b) in enumerate(zip(a_seq, b_seq)):
            pairs = [(f, a[f], b[f]) for f in FIELDS] + [("global_pose." + f, a["global_pose"][f], b["global_pose"][f])
                                                         for f in ("rotation", "translation")]
            for name, x, y in pairs:
                assert x.shape == y.shape, (what, s, k, name)
                assert np.array_equal(_bits(x), _bits(y)), f"{what}: sequence {s} frame {k} {name}"


@pytest.fixture(scope="module")
def tracked():
    """Every sequence through `forward` on a tracker in its fresh state (the switch off: forward() does not read it)."""
    seqs = _sequences()
    rets, losses = [], []
    with torch.no_grad():
        for seq in copy.deepcopy(seqs):
            model = _model(False)
            r = model(seq, dict(FLAGS))
            rets.append(r)
            losses.append(model.compute_loss(seq, r, dict(FLAGS))[0])
    return seqs, rets, losses


def _profiled(fn):
    from hotrack_amd import pointnet2_hip
    pointnet2_hip.PROFILE = []
    try:
        out = fn()
        return out, [p[0] for p in pointnet2_hip.PROFILE]
    finally:
        pointnet2_hip.PROFILE = None


def test_forward_batch_returns_forwards_bits(tracked, capsys):
    seqs, ref, _ = tracked
    seqs = copy.deepcopy(seqs)
    model = _model(True)
    capsys.readouterr()
    with torch.no_grad():
        got, names = _profiled(lambda: model.forward_batch(seqs, dict(FLAGS)))
    assert "MANO entries" not in capsys.readouterr().out   # (the per-sequence fallback would say so)
    # one lockstep call per frame step, the sequence that ended sitting out; no single-problem optimiser call
    assert names.count("hand_pose_mano_opt_batch") == max(LENGTHS) and "hand_pose_opt" not in names
    _assert_same(got, ref, "forward_batch")
    # (the comparison is not of three copies of one track, nor of an optimiser that stands still)
    assert not torch.equal(ref[0][0]["pred_beta"], ref[1][0]["pred_beta"])
    assert not torch.equal(ref[0][1]["MANO_theta"], ref[2][1]["MANO_theta"])
    assert all(float(r[0]["MANO_theta"].abs().max()) > 0 for r in ref)   # (frame 0 starts from the zero pose code)
    assert all(torch.isfinite(r["pred_kp"]).all() for seq in got for r in seq)


def test_trainer_test_batch_equals_test_per_sequence(tracked, tmp_path):
    from trainer import Trainer
    seqs, ref, losses = tracked
    cfg = {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False}, "num_points": 256,
           "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "experiment_dir": str(tmp_path),
           "network": {"type": "HandTrackNet"}, "warm_up": 0, "total_epoch": 1, "weight_init": "xavier", "learning_rate": 1e-3}
    trainer = Trainer(cfg)
    trainer.model = _model(True)   # (the trainer's plumbing around a hand tracker with the oracle network)
    results, names = _profiled(lambda: trainer.test_batch(copy.deepcopy(seqs)))
    assert names.count("hand_pose_mano_opt_batch") == max(LENGTHS) and "hand_pose_opt" not in names
    assert len(results) == 3
    _assert_same([r for _, r in results], ref, "test_batch")
    for s, (loss, _) in enumerate(results):
        assert {k: float(v) for k, v in loss.items()} == {k: float(v) for k, v in losses[s].items()}
