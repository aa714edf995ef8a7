"""GPU: several hand sequences tracked in lockstep (HandTrackModel.forward_batch, Trainer.test_batch) against the same
sequences tracked one at a time by `forward`, each on a tracker in its fresh state: the same bits per sequence and frame.  The
hand is the shaped synthetic one (`--hand_model synthetic_shaped`) with shape estimation (use_pred_hand_shape) and the
device-resident pose optimiser (opt.fused_pose) on; HandTrackNet is replaced by an oracle whose noise depends on the frame alone.
Small: a 41^3 volume, 512 points, 256 candidates, sequences of 4, 3 and 2 frames, two distinct objects."""
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


def _cfg(fused, hm):
    return {"device": torch.device("cuda", 0), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
            "use_optimization": True, "use_pred_hand_shape": 1, "hand_particles": 256, "shape_particles": 256, "hand_model": hm,
            "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": fused}}


def _model(fused):
    from models.hand_model import SyntheticLBSHand
    from models.track_network import HandTrackModel
    hm = SyntheticLBSHand(num_betas=10)
    model = HandTrackModel(_cfg(fused, hm), handnet=OracleNet, hand_model=hm).eval()
    assert model.optimizer.use_kernel() == fused and model.opt_shape is not None and model.opt_shape.use_kernel()
    model.use_graph = False
    return model


def _sequences():
    """Three sequences (4, 3, 2 frames) of hands with their own shapes; 0 and 2 hand over ONE volume tensor, 1 a fatter object."""
    from datasets.synthetic import SyntheticHandObjectSequences
    from models.hand_model import SyntheticLBSHand
    cfg = _cfg(True, SyntheticLBSHand(num_betas=10))
    ds = SyntheticHandObjectSequences(cfg, 3, max(LENGTHS), res=41, stride=0.01, hand_beta=1.0)
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


def _max_diff(got, ref):
    d = 0.0
    for a_seq, b_seq in zip(got, ref):
        for a, b in zip(a_seq, b_seq):
            for x, y in [(a[f], b[f]) for f in FIELDS] + [(a["global_pose"][f], b["global_pose"][f]) for f in ("rotation", "translation")]:
                d = max(d, float((x.double() - y.double()).abs().max()))
    return d


def _one_by_one(fused):
    seqs = _sequences()
    rets, losses = [], []
    with torch.no_grad():
        for seq in copy.deepcopy(seqs):
            model = _model(fused)   # a tracker in its fresh state per sequence
            r = model(seq, dict(FLAGS))
            rets.append(r)
            losses.append(model.compute_loss(seq, r, dict(FLAGS))[0])
    return seqs, rets, losses


@pytest.fixture(scope="module")
def tracked():
    return _one_by_one(True)


def test_forward_batch_returns_forwards_bits(tracked):
    seqs, ref, _ = tracked
    seqs = copy.deepcopy(seqs)
    model = _model(True)
    with torch.no_grad():
        got = model.forward_batch(seqs, dict(FLAGS))
    _assert_same(got, ref, "forward_batch")
    # (the comparison is not of three copies of one track, nor of an optimiser that stands still)
    assert not torch.equal(ref[0][0]["pred_beta"], ref[1][0]["pred_beta"])
    assert not torch.equal(ref[0][1]["MANO_theta"], ref[2][1]["MANO_theta"])
    assert all(torch.isfinite(r["pred_kp"]).all() for seq in got for r in seq)
    assert seqs[0][1]["pred_beta"] is got[0][1]["pred_beta"]   # what forward() writes back into the frames


def test_trainer_test_batch_equals_test_per_sequence(tracked, tmp_path):
    from trainer import Trainer
    seqs, ref, losses = tracked
    cfg = {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False}, "num_points": 256,
           "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "experiment_dir": str(tmp_path),
           "network": {"type": "HandTrackNet"}, "warm_up": 0, "total_epoch": 1, "weight_init": "xavier", "learning_rate": 1e-3}
    trainer = Trainer(cfg)
    trainer.model = _model(True)   # (the trainer's plumbing around a hand tracker with the oracle network)
    results = trainer.test_batch(copy.deepcopy(seqs))
    assert len(results) == 3
    _assert_same([r for _, r in results], ref, "test_batch")
    for s, (loss, _) in enumerate(results):
        assert {k: float(v) for k, v in loss.items()} == {k: float(v) for k, v in losses[s].items()}


def test_forward_batch_with_the_fused_route_off():
    """The torch route: forward_batch runs optimize() per entry.  The lockstep result is held to the torch route's own
    run-to-run equality: it may differ from one-by-one tracking by no more than two one-by-one runs differ from each other
    (nothing, where that route is deterministic)."""
    seqs, ref, _ = _one_by_one(False)
    _, again, _ = _one_by_one(False)
    own = _max_diff(again, ref)
    model = _model(False)
    with torch.no_grad():
        got = model.forward_batch(copy.deepcopy(seqs), dict(FLAGS))
    assert [len(r) for r in got] == list(LENGTHS)
    d = _max_diff(got, ref)
    print(f"torch route: run to run {own:.3e}, forward_batch against forward {d:.3e}")
    assert d <= own
