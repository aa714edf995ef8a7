"""GPU: several object sequences tracked in lockstep (ObjTrackModel_Optimization.forward_batch, Trainer.test_batch) against
the same sequences tracked one at a time by `forward` on a fresh model with the same particles: the same bits per sequence and
frame, the same compute_loss columns, one lookup volume per distinct volume tensor.  Small: a 41^3 volume, 256 points, 3-5
frames."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu
RES, STRIDE = 41, 0.01
LENGTHS = (3, 5, 4)
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


def _cfg():
    return {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False},
            "num_points": 256, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt"}


def _sequences():
    """Three sequences of different lengths: two hand over the SAME volume tensor, the third the capsule as a triangle mesh."""
    from datasets.synthetic import SyntheticObjectSequences
    cfg = _cfg()
    vol = SyntheticObjectSequences(cfg, 3, max(LENGTHS), res=RES, stride=STRIDE)
    mesh = SyntheticObjectSequences(cfg, 3, max(LENGTHS), res=RES, stride=STRIDE, obj_as_mesh=True)
    seqs = [vol[0][:LENGTHS[0]], mesh[1][:LENGTHS[1]], vol[2][:LENGTHS[2]]]
    assert seqs[0][0]["sdf_volume"] is seqs[2][0]["sdf_volume"] and "obj_mesh" in seqs[1][0]
    return seqs


def _model():
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    cfg = _cfg()
    model = ObjTrackModel_Optimization(cfg)
    model.optimizer = gf_optimize_obj(cfg, seed=7)   # the same particles in every model of this file
    model.optimizer.volume_size = RES                # (the size a mesh is voxelised at: the generator's small volume)
    return model


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


@pytest.fixture(scope="module")
def tracked():
    seqs = _sequences()
    one_by_one, losses = [], []
    with torch.no_grad():
        model = _model()                             # a fresh model, the sequences in the loader's order
        for seq in copy.deepcopy(seqs):
            rets = model(seq, dict(FLAGS))
            one_by_one.append(rets)
            losses.append(model.compute_loss(seq, rets, dict(FLAGS))[0])
    return seqs, one_by_one, losses


def test_forward_batch_returns_forwards_bits(tracked):
    seqs, one_by_one, losses = tracked
    seqs = copy.deepcopy(seqs)
    model = _model()
    with torch.no_grad():
        rets = model.forward_batch(seqs, dict(FLAGS))
    assert [len(r) for r in rets] == list(LENGTHS)
    for s, (got, ref) in enumerate(zip(rets, one_by_one)):
        for k, (a, b) in enumerate(zip(got, ref)):
            assert a["rotation"].shape == (1, 3, 3) and a["translation"].shape == (1, 3, 1)
            assert np.array_equal(_bits(a["rotation"]), _bits(b["rotation"])), f"sequence {s} frame {k}"
            assert np.array_equal(_bits(a["translation"]), _bits(b["translation"])), f"sequence {s} frame {k}"
        # the hand-off `forward` writes back into the frames: one pose dict per sequence, holding the last two poses
        assert seqs[s][-1]["jittered_obj_pose"] is seqs[s][1]["jittered_obj_pose"]
        assert torch.equal(seqs[s][1]["jittered_obj_pose"]["prev_rotation"], got[-2]["rotation"])
        assert torch.equal(seqs[s][1]["jittered_obj_pose"]["translation"], got[-1]["translation"])
    with torch.no_grad():
        for s, seq in enumerate(seqs):
            loss = model.compute_loss(seq, rets[s], dict(FLAGS))[0]
            assert loss.keys() == losses[s].keys()
            for k in loss:
                assert float(loss[k]) == float(losses[s][k]), (s, k)
    assert max(l["obj_pred_t_diff"] for l in losses) < 0.02   # (the trackers stay on the object: the comparison is not of garbage)


def test_sequences_sharing_a_volume_share_its_lookup_copy():
    seqs = copy.deepcopy(_sequences())
    seqs[2][0]["sdf_volume"] = seqs[0][0]["sdf_volume"]   # (deepcopy keeps the sharing; stated, because the test is about it)
    model = _model()
    built = {}
    got = [model._sequence_volume(seq[0], built) for seq in seqs]
    assert got[0][0] is got[2][0] and got[1][0] is not got[0][0]
    assert len(built) == 2 and all(abs(s - STRIDE) < 1e-12 for _, s in got)
    assert all(v.res == RES for v, _ in got)


def test_trainer_test_batch_equals_test_per_sequence(tracked, tmp_path):
    from trainer import Trainer
    seqs, one_by_one, losses = tracked
    cfg = dict(_cfg(), experiment_dir=str(tmp_path), network={"type": "HandTrackNet"}, warm_up=0, total_epoch=1, weight_init="xavier",
               learning_rate=1e-3)
    trainer = Trainer(cfg)
    trainer.model = _model()
    results = trainer.test_batch(copy.deepcopy(seqs))
    assert len(results) == 3
    for s, (loss, rets) in enumerate(results):
        assert len(rets) == LENGTHS[s]
        assert np.array_equal(_bits(rets[-1]["rotation"]), _bits(one_by_one[s][-1]["rotation"]))
        assert {k: float(v) for k, v in loss.items()} == {k: float(v) for k, v in losses[s].items()}


def test_entry_point_prints_the_same_columns_with_seq_batch(tmp_path, monkeypatch, capsys):
    """network/test.py --config objopt_test_HO3D.yml with and without --seq_batch, the optimiser's particles drawn from the same
    numpy seed (the entry point draws them unseeded, as the reference does): bit-equal poses, so every `Test <column>` line agrees
    to its last printed digit; one Trajectory line per sequence either way."""
    import argparse
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    import test as test_entry
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    outs = []
    for extra in ([], ["--seq_batch", "4"]):     # (the synthetic test set has fewer than 4 sequences: a last, smaller group)
        a = p.parse_args(["--config", "objopt_test_HO3D.yml", *extra])
        a.synthetic_frames = 3
        np.random.seed(11)
        test_entry.main(a)
        outs.append(capsys.readouterr().out.splitlines())
    cols = [[l for l in out if l.startswith("Test ")] for out in outs]
    assert cols[0] and cols[0] == cols[1]
    traj = [[l.split(":")[0] for l in out if l.startswith("Trajectory ")] for out in outs]
    assert len(traj[0]) >= 2 and traj[0] == traj[1]
    assert any("group of" in l for l in outs[1]) and not any("group of" in l for l in outs[0])


def test_differing_voxel_scales_are_refused():
    seqs = copy.deepcopy(_sequences())
    seqs[2][0]["voxel_scale"] = 2 * STRIDE
    with pytest.raises(ValueError, match="voxel_scale"), torch.no_grad():
        _model().forward_batch(seqs, dict(FLAGS))
