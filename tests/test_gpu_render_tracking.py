"""GPU: opt.render_model of ObjTrackModel_Optimization (network/models/volume_render.py, hotrack_amd/csrc/sdf_raycast.hip) on synthetic
--from_depth object sequences of 12 frames, a 101^3 volume at stride 0.004: the tracked poses do not depend on the switch, the three
columns are reported, a too-thin handed-over model shows in them, and lockstep groups report what single sequences do."""
import copy
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu
RES, STRIDE, N, FRAMES = 101, 0.004, 1024, 12
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}
COLUMNS = ("model_depth_residual(mm)", "model_silhouette_iou", "model_occluded_ratio")


def _cfg(on, from_depth=True):
    return {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False, "render_model": on},
            "num_points": N, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "from_depth": from_depth}


def _model(on):
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    model = ObjTrackModel_Optimization(_cfg(on))
    model.optimizer = gf_optimize_obj(_cfg(on), seed=7)
    model.optimizer.volume_size = RES
    return model


@pytest.fixture(scope="module")
def sequences():
    from datasets.synthetic import SyntheticObjectSequences
    true = SyntheticObjectSequences(_cfg(False), 2, FRAMES, res=RES, stride=STRIDE, from_depth=True)
    thin = SyntheticObjectSequences(_cfg(False), 1, FRAMES, res=RES, stride=STRIDE, from_depth=True, model_radius=0.03)
    return {"true": [true[0], true[1]], "thin": thin[0]}


def _track(on, seq):
    model = _model(on)
    seq = copy.deepcopy(seq)
    with torch.no_grad():
        rets = model(seq, dict(FLAGS))
        return rets, model.compute_loss(seq, rets, dict(FLAGS))[0]


@pytest.fixture(scope="module")
def tracked(sequences):
    return {(on, k): _track(on, sequences["true"][k]) for on, k in ((True, 0), (False, 0), (True, 1))}


def test_poses_do_not_depend_on_the_switch(tracked):
    on, off = tracked[(True, 0)][0], tracked[(False, 0)][0]
    assert len(on) == FRAMES == len(off) and "obj_render" in on[0] and "obj_render" not in off[0]
    for a, b in zip(on, off):
        assert torch.equal(a["rotation"], b["rotation"]) and torch.equal(a["translation"], b["translation"])
    assert not any(c in tracked[(False, 0)][1] for c in COLUMNS)


def test_columns_and_maps(tracked):
    rets, loss = tracked[(True, 0)]
    out = rets[0]["obj_render"]
    assert out["depth"].shape == (FRAMES, 480, 640) and out["normal"].shape == (FRAMES, 480, 640, 3) and out["stats"].shape == (FRAMES, 4)
    assert out["depth"].is_cuda and int(out["skipped"]) == 0
    print({c: loss[c] for c in COLUMNS})
    assert all(c in loss and math.isfinite(loss[c]) for c in COLUMNS)
    assert 0 < loss["model_depth_residual(mm)"] < 50 and 0.5 < loss["model_silhouette_iou"] <= 1 and 0 <= loss["model_occluded_ratio"] < 0.5
    assert "obs_surface_residual(mm)" not in loss and "rdiff_0" in loss   # next to the existing columns, which stay


def test_a_too_thin_model_shows_in_the_residual(tracked, sequences):
    thin = _track(True, sequences["thin"])[1]
    true = tracked[(True, 0)][1]
    print("residual (mm): true radius %.3f, radius 0.03 %.3f; IoU %.3f, %.3f" % (true[COLUMNS[0]], thin[COLUMNS[0]], true[COLUMNS[1]], thin[COLUMNS[1]]))
    assert thin["model_depth_residual(mm)"] > true["model_depth_residual(mm)"]


def test_forward_batch_reports_the_same_columns(tracked, sequences):
    model = _model(True)
    seqs = [copy.deepcopy(s) for s in sequences["true"]]
    with torch.no_grad():
        rets = model.forward_batch(seqs, dict(FLAGS))
        for k in range(2):
            loss = model.compute_loss(seqs[k], rets[k], dict(FLAGS))[0]
            want_rets, want = tracked[(True, k)]
            assert torch.equal(rets[k][0]["obj_render"]["depth"], want_rets[0]["obj_render"]["depth"])
            assert torch.equal(rets[k][0]["obj_render"]["stats"], want_rets[0]["obj_render"]["stats"])
            assert all(loss[c] == want[c] for c in COLUMNS), (k, loss, want)


def test_a_sequence_without_depth_frames_names_the_missing_keys():
    from datasets.synthetic import SyntheticObjectSequences
    seq = SyntheticObjectSequences(_cfg(False, False), 1, 2, res=RES, stride=STRIDE)[0]
    with pytest.raises(KeyError) as err:
        _model(True)(seq, dict(FLAGS))
    assert "render_model" in str(err.value) and all(k in str(err.value) for k in ("depth", "seg", "intrinsics"))


def test_save_writes_the_last_frames_maps(sequences, tmp_path):
    model = _model(True)
    model.save_folder = str(tmp_path)
    seq = copy.deepcopy(sequences["true"][0][:2])
    with torch.no_grad():
        rets = model(seq, dict(FLAGS, save_flag=True))
    paths = rets[0]["obj_render"]["paths"]
    assert [os.path.basename(p) for p in paths] == ["synthetic_obj_000_model_depth.png", "synthetic_obj_000_model_normal.png"]
    assert all(open(p, "rb").read(8) == b"\x89PNG\r\n\x1a\n" for p in paths)
