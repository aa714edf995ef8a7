"""GPU: opt.fuse_depth inside lockstep groups (opt.lockstep_fuse; ObjTrackModel_Optimization.forward_batch,
network/models/shape_fusion.VolumeFusionGroup, hotrack_amd.sdf.tsdf_integrate_batch): three synthetic --from_depth sequences of
12, 7 and 5 frames that hand over ONE volume tensor (101^3, stride 0.004, a capsule of radius 0.03 where the frames show 0.04),
a flush every 4 frames -- so one sequence ends in the middle of a cadence and one a frame after a flush."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu
RES, STRIDE, N, LENGTHS = 101, 0.004, 1024, (12, 7, 5)
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


def _cfg(fuse, lockstep):
    return {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"},
            "opt": {"updateobjshape": False, "fuse_depth": fuse, "fuse_every": 4, "lockstep_fuse": lockstep}, "num_points": N,
            "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "from_depth": True}


def _model(fuse, lockstep, mesh=False):
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    model = ObjTrackModel_Optimization(_cfg(fuse, lockstep))
    model.optimizer = gf_optimize_obj(_cfg(fuse, lockstep), seed=7)
    model.optimizer.volume_size = RES
    model.extract_mesh = mesh
    return model


@pytest.fixture(scope="module")
def sequences():
    from datasets.synthetic import SyntheticObjectSequences
    data = SyntheticObjectSequences(_cfg(False, False), len(LENGTHS), max(LENGTHS), res=RES, stride=STRIDE, from_depth=True, model_radius=0.03)
    seqs = [data[k][:n] for k, n in enumerate(LENGTHS)]
    assert all(s[0]["sdf_volume"] is seqs[0][0]["sdf_volume"] for s in seqs)
    return seqs


@pytest.fixture(scope="module")
def tracked(sequences):
    """forward_batch with both switches (and the mesh extraction) on the group, and forward on a copy of every sequence alone."""
    with torch.no_grad():
        group = copy.deepcopy(sequences)   # (one copy: the three still share the volume tensor)
        handed = group[0][0]["sdf_volume"]
        assert all(s[0]["sdf_volume"] is handed for s in group)
        before = handed.clone()
        batch = _model(True, True, mesh=True).forward_batch(group, dict(FLAGS))
        alone = [_model(True, False)(copy.deepcopy(seq), dict(FLAGS)) for seq in sequences]
    return batch, alone, handed, before


def test_every_sequence_is_bit_equal_to_forward_on_it_alone(tracked):
    batch, alone, _, _ = tracked
    for k, n in enumerate(LENGTHS):
        assert len(batch[k]) == len(alone[k]) == n
        for t, (a, b) in enumerate(zip(batch[k], alone[k])):
            assert torch.equal(a["rotation"], b["rotation"]) and torch.equal(a["translation"], b["translation"]), (k, t)
        got, want = batch[k][0]["obj_fused"], alone[k][0]["obj_fused"]
        assert got["frames"] == want["frames"] == n
        assert torch.equal(got["volume"], want["volume"]) and torch.equal(got["weight"], want["weight"]), k
        assert not torch.equal(got["volume"].cpu(), tracked[3])   # (something was fused)


def test_the_handed_over_tensor_is_untouched_and_every_sequence_owns_its_volume(tracked):
    batch, _, handed, before = tracked
    assert torch.equal(handed, before)
    vols = [batch[k][0]["obj_fused"]["volume"] for k in range(len(LENGTHS))]
    wts = [batch[k][0]["obj_fused"]["weight"] for k in range(len(LENGTHS))]
    assert len({v.data_ptr() for v in vols} | {handed.data_ptr()}) == len(LENGTHS) + 1 and len({w.data_ptr() for w in wts}) == len(LENGTHS)
    assert not torch.equal(vols[0], vols[1]) and not torch.equal(vols[1], vols[2])   # different frames were fused


def test_the_extracted_mesh_is_each_sequences_fused_volumes(tracked):
    from models import mesh_sdf
    batch = tracked[0]
    for k in range(len(LENGTHS)):
        want_v, want_f = mesh_sdf.volume_to_mesh(batch[k][0]["obj_fused"]["volume"], STRIDE, 0.0)
        got = batch[k][0]["obj_info"]["recon_mesh"]
        assert want_f.shape[0] > 0 and torch.equal(got["vertices"], want_v) and torch.equal(got["faces"], want_f), k


def test_lockstep_fuse_alone_changes_nothing(sequences):
    with torch.no_grad():
        on = _model(False, True).forward_batch(copy.deepcopy(sequences), dict(FLAGS))
        off = _model(False, False).forward_batch(copy.deepcopy(sequences), dict(FLAGS))
    for k, n in enumerate(LENGTHS):
        assert len(on[k]) == len(off[k]) == n and "obj_fused" not in on[k][0]
        for a, b in zip(on[k], off[k]):
            assert torch.equal(a["rotation"], b["rotation"]) and torch.equal(a["translation"], b["translation"])


def test_fuse_depth_alone_is_still_refused_and_names_the_new_switch(sequences):
    with pytest.raises(ValueError, match="fuse_depth") as err:
        _model(True, False).forward_batch(copy.deepcopy(sequences[2:]), dict(FLAGS))
    assert "lockstep_fuse" in str(err.value)


def test_missing_keys_are_reported_before_any_work(sequences):
    group = copy.deepcopy(sequences[1:])
    del group[1][3]["seg"], group[1][3]["intrinsics"]
    with pytest.raises(KeyError) as err:
        _model(True, True).forward_batch(group, dict(FLAGS))
    assert all(s in str(err.value) for s in ("sequence 1", "frame 3", "seg", "intrinsics"))
    assert "obj_points" not in group[0][0]   # (the front end has not run)
