"""GPU: opt.fuse_depth of ObjTrackModel_Optimization (network/models/shape_fusion.py, hotrack_amd/csrc/tsdf_fuse.hip): one synthetic
--from_depth object sequence of 12 frames whose handed-over volume describes a capsule of radius 0.03 while the depth frames show
the true one (0.04); a 101^3 volume at stride 0.004, a flush every 4 frames."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu
RES, STRIDE, N, FRAMES = 101, 0.004, 1024, 12
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


def _cfg(on, from_depth=True):
    return {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"},
            "opt": {"updateobjshape": False, "fuse_depth": on, "fuse_every": 4}, "num_points": N, "obj_category": ["bottle"],
            "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "from_depth": from_depth}


def _model(on):
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    model = ObjTrackModel_Optimization(_cfg(on))
    model.optimizer = gf_optimize_obj(_cfg(on), seed=7)
    model.optimizer.volume_size = RES
    return model


@pytest.fixture(scope="module")
def sequence():
    from datasets.synthetic import SyntheticObjectSequences
    return SyntheticObjectSequences(_cfg(False), 1, FRAMES, res=RES, stride=STRIDE, from_depth=True, model_radius=0.03)[0]


@pytest.fixture(scope="module")
def tracked(sequence):
    out = {}
    with torch.no_grad():
        for on in (True, False):
            seq = copy.deepcopy(sequence)
            handed = seq[0]["sdf_volume"]
            before = handed.clone()
            out[on] = (_model(on)(seq, dict(FLAGS)), handed, before, seq)
    return out


def _surface_residual(volume, points):
    from hotrack_amd import sdf
    dev = torch.device("cuda", 0)
    return float(sdf.distance(points.to(dev).float().contiguous(), volume.to(dev).contiguous(), STRIDE).abs().mean())


def test_fused_volume_is_returned_and_fits_the_true_surface_better(tracked):
    rets, handed, before, seq = tracked[True]
    assert len(rets) == FRAMES
    assert torch.equal(handed, before)   # the handed-over tensor is never written
    fused = rets[0]["obj_fused"]
    assert fused["frames"] == FRAMES and fused["volume"].shape == (RES, RES, RES) and fused["weight"].shape == (RES, RES, RES)
    assert fused["volume"].is_cuda and fused["volume"].dtype == handed.dtype and fused["weight"].dtype == torch.float32
    assert fused["volume"].data_ptr() != handed.data_ptr()
    assert not torch.equal(fused["volume"].cpu(), before)
    assert float(fused["weight"].min()) == 8.0 and float(fused["weight"].max()) > 8.0   # the prior weight, and what was seen
    prior_fit = _surface_residual(before, seq[0]["obj_model_points"])
    fused_fit = _surface_residual(fused["volume"], seq[0]["obj_model_points"])
    print("mean |V| at obj_model_points: prior %.4e, fused %.4e" % (prior_fit, fused_fit))
    assert 0.009 < prior_fit < 0.011 and fused_fit < prior_fit


def test_switch_off_changes_nothing(tracked):
    rets, handed, before, _ = tracked[False]
    assert len(rets) == FRAMES and "obj_fused" not in rets[0] and torch.equal(handed, before)
    # frames 0 .. 3 precede the first flush: the same volume, the same poses, bit for bit
    on = tracked[True][0]
    for a, b in zip(rets[:4], on[:4]):
        assert torch.equal(a["rotation"], b["rotation"]) and torch.equal(a["translation"], b["translation"])
    assert any(not torch.equal(a["translation"], b["translation"]) for a, b in zip(rets[4:], on[4:]))   # then the volume differs


def test_extracted_mesh_is_the_fused_volumes(sequence):
    from models import mesh_sdf
    model = _model(True)
    model.extract_mesh = True
    with torch.no_grad():
        rets = model(copy.deepcopy(sequence), dict(FLAGS))
    want_v, want_f = mesh_sdf.volume_to_mesh(rets[0]["obj_fused"]["volume"], STRIDE, 0.0)
    got = rets[0]["obj_info"]["recon_mesh"]
    assert want_f.shape[0] > 0 and torch.equal(got["vertices"], want_v) and torch.equal(got["faces"], want_f)


def test_forward_batch_refuses_the_switch(sequence):
    with pytest.raises(ValueError, match="fuse_depth"):
        _model(True).forward_batch([copy.deepcopy(sequence)], dict(FLAGS))


def test_a_sequence_without_depth_frames_names_the_missing_keys():
    from datasets.synthetic import SyntheticObjectSequences
    seq = SyntheticObjectSequences(_cfg(False, False), 1, 2, res=RES, stride=STRIDE)[0]
    with pytest.raises(KeyError) as err:
        _model(True)(seq, dict(FLAGS))
    assert all(k in str(err.value) for k in ("depth", "seg", "intrinsics"))
