"""CPU: the per-frame tracking rule of ObjTrackModel_Optimization is stated once (track_network._ObjSequence) and driven by both
`forward` and `forward_batch`.  A stub stands in for gf_optimize_obj: its poses are a fixed function of the cloud and the pose it
is handed, and it records every call, so what the two methods feed the optimiser and what they make of its answers can be compared
exactly, without a GPU.  Sequences: SyntheticObjectSequences at 64 points and a 41^3 volume, of 3, 1 and 0 frames; the first two
hand over the same volume tensor.  (`forward` has no answer for a sequence without frames -- it reads the first frame's volume --
so the empty one is tracked in the group only, where it must come back empty and disturb nobody.)  Surface accumulation and depth
fusion need the kernels and stay with their GPU tests."""
import copy
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

RES, STRIDE, N, LENGTHS = 41, 0.01, 64, (3, 1, 0)
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


def _moved(cloud, pose, turn, share):
    """The stub's pose rule: rotate about z by `turn` plus the cloud's mean x, translate by `share` of the cloud's mean."""
    mean = cloud.float().reshape(-1, 3).mean(dim=0)
    a = turn + float(mean[0])
    Rz = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return {"rotation": (Rz @ pose["rotation"].float().reshape(3, 3)).reshape(1, 3, 3),
            "translation": pose["translation"].float().reshape(1, 3, 1) + share * mean.reshape(1, 3, 1)}


class StubOptimizer:
    """What the tracker uses of gf_optimize_obj.  `calls` holds (entry, sequence, cloud, pose as handed over); `sequence` is the
    slot of a batched call, or `self.current` (set by the test) for a single one."""

    def __init__(self, cfg=None):
        self.device = torch.device("cpu")
        self.volume_size, self.voxel_scale, self.sdf_volume, self._corners = 201, 0.002, None, None
        self.calls, self.loads, self.forgets, self.current = [], 0, 0, None

    def load_volume(self, sdf_volume, voxel_scale=None):
        self.loads += 1
        self.volume_size = sdf_volume.shape[0]
        if voxel_scale is not None:
            self.voxel_scale = float(voxel_scale)
        self.sdf_volume = sdf_volume
        self._corners = SimpleNamespace(source=sdf_volume)

    def forget_volume_tables(self):
        self.forgets += 1

    def _note(self, entry, k, cloud, pose):
        self.calls.append((entry, k, cloud.clone(), {key: value.clone() for key, value in pose.items()}))

    def optimize(self, pcld, init_obj_pose, category=None, file_name=None, projection=None):
        self._note("optimize", self.current, pcld, init_obj_pose)
        return _moved(pcld, init_obj_pose, 0.05, 1.0)

    def refine(self, pcld, pose, route=None):
        self._note("refine", self.current, pcld, pose)
        return dict(_moved(pcld, pose, -0.02, 0.25), refine_stats=torch.arange(8.0) + pcld.float().sum())

    def optimize_batch(self, pclds, init_obj_poses, corner_volumes, voxel_scale=None):
        out = []
        for k, (cloud, pose, vol) in enumerate(zip(pclds, init_obj_poses, corner_volumes)):
            assert (cloud is None) == (vol is None)
            if cloud is None:
                out.append({"rotation": pose["rotation"], "translation": pose["translation"]})
            else:
                self._note("optimize", k, cloud, pose)
                out.append(_moved(cloud, pose, 0.05, 1.0))
        return out

    def refine_batch(self, pclds, poses, corner_volumes, voxel_scale=None):
        out = []
        for k, (cloud, pose) in enumerate(zip(pclds, poses)):
            if cloud is None:
                out.append(dict(pose, refine_stats=torch.zeros(8)))
            else:
                self._note("refine", k, cloud, pose)
                out.append(dict(_moved(cloud, pose, -0.02, 0.25), refine_stats=torch.arange(8.0) + cloud.float().sum()))
        return out


def _model(monkeypatch, **switches):
    from models import optimization_obj
    from models.track_network import ObjTrackModel_Optimization
    monkeypatch.setattr(optimization_obj, "gf_optimize_obj", StubOptimizer)
    model = ObjTrackModel_Optimization({"device": torch.device("cpu"), "data_cfg": {"dataset_name": "HO3D"}, "num_points": N,
                                        "obj_category": ["bottle"], "opt": dict(switches)})
    assert isinstance(model.optimizer, StubOptimizer)
    model.extract_mesh_route = "torch"
    return model


@pytest.fixture(scope="module")
def sequences():
    from datasets.synthetic import SyntheticObjectSequences
    data = SyntheticObjectSequences({"num_points": N, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}}, 3, max(LENGTHS),
                                    res=RES, stride=STRIDE)
    seqs = [data[k][:n] for k, n in enumerate(LENGTHS)]
    assert seqs[0][0]["sdf_volume"] is seqs[1][0]["sdf_volume"] and seqs[2] == []
    return seqs


def _same(a, b, where="ret"):
    """Exactly the same: types, keys and their order, tensors bit for bit."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for key in a:
            _same(a[key], b[key], f"{where}[{key!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a == b, where


def _track_both(monkeypatch, sequences, **switches):
    """-> (the group's sequences, its results, its stub; per sequence with frames: the single run's sequence, results, stub)."""
    group = _model(monkeypatch, **switches)
    group_seqs = copy.deepcopy(sequences)   # (one copy of the list: the two sequences go on sharing their volume tensor)
    with torch.no_grad():
        group_rets = group.forward_batch(group_seqs, dict(FLAGS))
    singles = {}
    for k, seq in enumerate(sequences):
        if len(seq):
            model, seq = _model(monkeypatch, **switches), copy.deepcopy(seq)
            model.optimizer.current = k
            with torch.no_grad():
                singles[k] = (seq, model(seq, dict(FLAGS)), model.optimizer)
    return group_seqs, group_rets, group.optimizer, singles


def _calls(stub, entry, k):
    return [(cloud, pose) for e, s, cloud, pose in stub.calls if e == entry and s == k]


@pytest.mark.parametrize("switches", [{}, {"refine_pose": True}, {"extract_mesh": True}, {"refine_pose": True, "extract_mesh": True}],
                         ids=["plain", "refine", "mesh", "refine+mesh"])
def test_a_group_gives_what_forward_gives_on_each_sequence_alone(monkeypatch, sequences, switches):
    group_seqs, group_rets, group_stub, singles = _track_both(monkeypatch, sequences, **switches)
    assert [len(r) for r in group_rets] == list(LENGTHS)
    extras = ["obj_refine"] * bool(switches.get("refine_pose")) + ["obj_info"] * bool(switches.get("extract_mesh"))
    for k, (seq, rets, stub) in singles.items():
        _same(group_rets[k], rets, f"sequence {k}")                                                       # (a)
        assert list(rets[0]) == ["rotation", "translation", *extras]
        for entry in ("optimize", "refine"):                                                               # (b)
            _same(_calls(group_stub, entry, k), _calls(stub, entry, k), f"{entry} calls of sequence {k}")
        assert len(_calls(stub, "optimize", k)) == LENGTHS[k]
        assert len(_calls(stub, "refine", k)) == (LENGTHS[k] if switches.get("refine_pose") else 0)
        for frames in (seq, group_seqs[k]):   # the hand-off written back into the frames: one pose dict from frame 1 on
            assert all(d["jittered_obj_pose"] is frames[1]["jittered_obj_pose"] for d in frames[2:])
    assert group_stub.loads == 1 and all(stub.loads == 1 for _, _, stub in singles.values())   # one volume tensor, loaded once
    assert group_stub.forgets == 0


@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
def test_a_frame_starts_from_the_frame_before(monkeypatch, sequences, refine):
    _, group_rets, group_stub, singles = _track_both(monkeypatch, sequences, refine_pose=refine)
    for rets, stub in ((group_rets[0], group_stub), (singles[0][1], singles[0][2])):
        starts = [pose for _, pose in _calls(stub, "optimize", 0)]
        assert len(starts) == 3 and all(p["rotation"].shape == (1, 3, 3) and p["translation"].shape == (1, 3, 1) for p in starts)
        for key in ("rotation", "translation"):                                                           # (c)
            assert torch.equal(starts[0]["prev_" + key], starts[0][key])
            assert torch.equal(starts[0][key], sequences[0][0]["jittered_obj_pose"][key].float().reshape(starts[0][key].shape))
            for t in (1, 2):
                assert torch.equal(starts[t][key], rets[t - 1][key])
                assert torch.equal(starts[t]["prev_" + key], starts[t - 1][key])
        if refine:                                                                                        # (d)
            assert rets[0]["obj_refine"].shape == (3, 8) and all("refine_stats" not in r for r in rets)
            searched = [pose for _, pose in _calls(stub, "refine", 0)]
            for t in range(3):   # the refinement starts from the search's result, and its own result is the frame's pose
                _same(searched[t], _moved(sequences[0][t]["obj_points"], starts[t], 0.05, 1.0))
                _same({key: rets[t][key] for key in ("rotation", "translation")}, _moved(sequences[0][t]["obj_points"], searched[t], -0.02, 0.25))
                assert torch.equal(rets[0]["obj_refine"][t], torch.arange(8.0) + sequences[0][t]["obj_points"].sum())
        else:
            assert "obj_refine" not in rets[0]
    assert group_rets[1][0]["obj_refine"].shape == (1, 8) if refine else "obj_refine" not in group_rets[1][0]


def test_sequences_sharing_a_volume_share_one_extraction(monkeypatch, sequences):
    from models import mesh_sdf
    extracted = []
    real = mesh_sdf.volume_to_mesh

    def counting(volume, *a, **k):
        extracted.append(volume)
        return real(volume, *a, **k)
    monkeypatch.setattr(mesh_sdf, "volume_to_mesh", counting)
    _, group_rets, _, singles = _track_both(monkeypatch, sequences, extract_mesh=True)                  # (e)
    assert len(extracted) == 1 + len(singles)   # the group: once for its two sequences; then once per single run
    meshes = [group_rets[k][0]["obj_info"]["recon_mesh"] for k in (0, 1)]
    assert meshes[0] is meshes[1] and meshes[0]["faces"].shape[0] > 0
    for k in (0, 1):
        assert group_rets[k][0]["obj_info"]["recon_path"] is None
        _same(singles[k][1][0]["obj_info"]["recon_mesh"], meshes[0])


@pytest.mark.parametrize("lacking", [(0, 0), (0, 2)], ids=["first frame", "a later frame"])
def test_a_frame_without_depth_is_refused_before_any_work(monkeypatch, sequences, lacking):
    k, t = lacking                                                                                        # (f)
    seqs = copy.deepcopy(sequences)
    for seq in seqs:   # what opt.render_model reads, on every frame but one
        for i, data in enumerate(seq):
            data.update(depth=torch.zeros(4, 4), seg=torch.zeros(4, 4, 3, dtype=torch.uint8), intrinsics=[1.0, 1.0, 2.0, 2.0])
    del seqs[k][t]["depth"]
    for run in ("forward", "forward_batch"):
        model = _model(monkeypatch, render_model=True)
        with pytest.raises(KeyError) as err:
            model(copy.deepcopy(seqs[k]), dict(FLAGS)) if run == "forward" else model.forward_batch(copy.deepcopy(seqs), dict(FLAGS))
        text = str(err.value)
        assert "opt.render_model" in text and "--from_depth" in text and f"frame {t}" in text and "lacks ['depth']" in text
        assert seqs[k][t]["file_name"][0] in text and ("sequence 0" in text) == (run == "forward_batch")
        assert model.optimizer.calls == [] and model.optimizer.loads == 0


def test_a_tracker_with_its_switches_deleted_reads_their_defaults(monkeypatch, sequences):
    model = _model(monkeypatch, refine_pose=True, extract_mesh=True)
    for name in ("refine_pose", "refine_route", "extract_mesh", "extract_mesh_route", "render_model", "render_route", "render_occl_margin",
                 "fuse_depth", "fuse_route", "lockstep_fuse", "save_folder"):
        delattr(model, name)
    model.optimizer.current = 0
    with torch.no_grad():
        rets = model(copy.deepcopy(sequences[0]), dict(FLAGS))
        group = model.forward_batch(copy.deepcopy(sequences), dict(FLAGS))
    assert all(list(r) == ["rotation", "translation"] for r in rets) and not _calls(model.optimizer, "refine", 0)
    _same(group[0], rets)
