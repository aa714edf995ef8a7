"""CPU: the torch route of the batched TSDF fusion (network/models/shape_fusion.py: tsdf_integrate_batch_torch, VolumeFusionGroup
with route='torch') over the groups of tests/_tsdf_batch_cases.py: bitwise the per-sequence torch route, inside the float64 check
with its cap; the group's refusals; the --lockstep_fuse flag and its default."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import _tsdf_batch_cases as B
import _tsdf_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "network"))

CPU = torch.device("cpu")
IDS = [g["name"] for g in B.GROUPS]


def test_groups_keep_the_exclusions_under_the_cap_and_differ_per_sequence():
    worst = 0.0
    for group in B.GROUPS:
        live = [B.sequence_case(group, k) for k in range(len(group["poses"])) if group["poses"][k]]
        refs = [B.reference(c) for c in live]
        for c, (a, V64, W64, cmp) in zip(live, refs):
            worst = max(worst, 1.0 - cmp.mean())
            assert 1.0 - cmp.mean() <= T.MAX_EXCLUDED, c["name"]
            assert (V64 != a["volume"].astype(np.float64)).any(), c["name"]
        assert all(not np.array_equal(x[0]["volume"], y[0]["volume"]) for x, y in zip(refs, refs[1:]))   # the priors differ
        assert all(not np.array_equal(x[0]["rotation"][0], y[0]["rotation"][0]) for x, y in zip(refs, refs[1:]))   # and the poses
    print("worst excluded share over the groups' sequences: %.2f %%" % (100 * worst))
    # sequence 2's frame: part of the volume behind the camera, part of it outside the image
    a = B.reference(B.sequence_case(B.GROUPS[3], 2))[0]
    res = a["volume"].shape[0]
    idx = (np.arange(res) - res // 2) * a["voxel_scale"]
    p = np.stack(np.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3)
    q = (p @ a["rotation"][0].astype(np.float64).T + a["translation"][0]) * (np.array([1.0, -1.0, -1.0]) if a["flip_yz"] else 1.0)
    fx, _, cx, _ = a["intrinsics"][0]
    u = q[:, 0] / np.where(q[:, 2] > 0, q[:, 2], 1) * fx + cx
    assert (q[:, 2] < 0).any() and (q[:, 2] > 0).any() and ((q[:, 2] > 0) & ((u < -1) | (u > a["depth"].shape[2]))).any()


@pytest.mark.parametrize("group", B.GROUPS, ids=IDS)
def test_batched_torch_route_is_the_per_sequence_route_and_passes_the_fp64_check(group):
    from models.shape_fusion import tsdf_integrate_batch_torch, tsdf_integrate_torch
    args, kw, singles = B.pack(group, CPU)
    vols, wts = tsdf_integrate_batch_torch(*args, **kw)
    assert vols is args[0] and wts is args[1]
    for k, single in enumerate(singles):
        if single is None:
            assert vols[k] is None
            continue
        V, W = tsdf_integrate_torch(*single[0], **single[1])
        assert torch.equal(vols[k], V) and torch.equal(wts[k], W), k
        T.check(B.sequence_case(group, k), vols[k].numpy(), wts[k].numpy(), "batched torch route")


def _frames(single, depth_scale):
    args = single[0]
    return [({"depth": args[3][i], "seg": args[4][i], "intrinsics": args[5][i].tolist(), "depth_scale": depth_scale},
             {"rotation": args[6][i][None], "translation": args[7][i].reshape(1, 3, 1)}) for i in range(args[3].shape[0])]


@pytest.mark.parametrize("group", [B.GROUPS[0], B.GROUPS[2]], ids=[IDS[0], IDS[2]])
def test_volume_fusion_group_on_the_torch_route(group):
    from models.shape_fusion import VolumeFusionGroup, tsdf_integrate_torch
    _, kw, singles = B.pack(group, CPU)
    handed = [None if s is None else s[0][0].clone() for s in singles]
    keep = [None if h is None else h.clone() for h in handed]
    scale = next(s for s in singles if s is not None)[0][2]
    fusion = VolumeFusionGroup(handed, scale, 1.0, kw["trunc"], every=3, obj_class=kw["obj_class"], flip_yz=kw["flip_yz"], route="torch")
    assert fusion.states[1] is None and fusion.pending(1) == 0 and not fusion.due(1)
    for k, s in enumerate(singles):
        for fr in ([] if s is None else _frames(s, kw["depth_scale"])):
            fusion.push(k, *fr)
    assert [fusion.pending(k) for k in range(4)] == list(B.COUNTS4) and [fusion.due(k) for k in range(4)] == [True, False, False, False]
    out = fusion.flush([3, 0, 2])
    assert [fusion.pending(k) for k in range(4)] == [0, 0, 0, 0]
    for k, vol in zip((3, 0, 2), out):
        st = fusion.state(k)
        assert vol is st["volume"] and st["frames"] == B.COUNTS4[k] and vol.data_ptr() != handed[k].data_ptr()
        assert torch.equal(handed[k], keep[k])
        V, W = tsdf_integrate_torch(handed[k].clone(), torch.full_like(singles[k][0][1], 1.0), *singles[k][0][2:], **kw)
        assert torch.equal(vol, V) and torch.equal(st["weight"], W)
    again = fusion.flush([0, 3])   # nothing pending: nothing happens
    assert again[0] is fusion.state(0)["volume"] and fusion.state(0)["frames"] == 3


def test_the_group_refuses_frames_that_one_launch_cannot_share():
    from models.shape_fusion import VolumeFusionGroup
    _, kw, singles = B.pack(B.GROUPS[0], CPU)
    _, kw_u16, singles_u16 = B.pack(B.GROUPS[2], CPU)
    handed = [s[0][0] if s is not None else None for s in singles]
    new = lambda: VolumeFusionGroup(handed, singles[0][0][2], 1.0, kw["trunc"], route="torch")
    fusion = new()   # mixed image sizes
    fusion.push(0, *_frames(singles[0], None)[0])
    fr, pose = _frames(singles[2], None)[0]
    fusion.push(2, dict(fr, depth=fr["depth"][:12, :16].contiguous(), seg=fr["seg"][:12, :16].contiguous()), pose)
    before = [fusion.state(k)["volume"].clone() for k in (0, 2)]
    with pytest.raises(ValueError, match="sequences 0 and 2"):
        fusion.flush([0, 2])
    assert fusion.pending(0) == 1 and all(torch.equal(fusion.state(k)["volume"], b) for k, b in zip((0, 2), before))
    fusion = new()   # one sequence with depth_scale, one without
    fusion.push(0, *_frames(singles[0], None)[0])
    fusion.push(3, *_frames(singles_u16[3], kw_u16["depth_scale"])[0])
    with pytest.raises(ValueError, match="sequences 0 and 3"):
        fusion.flush([0, 3])


BAD = [
    ("mixed res", lambda a: (a[0].__setitem__(0, a[0][0][:9, :9, :9].contiguous()), a[1].__setitem__(0, a[1][0][:9, :9, :9].contiguous()))),
    ("mixed dtype", lambda a: a[0].__setitem__(2, a[0][2].float())),
    ("aliased volumes", lambda a: a[0].__setitem__(3, a[0][0])),
    ("counts do not sum to F", lambda a: a[8].__setitem__(0, 2)),
    ("None with a count", lambda a: (a[8].__setitem__(1, 1), a[8].__setitem__(0, 2))),
    ("S above the limit", lambda a: [a[i].extend([x] * 65533) for i, x in ((0, None), (1, None), (8, 0))]),
]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_refused_groups_raise_and_change_nothing(what, spoil):
    from models.shape_fusion import tsdf_integrate_batch_torch
    args, kw, _ = B.pack(B.GROUPS[0], CPU)
    args = list(args)
    held = [(v, w) for v, w in zip(args[0], args[1]) if v is not None]
    before = [(v.clone(), w.clone()) for v, w in held]
    spoil(args)
    with pytest.raises(ValueError):
        tsdf_integrate_batch_torch(*args, **kw)
    assert all(torch.equal(v, bv) and torch.equal(w, bw) for (v, w), (bv, bw) in zip(held, before))


def test_the_flag_parses_and_defaults_to_off():
    from parse_args import add_args
    parser = add_args(argparse.ArgumentParser())
    assert getattr(parser.parse_args(["--lockstep_fuse"]), "opt/lockstep_fuse") is True
    assert getattr(parser.parse_args([]), "opt/lockstep_fuse") is None
    assert "130 MB" in parser.format_help()


def test_the_configuration_sets_lockstep_fuse_to_false(tmp_path, monkeypatch):
    from configs.config import get_config
    from parse_args import add_args
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    parser = add_args(argparse.ArgumentParser())
    cfg = get_config(parser.parse_args(["--config", "objopt_test_HO3D.yml"]), save=False)
    assert cfg["opt"]["lockstep_fuse"] is False and cfg["opt"]["fuse_depth"] is False
    cfg = get_config(parser.parse_args(["--config", "objopt_test_HO3D.yml", "--lockstep_fuse", "--fuse_obj_depth"]), save=False)
    assert cfg["opt"]["lockstep_fuse"] is True and cfg["opt"]["fuse_depth"] is True
