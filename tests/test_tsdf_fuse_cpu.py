"""CPU: the torch route of the TSDF fusion (network/models/shape_fusion.py) against the float64 restatement of the rule
(tests/_tsdf_cases.py), the shape improvement the weights promise, untouched voxels, VolumeFusion's ownership of its volume, and
the refused inputs."""
import os
import sys

import numpy as np
import pytest
import torch

import _tsdf_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "network"))

CPU = torch.device("cpu")


def _torch_route(case):
    from models.shape_fusion import tsdf_integrate_torch
    a = T.reference(case)[0]
    args, kw = T.to_torch(a, CPU)
    V, W = tsdf_integrate_torch(*args, **kw)
    assert V is args[0] and W is args[1]
    return a, V.numpy(), W.numpy()


def test_cases_keep_the_exclusions_under_the_cap_and_exercise_the_rule():
    seen_behind = seen_outside = seen_carve = seen_saturated = False
    for case in T.CASES:
        a, V64, W64, cmp = T.reference(case)
        assert 1.0 - cmp.mean() <= T.MAX_EXCLUDED, case["name"]
        assert (V64 != a["volume"].astype(np.float64)).any(), case["name"]
        seen_saturated |= bool((W64 == a["max_weight"]).any() and a["max_weight"] < 64)
        seen_carve |= bool((W64 > a["weight"]).any())
    # part of a volume behind the camera, part outside the image: the close poses
    a = T.reference(T.CASES[5])[0]
    res = a["volume"].shape[0]
    idx = (np.arange(res) - res // 2) * a["voxel_scale"]
    p = np.stack(np.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3)
    q = p @ a["rotation"][0].astype(np.float64).T + a["translation"][0]
    seen_behind = bool((q[:, 2] < 0).any() and (q[:, 2] > 0).any())
    fx, fy, cx, cy = a["intrinsics"][0]
    u = q[:, 0] / np.where(q[:, 2] > 0, q[:, 2], 1) * fx + cx
    seen_outside = bool(((q[:, 2] > 0) & ((u < -1) | (u > a["depth"].shape[2]))).any())
    assert seen_behind and seen_outside and seen_carve and seen_saturated
    tol_v, tol_w = T.tolerances()
    print("fp32 restatement against fp64: tolerance |dV| %.3e  |dW| %.3e" % (tol_v, tol_w))
    assert 0 < tol_v < 1e-6


@pytest.mark.parametrize("case", T.CASES, ids=[c["name"] for c in T.CASES])
def test_torch_route_against_fp64(case):
    a, V, W = _torch_route(case)
    T.check(case, V, W, "torch route")


@pytest.mark.parametrize("case", T.CASES[:3], ids=[c["name"] for c in T.CASES[:3]])
def test_unobserved_voxels_keep_their_bits(case):
    a, V, W = _torch_route(case)
    _, _, touched = T.fuse_fp32(a)
    keep = ~touched
    assert keep.any() and touched.any()
    bits = lambda x: x.view(np.uint16 if x.dtype == np.float16 else np.uint32)
    assert np.array_equal(bits(V)[keep], bits(a["volume"])[keep]) and np.array_equal(bits(W)[keep], bits(a["weight"])[keep])
    assert (W[touched] != a["weight"][touched]).any()


def _trilinear_abs_mean(vol, scale, pts):
    res = vol.shape[0]
    x = pts / scale + res // 2
    i0 = np.clip(np.floor(x).astype(np.int64), 0, res - 2)
    fr = x - i0
    out = 0.0
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = np.abs(1 - dx - fr[:, 0]) * np.abs(1 - dy - fr[:, 1]) * np.abs(1 - dz - fr[:, 2])
                out = out + w * vol[i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz]
    return float(np.abs(out).mean())


def test_fusing_true_views_halves_the_surface_residual():
    """prior_weight = 1 and one observation of weight 1: a seen voxel moves at least half way, prior / (prior + 1) = 1/2."""
    from datasets.synthetic import capsule_surface, capsule_volume, render_depth_frame, _rot
    from models.shape_fusion import VolumeFusion
    res, scale, h, w = 101, 0.004, 120, 160
    prior = torch.from_numpy(capsule_volume(res, scale, model_radius=0.03))
    K = dict(fx=150.0, fy=150.0, cx=79.5, cy=59.5)
    rng = np.random.default_rng(5)
    dense = capsule_surface(rng, 60000, noise=0.0)
    surface = capsule_surface(rng, 4000, noise=0.0)
    fusion = VolumeFusion(prior, scale, prior_weight=1.0, trunc=5 * scale, every=8)
    seen = np.zeros(len(surface), dtype=bool)
    for k in range(8):
        R = _rot(np.array([0.3, 1.0, 0.2]), 2 * np.pi * k / 8) @ _rot(np.array([1.0, 0.0, 0.0]), 0.4 * k)
        t = np.array([0.01, -0.01, 0.5])
        depth, seg, _, _ = render_depth_frame(None, dense @ R.T + t, K, h, w, splat=1)
        fusion.push({"depth": torch.from_numpy(depth), "seg": torch.from_numpy(seg), "intrinsics": K},
                    {"rotation": torch.from_numpy(R.astype(np.float32)), "translation": torch.from_numpy(t.astype(np.float32))})
        q = surface @ R.T + t
        u, v = np.rint(q[:, 0] / q[:, 2] * K["fx"] + K["cx"]).astype(int), np.rint(q[:, 1] / q[:, 2] * K["fy"] + K["cy"]).astype(int)
        seen |= np.abs(depth[v, u] - q[:, 2]) < scale   # the depth at the point's pixel is the point's own surface, to a voxel
    assert fusion.due() and fusion.pending == 8
    fused = fusion.flush()
    assert fusion.pending == 0 and fusion.frames == 8 and fused is fusion.volume
    assert seen.mean() > 0.3
    before = _trilinear_abs_mean(prior.numpy().astype(np.float64), scale, surface[seen])
    after = _trilinear_abs_mean(fused.numpy().astype(np.float64), scale, surface[seen])
    print("mean |V| at %d seen surface points: %.4e before, %.4e after (ratio %.3f)" % (seen.sum(), before, after, after / before))
    assert 0.009 < before < 0.011 and after < 0.5 * before


def test_volume_fusion_leaves_the_callers_tensor_untouched():
    from models.shape_fusion import VolumeFusion
    a = T.reference(T.CASES[2])[0]
    handed = torch.from_numpy(a["volume"].copy())
    keep = handed.clone()
    fusion = VolumeFusion(handed, a["voxel_scale"], 1.0, a["trunc"], every=2, route="torch")
    assert fusion.volume.data_ptr() != handed.data_ptr() and float(fusion.weight.min()) == float(fusion.weight.max()) == 1.0
    for k in range(3):
        fusion.push({"depth": torch.from_numpy(a["depth"][k].view(np.int16).copy()), "seg": torch.from_numpy(a["seg"][k].copy()),
                     "intrinsics": a["intrinsics"][k].tolist(), "depth_scale": a["depth_scale"]},
                    {"rotation": torch.from_numpy(a["rotation"][k].copy())[None], "translation": torch.from_numpy(a["translation"][k].copy()).reshape(1, 3, 1)})
        assert fusion.due() == (k >= 1)
    out = fusion.flush()
    assert torch.equal(handed, keep) and not torch.equal(out, keep)
    # the three pushes are the case's three frames: the result is the route's
    args, kw = T.to_torch(a, CPU)
    from models.shape_fusion import tsdf_integrate_torch
    V, W = tsdf_integrate_torch(*args, **kw)
    assert torch.equal(V, out) and torch.equal(W, fusion.weight)
    assert fusion.flush() is out and fusion.frames == 3   # nothing pending: nothing happens


BAD = [
    ("res", lambda a, k: a.__setitem__(0, torch.zeros(1, 1, 1)) or a.__setitem__(1, torch.zeros(1, 1, 1)), ValueError),
    ("volume dtype", lambda a, k: a.__setitem__(0, a[0].double()), TypeError),
    ("non-contiguous volume", lambda a, k: a.__setitem__(0, a[0].transpose(0, 1)), ValueError),
    ("non-contiguous depth", lambda a, k: a.__setitem__(3, a[3].transpose(1, 2)), ValueError),
    ("weight dtype", lambda a, k: a.__setitem__(1, a[1].half()), ValueError),
    ("trunc", lambda a, k: k.__setitem__("trunc", 0.0), ValueError),
    ("trunc nan", lambda a, k: k.__setitem__("trunc", float("nan")), ValueError),
    ("voxel_scale", lambda a, k: a.__setitem__(2, float("inf")), ValueError),
    ("max_weight", lambda a, k: k.__setitem__("max_weight", -1.0), ValueError),
    ("carve_weight", lambda a, k: k.__setitem__("carve_weight", -0.5), ValueError),
    ("no frames", lambda a, k: [a.__setitem__(i, a[i][:0]) for i in (3, 4, 5, 6, 7)], ValueError),
    ("depth dtype", lambda a, k: a.__setitem__(3, a[3].double()), TypeError),
    ("depth_scale without counts", lambda a, k: k.__setitem__("depth_scale", 0.001), TypeError),
    ("seg factor", lambda a, k: a.__setitem__(4, a[4][:, :5].contiguous()), ValueError),
    ("class channel", lambda a, k: k.__setitem__("obj_class", (3, 255)), ValueError),
    ("rotation shape", lambda a, k: a.__setitem__(6, a[6].reshape(-1, 9)), ValueError),
]


@pytest.mark.parametrize("what,spoil,error", BAD, ids=[b[0] for b in BAD])
def test_refused_inputs_raise(what, spoil, error):
    from models.shape_fusion import tsdf_integrate_torch
    args, kw = T.to_torch(T.reference(T.CASES[0])[0], CPU)
    args = list(args)
    spoil(args, kw)
    before = [x.clone() if isinstance(x, torch.Tensor) else x for x in args[:2]]
    with pytest.raises(error):
        tsdf_integrate_torch(*args, **kw)
    assert torch.equal(before[0], args[0]) and torch.equal(before[1], args[1])


def test_capsule_model_radius_default_is_unchanged():
    from datasets.synthetic import SyntheticObjectSequences, capsule_volume
    assert np.array_equal(capsule_volume(21, 0.02).view(np.uint16), capsule_volume(21, 0.02, model_radius=0.04).view(np.uint16))
    small = capsule_volume(21, 0.02, model_radius=0.03)
    inner = np.abs(small.astype(np.float64)) < 0.08   # (not clamped in either volume)
    assert inner.any() and np.allclose((small.astype(np.float64) - capsule_volume(21, 0.02))[inner], 0.01, atol=2e-4)
    cfg = {"num_points": 64, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}}
    a = SyntheticObjectSequences(cfg, 1, 2, res=21, stride=0.02)[0]
    b = SyntheticObjectSequences(cfg, 1, 2, res=21, stride=0.02, model_radius=0.03)[0]
    assert torch.equal(a[0]["obj_points"], b[0]["obj_points"]) and torch.equal(a[1]["obj_points"], b[1]["obj_points"])
    assert torch.equal(a[0]["obj_model_points"], b[0]["obj_model_points"])
    assert torch.equal(b[0]["sdf_volume"], torch.from_numpy(small)) and not torch.equal(a[0]["sdf_volume"], b[0]["sdf_volume"])
