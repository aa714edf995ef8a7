"""GPU: the volume raycast kernel (hotrack_amd/csrc/sdf_raycast.hip, hotrack_amd.sdf.volume_raycast) against the float64 restatement of
the rule on every case of tests/_raycast_cases.py, under the tolerances measured there; its determinism, the equality of one launch
of F frames with F launches of one, of the depth with and without normals; the comparison launch against the torch route; and that
neither binding reads anything back."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "network"), os.path.dirname(os.path.abspath(__file__))]

import _raycast_cases as C  # noqa: E402
import _tsdf_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [c["name"] for c in C.CASES]


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def rendered():
    from hotrack_amd import sdf
    out = {}
    for case in C.CASES:
        args, kw = C.to_torch(C.reference(case)[0], _dev())
        out[case["name"]] = (args, kw) + sdf.volume_raycast(*args, **kw)
    return out


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_kernel_matches_the_float64_rule(case, rendered):
    _, _, z, n = rendered[case["name"]]
    assert z.is_cuda and z.dtype == torch.float32 and n.dtype == torch.float32
    C.check(case, z.cpu().numpy(), n.cpu().numpy(), "kernel")


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_two_runs_one_launch_per_frame_and_no_normals_are_bit_equal(case, rendered):
    from hotrack_amd import sdf
    args, kw, z, n = rendered[case["name"]]
    z2, n2 = sdf.volume_raycast(*args, **kw)
    assert torch.equal(z.view(torch.int32), z2.view(torch.int32)) and torch.equal(n.view(torch.int32), n2.view(torch.int32))
    z3, none = sdf.volume_raycast(*args, normals=False, **kw)
    assert none is None and torch.equal(z.view(torch.int32), z3.view(torch.int32))
    vol, scale, K, R, t, hw = args
    if K.shape[0] > 1:
        for k in range(K.shape[0]):
            zk, nk = sdf.volume_raycast(vol, scale, K[k:k + 1].contiguous(), R[k:k + 1].contiguous(), t[k:k + 1].contiguous(), hw, **kw)
            assert torch.equal(zk[0].view(torch.int32), z[k].view(torch.int32)) and torch.equal(nk[0].view(torch.int32), n[k].view(torch.int32))


def test_nan_cell_leaves_other_rays_alone(rendered):
    from hotrack_amd import sdf
    case = next(c for c in C.CASES if c["kind"] == "nan")
    args, kw, z, _ = rendered[case["name"]]
    clean = torch.where(torch.isnan(args[0]), torch.full_like(args[0], 0.05), args[0])
    zc, _ = sdf.volume_raycast(clean, *args[1:], **kw)
    keep = torch.from_numpy(~C.sensitive(case)).to(_dev())   # (the rays that sampled the NaN are among the left-out pixels)
    assert torch.equal(z[keep].view(torch.int32), zc[keep].view(torch.int32)) and int((z[keep] > 0).sum()) > 500


def _observed(name):
    """The frames of a _tsdf_cases case on the device, and the true capsule rendered at their poses by the kernel."""
    from hotrack_amd import sdf
    a = T.build(next(c for c in T.CASES if c["name"] == name))
    res, scale = 33, 0.008
    ax = (np.arange(res) - res // 2) * scale
    vol = T.capsule_sdf(np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1), 0.04).astype(np.float16)
    t = lambda x: torch.from_numpy(np.array(x, order="C")).to(_dev())
    z, _ = sdf.volume_raycast(t(vol), scale, t(a["intrinsics"]), t(a["rotation"]), t(a["translation"]), a["depth"].shape[1:],
                              flip_yz=a["flip_yz"], normals=False)
    depth = a["depth"]
    depth = torch.from_numpy(depth.view(np.int16).copy()).to(_dev()) if depth.dtype == np.uint16 else t(depth)
    return a, z, depth, t(a["seg"])


@pytest.mark.parametrize("name", ["res17_f16_flip_F3", "res33_u16_seg2_F3", "res33_f16_u16_flip", "res17_u16_seg3_F2"])
def test_compare_matches_the_torch_route(name):
    from hotrack_amd import sdf
    from models.volume_render import raycast_compare_torch
    a, z, depth, seg = _observed(name)
    kw = dict(obj_class=a["obj_class"], depth_scale=a["depth_scale"], occl_margin=0.01)
    got = sdf.raycast_compare(z, depth, seg, **kw)
    assert torch.equal(got, sdf.raycast_compare(z, depth, seg, **kw))
    want = raycast_compare_torch(z.cpu(), depth.cpu(), seg.cpu(), **kw)
    # the residual in float64 from the same fp32 terms: n fp32 additions of n non-negative terms err by at most n u sum (u = 2^-24)
    D = a["depth"].astype(np.float64) * a["depth_scale"] if a["depth_scale"] is not None else a["depth"].astype(np.float64)
    D = D.astype(np.float32)
    Z = z.cpu().numpy()
    got = got.cpu().numpy()
    print(name, got.tolist())
    assert np.array_equal(got[:, [0, 1, 3]], want.numpy()[:, [0, 1, 3]]) and (got[:, 0] > 0).all()
    obj = np.repeat(np.repeat(a["seg"][..., a["obj_class"][0]] == a["obj_class"][1], a["depth"].shape[1] // a["seg"].shape[1], axis=1),
                    a["depth"].shape[2] // a["seg"].shape[2], axis=2)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(D) & (D > 0)
        hit = Z > 0
        occ = ~obj & valid & hit & (D < Z - np.float32(0.01))
        both = obj & valid & hit & ~occ
        terms = np.where(both, np.abs(D - Z), np.float32(0)).astype(np.float64)
    exact = terms.reshape(terms.shape[0], -1).sum(axis=1)
    assert np.array_equal(both.reshape(both.shape[0], -1).sum(axis=1), got[:, 0])
    assert (np.abs(got[:, 2] - exact) <= got[:, 0] * 2.0 ** -24 * exact + 1e-12).all(), (got[:, 2], exact)


def test_no_read_backs():
    from hotrack_amd import sdf
    a, z, depth, seg = _observed("res33_u16_seg2_F3")
    args, kw = C.to_torch(C.reference(C.CASES[2])[0], _dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = sdf.volume_raycast(*args, **kw)
        stats = sdf.raycast_compare(z, depth, seg, obj_class=a["obj_class"], depth_scale=a["depth_scale"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out[0].shape == (3, 48, 64) and stats.shape == (3, 4)


def test_cpu_tensors_are_refused_in_words():
    from hotrack_amd import sdf
    args, kw = C.to_torch(C.reference(C.CASES[0])[0], "cpu")
    with pytest.raises(RuntimeError, match="volume_raycast_torch"):
        sdf.volume_raycast(*args, **kw)
