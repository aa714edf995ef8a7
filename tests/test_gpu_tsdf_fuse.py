"""GPU: the TSDF fusion kernel (hotrack_amd/csrc/tsdf_fuse.hip, hotrack_amd.sdf.tsdf_integrate) against the float64 restatement of
the rule over the case list of tests/_tsdf_cases.py, within the tolerance measured there and with the same exclusions; one launch
of three frames against three launches of one; repeatability; refused calls; VolumeFusion without host synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

import _tsdf_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _run(case):
    from hotrack_amd import sdf
    a = T.reference(case)[0]
    args, kw = T.to_torch(a, _dev())
    V, W = sdf.tsdf_integrate(*args, **kw)
    assert V is args[0] and W is args[1]
    return a, args, kw, V, W


def _bits(x):
    x = x.detach().cpu().contiguous().numpy()
    return x.view(np.uint16 if x.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize("case", T.CASES, ids=[c["name"] for c in T.CASES])
def test_kernel_against_fp64(case):
    a, _, _, V, W = _run(case)
    T.check(case, V.cpu().numpy(), W.cpu().numpy(), "kernel")
    # a voxel no frame updated keeps its bytes (the fp32 restatement's update set, where the comparison holds)
    _, _, touched = T.fuse_fp32(a)
    keep = ~touched & T.reference(case)[3]
    assert keep.any()
    assert np.array_equal(_bits(V)[keep], _bits(torch.from_numpy(a["volume"].copy()))[keep])
    assert np.array_equal(_bits(W)[keep], _bits(torch.from_numpy(a["weight"].copy()))[keep])


@pytest.mark.parametrize("case", [c for c in T.CASES if c["vol"] == "float32" and len(c["poses"]) == 3], ids=lambda c: c["name"])
def test_one_launch_of_three_frames_equals_three_launches(case):
    from hotrack_amd import sdf
    _, args, kw, V, W = _run(case)
    single, _ = T.to_torch(T.reference(case)[0], _dev())
    for k in range(3):
        sdf.tsdf_integrate(single[0], single[1], single[2], *(x[k:k + 1].contiguous() for x in single[3:]), **kw)
    assert np.array_equal(_bits(V), _bits(single[0])) and np.array_equal(_bits(W), _bits(single[1]))


@pytest.mark.parametrize("case", [T.CASES[1], T.CASES[2]], ids=lambda c: c["name"])
def test_two_runs_are_bitwise_equal(case):
    _, _, _, V0, W0 = _run(case)
    _, _, _, V1, W1 = _run(case)
    assert np.array_equal(_bits(V0), _bits(V1)) and np.array_equal(_bits(W0), _bits(W1))


BAD = [
    ("res", lambda a, k: a.__setitem__(0, torch.zeros(1, 1, 1, device=_dev())) or a.__setitem__(1, torch.zeros(1, 1, 1, device=_dev())), ValueError),
    ("volume dtype", lambda a, k: a.__setitem__(0, a[0].double()), TypeError),
    ("non-contiguous volume", lambda a, k: a.__setitem__(0, a[0].transpose(0, 1)), ValueError),
    ("trunc", lambda a, k: k.__setitem__("trunc", 0.0), ValueError),
    ("voxel_scale", lambda a, k: a.__setitem__(2, float("nan")), ValueError),
    ("max_weight", lambda a, k: k.__setitem__("max_weight", float("inf")), ValueError),
    ("carve_weight", lambda a, k: k.__setitem__("carve_weight", -1.0), ValueError),
    ("no frames", lambda a, k: [a.__setitem__(i, a[i][:0]) for i in (3, 4, 5, 6, 7)], ValueError),
    ("cpu depth", lambda a, k: a.__setitem__(3, a[3].cpu()), RuntimeError),
]


@pytest.mark.parametrize("what,spoil,error", BAD, ids=[b[0] for b in BAD])
def test_refused_calls_raise_and_change_nothing(what, spoil, error):
    from hotrack_amd import sdf
    args, kw = T.to_torch(T.reference(T.CASES[0])[0], _dev())
    args = list(args)
    vol, wt = args[0], args[1]
    before = (_bits(vol).copy(), _bits(wt).copy())
    spoil(args, kw)
    with pytest.raises(error):
        sdf.tsdf_integrate(*args, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(vol), before[0]) and np.array_equal(_bits(wt), before[1])


def test_the_c_entry_refuses_and_launches_nothing():
    """The record checks of pn2s_tsdf_integrate itself, behind the binding's: a negative code, the volume's bytes unchanged."""
    import ctypes
    from hotrack_amd import sdf
    args, kw = T.to_torch(T.reference(T.CASES[0])[0], _dev())
    vol, wt, scale, depth, seg, intr, rot, trans = args
    before = (_bits(vol).copy(), _bits(wt).copy())

    def record(**over):
        r = sdf._TsdfFrames(res=5, vol_f16=0, frames=1, h=24, w=32, hs=24, ws=32, c=3, depth_u16=0, flip_yz=0, channel=1, value=255,
                            depth_scale=0.0, voxel_scale=scale, trunc=kw["trunc"], carve_weight=1.0, max_weight=64.0)
        r.volume, r.weight, r.depth, r.seg = vol.data_ptr(), wt.data_ptr(), depth.data_ptr(), seg.data_ptr()
        r.intrinsics, r.rotation, r.translation = intr.data_ptr(), rot.data_ptr(), trans.data_ptr()
        for k, v in over.items():
            setattr(r, k, v)
        return r

    for over in (dict(res=1), dict(res=513), dict(vol_f16=2), dict(trunc=0.0), dict(trunc=float("nan")), dict(voxel_scale=float("inf")),
                 dict(max_weight=0.0), dict(carve_weight=-1.0), dict(frames=0), dict(hs=5), dict(c=2), dict(channel=3), dict(depth=None),
                 dict(depth_u16=1)):
        assert sdf._lib.pn2s_tsdf_integrate(ctypes.byref(record(**over)), None) < 0, over
    assert sdf._lib.pn2s_tsdf_integrate(None, None) < 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(vol), before[0]) and np.array_equal(_bits(wt), before[1])
    assert sdf._lib.pn2s_tsdf_integrate(ctypes.byref(record()), None) == 0   # the unspoilt record is accepted
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(vol), before[0])


def test_volume_fusion_does_not_synchronise_and_keeps_the_callers_tensor():
    from models.shape_fusion import VolumeFusion
    case = T.CASES[2]
    a = T.reference(case)[0]
    args, kw = T.to_torch(a, _dev())
    handed = args[0].clone()
    keep = handed.clone()
    frames = [({"depth": args[3][k], "seg": args[4][k], "intrinsics": args[5][k], "depth_scale": a["depth_scale"]},
               {"rotation": args[6][k:k + 1], "translation": args[7][k].reshape(1, 3, 1)}) for k in range(3)]
    warm = VolumeFusion(handed, a["voxel_scale"], 1.0, a["trunc"], every=3)
    warm.push(*frames[0])
    warm.flush()   # (first use: whatever is set up once)
    fusion = VolumeFusion(handed, a["voxel_scale"], 1.0, a["trunc"], every=3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fr, pose in frames:
            fusion.push(fr, pose)
        out = fusion.flush()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert fusion.frames == 3 and torch.equal(handed, keep) and out.data_ptr() != handed.data_ptr()
    T.check(case, out.cpu().numpy(), fusion.weight.cpu().numpy(), "VolumeFusion")
