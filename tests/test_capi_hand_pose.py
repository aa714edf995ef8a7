"""CPU: argument validation of pn2x_hand_pose_energy / pn2x_hand_pose_opt and the pn2x_hand_pose_opt_supported query
(include/pn2_ext.h) -- everything is checked before any device work -- and of their Python bindings."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

ci, cl, cf, cd, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
COMMON = [ci] * 4 + [vp] * 7 + [cf] + [vp] * 7 + [ci, ci, cf, vp, ci, ci] + [cf] * 10


def _common(p=768, v=778, j=21, k=2, ptr=None, res=151, f16=1, scale=0.003, h=480, w=640):
    return [p, v, j, k] + [ptr] * 7 + [30.0] + [ptr] * 7 + [f16, res, scale, ptr, h, w] + [1.0] * 10


def test_hand_pose_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    sup = lib.pn2x_hand_pose_opt_supported
    sup.argtypes = [ci] * 6
    assert sup(5120, 778, 21, 2, 10, 151) == 1 and sup(8192, 1024, 21, 4, 10, 201) == 1 and sup(1, 1, 21, 1, 10, 1) == 1
    assert sup(8193, 778, 21, 2, 10, 151) == 0 and sup(0, 778, 21, 2, 10, 151) == 0      # candidates
    assert sup(5120, 1025, 21, 2, 10, 151) == 0 and sup(5120, 0, 21, 2, 10, 151) == 0    # vertices
    assert sup(5120, 778, 20, 2, 10, 151) == 0 and sup(5120, 778, 22, 2, 10, 151) == 0   # the 21 keypoints
    assert sup(5120, 778, 21, 5, 10, 151) == 0 and sup(5120, 778, 21, 0, 10, 151) == 0   # weights per vertex
    assert sup(5120, 778, 21, 2, 12, 151) == 0                                           # pose components
    assert sup(5120, 778, 21, 2, 10, 150) == 0 and sup(5120, 778, 21, 2, 10, 1025) == 0  # volume
    wf = lib.pn2x_hand_pose_opt_work_floats
    wf.argtypes, wf.restype = [ci], cl
    assert wf(5120) == 4 * 5120 and wf(-1) == -1
    one = ctypes.c_void_p(16)
    e = lib.pn2x_hand_pose_energy
    e.argtypes = COMMON + [vp] * 6
    tail = [one, one, one, None, None, None]
    assert e(*_common(ptr=one, p=0), *tail) == -1                 # p < 1
    assert e(*_common(ptr=one, res=150), *tail) == -1             # even res
    assert e(*_common(ptr=one, scale=0.0), *tail) == -1           # voxel_scale <= 0
    assert e(*_common(ptr=one, f16=2), *tail) == -1
    assert e(*_common(ptr=one, p=8193), *tail) == -3              # beyond the limits
    assert e(*_common(ptr=one, j=20), *tail) == -3
    assert e(*_common(ptr=one, k=5), *tail) == -3
    assert e(*_common(ptr=None), *tail) == -2                     # NULL tables
    assert e(*_common(ptr=one), None, one, one, None, None, None) == -2   # NULL state
    o = lib.pn2x_hand_pose_opt
    o.argtypes = COMMON + [ci, cd, cd] + [vp] * 4
    assert o(*_common(ptr=one), -1, 0.1, 0.9, one, one, None, None) == -1       # iterations < 0
    assert o(*_common(ptr=one), 5000, 0.1, 0.9, one, one, None, None) == -3
    assert o(*_common(ptr=one), 0, 0.1, 0.9, None, None, None, None) == 0       # no iterations: no-op
    assert o(*_common(ptr=one), 5, 0.1, 0.9, None, one, None, None) == -2       # NULL state
    assert o(*_common(ptr=None), 5, 0.1, 0.9, one, one, None, None) == -2
    assert o(*_common(ptr=one, v=2000), 5, 0.1, 0.9, one, one, None, None) == -3


def _cpu_call(P=64, res=151):
    from hotrack_amd import ext
    from models.hand_model import SyntheticLBSHand
    model = ext.hand_pose_model(SyntheticLBSHand().skinning_tables(), "cpu")
    z = torch.zeros
    return ext, dict(model=model, rest=ext.hand_pose_rest(model), theta_scale=30, pre=z(P, 16), state=z(ext.HAND_POSE_STATE_FLOATS),
                     pred_kp=z(21, 3), last_kp=None, vis_mask=z(21, dtype=torch.uint8), obj_r=torch.eye(3), obj_t=z(3),
                     volume=z(res, res, res, dtype=torch.float16), voxel_scale=0.003, mask=z(48, 64, dtype=torch.uint8),
                     proj={"fx": 60.0, "fy": 60.0, "cx": 32.0, "cy": 24.0},
                     weights={k: 1.0 for k in ext.HAND_POSE_WEIGHTS})


def test_bindings_refuse_cpu_tensors_and_unsupported_sizes():
    ext, kw = _cpu_call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.hand_pose_opt(iterations=5, scaling_coefficient2=0.1, beta=0.9, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.hand_pose_energy(**kw)
    ext, kw = _cpu_call(P=8200)
    with pytest.raises(ValueError, match="outside"):
        ext.hand_pose_opt(iterations=5, scaling_coefficient2=0.1, beta=0.9, **kw)
    ext, kw = _cpu_call(res=150)
    with pytest.raises(ValueError, match="outside"):
        ext.hand_pose_energy(**kw)
    assert ext.hand_pose_opt_supported(5120, 778, 21, 2) and not ext.hand_pose_opt_supported(5120, 778, 21, 2, 10, 150)


def test_packed_skinning_table_round_trips():
    from hotrack_amd import ext
    from models.hand_model import SyntheticLBSHand
    t = SyntheticLBSHand().skinning_tables()
    m = ext.hand_pose_model(t, "cpu")
    pack = m["skin_pack"].long()
    assert torch.equal(pack & 31, t["skin_idx"][:, 0]) and torch.equal((pack >> 5) & 31, t["skin_idx"][:, 1])
    offs = t["finger_offsets"].tolist()
    for f in range(5):
        assert sorted(torch.nonzero((pack >> (20 + f)) & 1).flatten().tolist()) == sorted(set(t["tips"][offs[f]:offs[f + 1]].tolist()))
    assert m["fingers_ok"] and m["V"] == 778 and m["K"] == 2 and m["J"] == 21
