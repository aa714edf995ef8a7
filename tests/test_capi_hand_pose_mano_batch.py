"""CPU: the argument validation of the batched MANO hand-pose optimiser (include/pn2_ext.h: pn2x_hand_pose_mano_opt_batch,
pn2x_hand_pose_mano_batch_work_floats) -- bad sizes -1, NULL pointers -2, over a limit -3; no iterations and a batch whose
problems all sit out are no-ops -- and of its binding's refusals, before anything touches the device."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from hotrack_amd.ext import _HandPoseSetup as Setup, _lib  # noqa: E402

vp = ctypes.c_void_p
EINVAL, ENULL, ERANGE = -1, -2, -3


def _ceil16(n):
    return (n + 15) // 16 * 16


def test_the_library_exports_the_batched_mano_entry(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("pn2x_hand_pose_mano_opt_batch", "pn2x_hand_pose_mano_batch_work_floats"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(Setup) == 136


def test_work_floats():
    lib = _lib
    for p, v, s in ((67, 97, 3), (5120, 778, 8), (0, 5, 2)):
        assert lib.pn2x_hand_pose_mano_batch_work_floats(p, v, s) == s * p * _ceil16(3 * v) == s * lib.pn2x_hand_pose_mano_work_floats(p, v)
    assert lib.pn2x_hand_pose_mano_batch_work_floats(67, 97, 3) == 3 * 67 * 304
    assert lib.pn2x_hand_pose_mano_batch_work_floats(5120, 778, 8) == 8 * 5120 * 2336   # 95.7 M floats: 47.8 MB per sequence
    assert lib.pn2x_hand_pose_mano_batch_work_floats(0, 5, 2) == 0
    for bad in ((-1, 97, 3), (67, -1, 3), (67, 97, -1)):
        assert lib.pn2x_hand_pose_mano_batch_work_floats(*bad) == EINVAL, bad


def test_hand_pose_mano_opt_batch_argument_validation():
    lib = _lib
    one = vp(16)
    model = dict(parents=16, pose_block=16, skin_pack=16, skin_w=16, comps=16, pre=16, posedirs=16, pose_mean=16, kp_vertex=16)

    def call(p=256, v=70, j=21, k=2, f16=1, res=17, scale=0.01, centre=1, s=3, active=3, problems=one, offsets=one, iterations=5, **ptr):
        setup = Setup(p=p, v=v, j=j, k=k, vol_f16=f16, res=res, centre_root=centre, theta_scale=30.0, voxel_scale=scale, w_sil=0.1,
                      w_pen=1.0, w_vis=10.0, w_invis=0.0, w_temporal=1.0, w_attr=0.05, **dict(model, **ptr))
        return lib.pn2x_hand_pose_mano_opt_batch(setup, s, active, problems, offsets, iterations, 0.1, 0.9, None)

    # bad sizes: what pn2x_hand_pose_opt_batch rejects, and the MANO fields
    assert call(s=0) == EINVAL and call(s=-2) == EINVAL and call(active=-1) == EINVAL and call(active=4) == EINVAL
    assert call(p=0) == EINVAL and call(v=0) == EINVAL and call(j=0) == EINVAL and call(k=0) == EINVAL and call(iterations=-1) == EINVAL
    assert call(res=0) == EINVAL and call(res=16) == EINVAL and call(f16=2) == EINVAL and call(f16=-1) == EINVAL
    assert call(scale=0.0) == EINVAL and call(scale=-0.01) == EINVAL and call(scale=float("nan")) == EINVAL
    assert call(centre=2) == EINVAL and call(centre=-1) == EINVAL
    # over a limit
    assert call(s=65536, active=1) == ERANGE and call(iterations=4097) == ERANGE
    assert call(p=8193) == ERANGE and call(v=1025) == ERANGE and call(j=20) == ERANGE and call(k=5) == ERANGE and call(res=1025) == ERANGE
    # NULL: each shared pointer but posedirs, the table and the workspace when there is work to do
    for name in model:
        if name != "posedirs":
            assert call(**{name: None}) == ENULL, name
    assert call(problems=None) == ENULL and call(offsets=None) == ENULL
    # a setup without posedirs belongs to the plain entry; posedirs and offsets are read / written 16 bytes at a time
    assert call(posedirs=None) == EINVAL
    assert call(posedirs=24) == EINVAL and call(offsets=vp(24)) == EINVAL
    # a bad value before a limit before a NULL pointer
    assert call(offsets=vp(24), p=8193, pre=None) == EINVAL and call(p=8193, offsets=None) == ERANGE
    # no iterations, or nobody active: OK, nothing launched, neither the table nor the workspace needed
    assert call(iterations=0, problems=None, offsets=None) == 0 and call(iterations=0) == 0 and call(iterations=0, offsets=vp(24)) == 0
    assert call(active=0) == 0 and call(active=0, problems=None, offsets=None) == 0 and call(active=0, problems=None, iterations=0) == 0
    assert call(s=65535, active=0) == 0
    # (a no-op does not excuse a bad argument)
    assert call(iterations=0, s=0) == EINVAL and call(iterations=0, pre=None) == ENULL and call(active=0, posedirs=None) == EINVAL
    assert call(iterations=0, kp_vertex=None) == ENULL and call(active=0, pose_mean=None) == ENULL
    # the setup record itself: NULL, and an address no process owns (what a caller of an older ABI passes)
    assert lib.pn2x_hand_pose_mano_opt_batch(None, 3, 3, one, one, 5, 0.1, 0.9, None) == ENULL
    assert lib.pn2x_hand_pose_mano_opt_batch(ctypes.cast(vp(256), ctypes.POINTER(Setup)), 3, 3, one, one, 5, 0.1, 0.9, None) == EINVAL
    assert lib.pn2x_hand_pose_mano_opt_batch(ctypes.cast(vp(65535), ctypes.POINTER(Setup)), 3, 3, one, one, 0, 0.1, 0.9, None) == EINVAL


def test_the_plain_entry_still_refuses_a_mano_setup():
    setup = Setup(p=256, v=70, j=21, k=2, vol_f16=1, res=17, centre_root=1, theta_scale=30.0, voxel_scale=0.01,
                  **{n: 16 for n in ("parents", "pose_block", "skin_pack", "skin_w", "comps", "pre", "posedirs", "pose_mean", "kp_vertex")})
    assert _lib.pn2x_hand_pose_opt_batch(setup, 3, 3, vp(16), 5, 0.1, 0.9, None) == EINVAL
    setup.posedirs = None
    assert _lib.pn2x_hand_pose_opt_batch(setup, 3, 0, vp(16), 5, 0.1, 0.9, None) == 0


def _models():
    from hotrack_amd import ext
    from models.hand_model import SyntheticLBSHand, named_hand_model
    tables = named_hand_model("synthetic_mano").skinning_tables()
    kpv = tables["kp_vertex"].clone()
    owned = [i for i, v in enumerate(kpv.tolist()) if v >= 0]
    kpv[owned[1]] = kpv[owned[0]]
    return (ext, ext.hand_pose_model(SyntheticLBSHand().skinning_tables(), "cpu"), ext.hand_pose_model(tables, "cpu"),
            ext.hand_pose_model(dict(tables, kp_vertex=kpv), "cpu"))


def test_the_bindings_send_each_kind_of_model_to_its_entry():
    """CPU tensors: every refusal comes before any device work."""
    ext, plain, mano, two_keypoints = _models()
    states = torch.zeros(1, ext.HAND_POSE_STATE_FLOATS)
    assert not plain["mano"] and mano["mano"] and mano["mano_ok"] and two_keypoints["mano"] and not two_keypoints["mano_ok"]
    with pytest.raises(ValueError, match="hand_pose_opt_batch"):
        ext.hand_pose_mano_opt_batch(plain, [None], states, 1, 0.1, 0.9)
    with pytest.raises(ValueError, match="one vertex serves two keypoints"):
        ext.hand_pose_mano_opt_batch(two_keypoints, [None], states, 1, 0.1, 0.9)
    with pytest.raises(ValueError, match="MANO entries"):
        ext.hand_pose_opt_batch(mano, [None], states, 1, 0.1, 0.9)
    with pytest.raises(ValueError, match="frames is empty"):
        ext.hand_pose_mano_opt_batch(mano, [], states, 1, 0.1, 0.9)
    with pytest.raises(ValueError, match=r"states .* is not \(2, 90\)"):
        ext.hand_pose_mano_opt_batch(mano, [None, None], states, 1, 0.1, 0.9)
    with pytest.raises(RuntimeError, match="no CPU path"):   # (the good model gets as far as the tensors)
        ext.hand_pose_mano_opt_batch(mano, [None], states, 1, 0.1, 0.9)
