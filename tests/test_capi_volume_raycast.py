"""CPU: the argument validation of the raycast entries (include/pn2_sdf.h: pn2s_volume_raycast, pn2s_raycast_compare) -- the record
sizes, bad values -1, NULL pointers -2, over a limit -3 -- before anything touches the device; GPU: a refused call launches nothing,
so outputs pre-filled with a pattern stay untouched."""
import ctypes

import pytest

vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class Raycast(ctypes.Structure):
    _fields_ = ([(n, vp) for n in ("volume", "intrinsics", "rotation", "translation", "depth", "normal")] +
                [(n, cf) for n in ("voxel_scale", "step_scale", "min_step")] +
                [(n, ci) for n in ("res", "vol_f16", "frames", "h", "w", "flip_yz", "refine", "max_steps", "pad_")])


class Frames(ctypes.Structure):
    _fields_ = ([(n, vp) for n in ("rendered", "depth", "seg", "out")] + [("depth_scale", ctypes.c_double), ("occl_margin", cf)] +
                [(n, ci) for n in ("frames", "h", "w", "hs", "ws", "c", "depth_u16", "channel", "value")])


def _lib(path):
    lib = ctypes.CDLL(path)
    lib.pn2s_volume_raycast.argtypes = [ctypes.POINTER(Raycast), vp]
    lib.pn2s_volume_raycast.restype = ci
    lib.pn2s_raycast_compare.argtypes = [ctypes.POINTER(Frames), vp]
    lib.pn2s_raycast_compare.restype = ci
    return lib


def _raycast(**over):
    one = 16
    r = dict(volume=one, intrinsics=one, rotation=one, translation=one, depth=one, normal=one, voxel_scale=0.002, step_scale=1.0, min_step=0.5,
             res=201, vol_f16=1, frames=1, h=480, w=640, flip_yz=0, refine=8, max_steps=1608)
    r.update(over)
    return Raycast(**r)


def _frames(**over):
    one = 16
    r = dict(rendered=one, depth=one, seg=one, out=one, depth_scale=0.001, occl_margin=0.01, frames=2, h=480, w=640, hs=240, ws=320, c=3,
             depth_u16=1, channel=1, value=255)
    r.update(over)
    return Frames(**r)


def test_record_sizes():
    assert ctypes.sizeof(Raycast) == 96 and ctypes.sizeof(Frames) == 80   # the static_asserts of sdf_raycast.hip


def test_volume_raycast_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    call = lambda **over: lib.pn2s_volume_raycast(ctypes.byref(_raycast(**over)), None)
    assert lib.pn2s_volume_raycast(None, None) == -2
    assert call(res=1) == -1 and call(res=0) == -1 and call(res=-5) == -1
    assert call(frames=0) == -1 and call(h=0) == -1 and call(w=-1) == -1
    assert call(vol_f16=2) == -1 and call(flip_yz=-1) == -1
    for name in ("voxel_scale", "step_scale", "min_step"):
        for x in (0.0, -0.5, float("nan"), float("inf")):
            assert call(**{name: x}) == -1, (name, x)
    assert call(refine=-1) == -1 and call(refine=17) == -1 and call(max_steps=0) == -1 and call(max_steps=-3) == -1
    assert call(res=513) == -3 and call(h=1 << 15, w=1 << 14) == -3 and call(frames=65536) == -3 and call(h=8 * 65535 + 1, w=1) == -3
    assert call(res=1, volume=None) == -1 and call(res=513, volume=None) == -3            # the order: values, limits, pointers
    for name in ("volume", "intrinsics", "rotation", "translation", "depth"):
        assert call(**{name: None}) == -2, name


def test_raycast_compare_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    call = lambda **over: lib.pn2s_raycast_compare(ctypes.byref(_frames(**over)), None)
    assert lib.pn2s_raycast_compare(None, None) == -2
    assert call(frames=0) == -1 and call(h=0) == -1 and call(ws=0) == -1
    assert call(hs=241) == -1 and call(hs=480) == -1 and call(c=2) == -1                  # no integer factor; two factors; channels
    assert call(channel=3) == -1 and call(channel=-1) == -1 and call(value=256) == -1 and call(value=-1) == -1
    assert call(depth_u16=2) == -1 and call(depth_scale=0.0) == -1 and call(depth_scale=float("nan")) == -1
    assert call(occl_margin=-0.01) == -1 and call(occl_margin=float("nan")) == -1 and call(occl_margin=float("inf")) == -1
    assert call(h=1 << 15, w=1 << 14, hs=1 << 15, ws=1 << 14) == -3 and call(frames=65536) == -3
    for name in ("rendered", "depth", "seg", "out"):
        assert call(**{name: None}) == -2, name


@pytest.mark.gpu
def test_a_refused_call_launches_nothing():
    import torch
    from hotrack_amd import sdf
    dev = torch.device("cuda", 0)
    lib = _lib(sdf._lib._name)
    vol = torch.full((9, 9, 9), 0.05, dtype=torch.float32, device=dev)
    K = torch.tensor([[40.0, 40.0, 16.0, 12.0]], device=dev)
    R, t = torch.eye(3, device=dev)[None].contiguous(), torch.tensor([[0.0, 0.0, 0.3]], device=dev)
    depth = torch.full((1, 24, 32), -7.0, device=dev)
    normal = torch.full((1, 24, 32, 3), -7.0, device=dev)
    stats = torch.full((1, 4), -7.0, device=dev)
    seg = torch.zeros((1, 24, 32, 3), dtype=torch.uint8, device=dev)
    good = dict(volume=vol.data_ptr(), intrinsics=K.data_ptr(), rotation=R.data_ptr(), translation=t.data_ptr(), depth=depth.data_ptr(),
                normal=normal.data_ptr(), voxel_scale=0.02, res=9, vol_f16=0, h=24, w=32, max_steps=72)
    for over, code in ((dict(refine=17), -1), (dict(min_step=0.0), -1), (dict(frames=65536), -3), (dict(rotation=None), -2)):
        assert lib.pn2s_volume_raycast(ctypes.byref(_raycast(**dict(good, **over))), None) == code
    cmp = dict(rendered=depth.data_ptr(), depth=depth.data_ptr(), seg=seg.data_ptr(), out=stats.data_ptr(), frames=1, h=24, w=32, hs=24, ws=32,
               depth_u16=0)
    for over, code in ((dict(c=2), -1), (dict(frames=65536), -3), (dict(seg=None), -2)):
        assert lib.pn2s_raycast_compare(ctypes.byref(_frames(**dict(cmp, **over))), None) == code
    torch.cuda.synchronize()
    assert bool((depth == -7).all()) and bool((normal == -7).all()) and bool((stats == -7).all())
    assert lib.pn2s_volume_raycast(ctypes.byref(_raycast(**good)), None) == 0                 # and the accepted call writes every pixel
    assert lib.pn2s_raycast_compare(ctypes.byref(_frames(**cmp)), None) == 0
    torch.cuda.synchronize()
    assert bool((depth == 0).all()) and bool((normal == 0).all()) and stats.tolist() == [[0.0, 0.0, 0.0, 0.0]]
