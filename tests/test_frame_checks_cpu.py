"""CPU: tsdf_check and raycast_compare_check agree on what observed frames are (hotrack_amd/sdf.py: one helper behind both; the
kernels' side is hotrack_amd/csrc/frame_device.h).  For one table of spoiled depth / seg / obj_class / depth_scale arguments both
raise the same exception type with the same message after their own name, and an unspoiled call returns the tuples the routes'
own tests pin."""
import pytest
import torch

F, H, W, HS, WS, C = 2, 8, 12, 4, 6, 3


def _good():
    return dict(depth=torch.zeros((F, H, W)), seg=torch.zeros((F, HS, WS, C), dtype=torch.uint8), obj_class=(1, 255), depth_scale=None)


def _both(frames):
    """The two checks on the same observed frames -> their results, or the exceptions they raised."""
    from hotrack_amd.sdf import raycast_compare_check, tsdf_check
    depth, seg = frames["depth"], frames["seg"]
    vol = torch.zeros((5, 5, 5))
    calls = ((tsdf_check, (vol, torch.zeros((5, 5, 5)), 0.01, depth, seg, torch.zeros((F, 4)), torch.zeros((F, 3, 3)), torch.zeros((F, 3)), 0.03,
                           frames["obj_class"], frames["depth_scale"], 1.0, 64.0)),
             (raycast_compare_check, (torch.zeros(tuple(depth.shape)), depth, seg, frames["obj_class"], frames["depth_scale"], 0.01)))
    out = []
    for fn, args in calls:
        try:
            out.append(fn(*args))
        except (TypeError, ValueError) as e:
            out.append(e)
    return out


def _raw(scale_given=True):
    return dict(depth=torch.zeros((F, H, W), dtype=torch.int16), depth_scale=0.001 if scale_given else None)


SPOILED = [
    ("depth_dtype", TypeError, dict(depth=torch.zeros((F, H, W), dtype=torch.float64))),
    ("scale_for_fp32", TypeError, dict(depth_scale=0.001)),
    ("no_scale_for_uint16", TypeError, _raw(False)),
    ("scale_zero", ValueError, dict(_raw(), depth_scale=0.0)),
    ("scale_negative", ValueError, dict(_raw(), depth_scale=-0.001)),
    ("scale_inf", ValueError, dict(_raw(), depth_scale=float("inf"))),
    ("seg_rank", ValueError, dict(seg=torch.zeros((F, HS, WS), dtype=torch.uint8))),
    ("seg_frames", ValueError, dict(seg=torch.zeros((F + 1, HS, WS, C), dtype=torch.uint8))),
    ("two_channels", ValueError, dict(seg=torch.zeros((F, HS, WS, 2), dtype=torch.uint8))),
    ("unequal_factors", ValueError, dict(seg=torch.zeros((F, HS, WS // 2, C), dtype=torch.uint8))),
    ("h_not_a_multiple", ValueError, dict(seg=torch.zeros((F, 3, WS, C), dtype=torch.uint8))),
    ("channel_is_c", ValueError, dict(obj_class=(C, 255))),
    ("value_256", ValueError, dict(obj_class=(1, 256))),
    # the smallest frames that reach the limit: 65536 images of one pixel
    ("frames_65536", ValueError, dict(depth=torch.zeros((65536, 1, 1)), seg=torch.zeros((65536, 1, 1, 1), dtype=torch.uint8), obj_class=(0, 1))),
]


@pytest.mark.parametrize("what,error,spoil", SPOILED, ids=[s[0] for s in SPOILED])
def test_both_checks_refuse_in_the_same_words(what, error, spoil):
    fusion, compare = _both(dict(_good(), **spoil))
    assert type(fusion) is error and type(compare) is error, (fusion, compare)
    a, b = str(fusion), str(compare)
    assert a.startswith("tsdf_integrate: ") and b.startswith("raycast_compare: ")
    assert a[len("tsdf_integrate: "):] == b[len("raycast_compare: "):]


def test_both_checks_accept_the_same_frames():
    fusion, compare = _both(_good())
    assert compare == (F, H, W, HS, WS, C, 2, False) and fusion == (5,) + compare
    fusion, compare = _both(dict(_good(), **_raw()))
    assert compare == (F, H, W, HS, WS, C, 2, True) and fusion == (5,) + compare
