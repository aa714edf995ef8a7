"""CPU: the argument validation of pn2x_hand_interaction_metrics (include/pn2_ext.h) -- a bad value -1 before a limit -3 before a
NULL pointer -2, a record pointer below 64 KiB refused unread, f = 0 / s = 0 return the column mask without a launch -- before
anything touches the device."""
import ctypes

vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
EINVAL, ENULL, ERANGE = -1, -2, -3


class Setup(ctypes.Structure):
    """pn2x_hand_pose_setup (136 bytes)."""
    _fields_ = ([(n, vp) for n in ("parents", "pose_block", "skin_pack", "skin_w", "comps", "pre", "posedirs", "pose_mean", "kp_vertex")] +
                [(n, ci) for n in ("p", "v", "j", "k", "vol_f16", "res", "centre_root", "reserved")] +
                [(n, cf) for n in ("theta_scale", "voxel_scale", "w_sil", "w_pen", "w_vis", "w_invis", "w_temporal", "w_attr")])


ONE = 1 << 20  # a non-NULL address; nothing is read through it before the checks have passed, and nothing passes here with f > 0
ARRAYS = ("global_r", "global_t", "theta", "obj_r", "obj_t", "pred_kp", "rest_joints", "rest_verts", "rest_of", "vols", "seq_off")
OUTPUTS = ("rows", "seq", "out_verts", "out_kp")
OPTIONAL = ("pred_kp", "out_verts", "out_kp")


def _lib(path):
    lib = ctypes.CDLL(path)
    lib.pn2x_hand_interaction_metrics.argtypes = [ctypes.POINTER(Setup), ci, ci, ci] + [vp] * 11 + [cf] + [vp] * 5
    lib.pn2x_hand_interaction_metrics.restype = ci
    return lib


def _setup(**kw):
    s = Setup(parents=ONE, pose_block=ONE, skin_pack=ONE, skin_w=ONE, v=778, j=21, k=2, vol_f16=1, res=151, voxel_scale=0.003)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _call(lib, setup, f=0, s=0, g=1, thr=0.005, **ptrs):
    a = [ptrs.get(n, ONE) for n in ARRAYS]
    o = [ptrs.get(n, ONE) for n in OUTPUTS]
    rec = setup if not isinstance(setup, Setup) else ctypes.byref(setup)
    return lib.pn2x_hand_interaction_metrics(rec, f, s, g, *a, thr, *o, None)


def test_sizes_limits_and_the_record(hip_lib_path):
    lib = _lib(hip_lib_path)
    ok = _setup()
    assert ctypes.sizeof(Setup) == 136
    # nothing to do: the mask, with and without pred_kp; the arrays are not looked at; p, pre, comps and the weights are not read
    assert _call(lib, ok) == 0xff and _call(lib, ok, pred_kp=None) == 0xbf
    assert _call(lib, ok, f=0, s=3) == 0xff and _call(lib, ok, f=5, s=0, pred_kp=None) == 0xbf
    assert _call(lib, ok, **{n: None for n in ARRAYS + OUTPUTS}) == 0xbf
    assert _call(lib, ok, g=0) == 0xff   # no tables are needed without frames
    # bad values
    for kw in (dict(f=-1), dict(s=-1), dict(g=-1), dict(thr=-1e-6), dict(thr=float("nan"))):
        assert _call(lib, ok, **kw) == EINVAL, kw
    for kw in (dict(v=0), dict(j=0), dict(k=0), dict(res=0), dict(res=150), dict(voxel_scale=0.0), dict(voxel_scale=-1.0), dict(vol_f16=2)):
        assert _call(lib, _setup(**kw)) == EINVAL, kw
    assert _call(lib, _setup(posedirs=ONE, pose_mean=ONE, kp_vertex=ONE, centre_root=2)) == EINVAL
    assert _call(lib, _setup(posedirs=ONE + 4, pose_mean=ONE, kp_vertex=ONE)) == EINVAL   # 16-byte loads
    assert _call(lib, _setup(posedirs=ONE, pose_mean=ONE, kp_vertex=ONE, centre_root=1)) == 0xff
    # a record pointer below 64 KiB is what a size passed in its place looks like: refused, not read
    assert _call(lib, ctypes.cast(5120, ctypes.POINTER(Setup))) == EINVAL
    assert _call(lib, ctypes.cast(65535, ctypes.POINTER(Setup))) == EINVAL
    assert _call(lib, None) == ENULL
    # limits (pn2x_hand_pose_opt_supported's for v, j, k, res)
    for kw in (dict(v=1025), dict(j=20), dict(j=22), dict(k=5), dict(res=1025)):
        assert _call(lib, _setup(**kw)) == ERANGE, kw
    assert _call(lib, _setup(v=1024, k=4, res=1023)) == 0xff
    # NULL tables of the record, with nothing to do as well
    for n in ("parents", "pose_block", "skin_pack", "skin_w"):
        assert _call(lib, _setup(**{n: None})) == ENULL, n
    assert _call(lib, _setup(posedirs=ONE, pose_mean=None, kp_vertex=ONE)) == ENULL
    assert _call(lib, _setup(posedirs=ONE, pose_mean=ONE, kp_vertex=None)) == ENULL
    assert _call(lib, _setup(comps=None, pre=None, p=0)) == 0xff   # the fields the entry does not read


def test_the_order_of_the_codes_and_the_arrays(hip_lib_path):
    lib = _lib(hip_lib_path)
    ok = _setup()
    # with frames to evaluate every array but the three optional ones must be there
    for n in ARRAYS + OUTPUTS:
        if n not in OPTIONAL:
            assert _call(lib, ok, f=4, s=2, **{n: None}) == ENULL, n
    assert _call(lib, ok, f=4, s=2, g=0) == EINVAL                                        # frames and no shape table
    # PN2_EINVAL before PN2_ERANGE before PN2_ENULL, whichever argument carries them
    assert _call(lib, _setup(v=1025), f=4, s=2, rows=None) == ERANGE
    assert _call(lib, _setup(v=1025, parents=None)) == ERANGE
    assert _call(lib, _setup(v=1025), thr=-1.0) == EINVAL
    assert _call(lib, _setup(res=150, k=5), f=4, s=2, theta=None) == EINVAL
    assert _call(lib, _setup(parents=None), f=-1) == EINVAL
    assert _call(lib, None, f=-1) == EINVAL and _call(lib, None, f=4, s=2, rows=None) == ENULL
    assert _call(lib, ctypes.cast(4096, ctypes.POINTER(Setup)), f=4, s=2, rows=None) == EINVAL
