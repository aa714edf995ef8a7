"""CPU: the argument validation of the sequence-evaluation entries (include/pn2_ext.h: pn2x_posed_chamfer,
pn2x_obj_pose_metrics) -- bad sizes -1, NULL pointers -2, an empty sequence is a no-op -- before anything touches the device."""
import ctypes

vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long


def _lib(path):
    lib = ctypes.CDLL(path)
    lib.pn2x_posed_chamfer_partial_floats.argtypes = [ci, ci, ci]
    lib.pn2x_posed_chamfer_partial_floats.restype = cl
    lib.pn2x_posed_chamfer.argtypes = [ci, ci, ci] + [vp] * 7 + [cl, vp, vp]
    lib.pn2x_posed_chamfer.restype = ci
    lib.pn2x_obj_pose_metrics.argtypes = [ci, vp, vp, vp, vp, ci, ci, vp, vp]
    lib.pn2x_obj_pose_metrics.restype = ci
    return lib


def test_posed_chamfer_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    one = vp(16)
    ptrs = [one] * 7
    call = lambda n, m, t, p=ptrs, floats=1 << 20, out=one: lib.pn2x_posed_chamfer(n, m, t, *p, floats, out, None)
    assert call(-1, 8, 2) == -1 and call(8, -1, 2) == -1 and call(8, 8, -1) == -1   # negative sizes
    assert call(0, 8, 2) == -1 and call(8, 0, 2) == -1                                  # an empty cloud with frames to evaluate
    assert call(0, 0, 0) == 0 and call(8, 8, 0, [None] * 7, 0, None) == 0               # no frames: a no-op, nothing is read
    assert call(8, 8, 2, [None] * 7) == -2                                              # NULL pointers
    for i in range(7):
        assert call(8, 8, 2, [None if j == i else one for j in range(7)]) == -2
    assert call(8, 8, 2, out=None) == -2
    # the scratch the caller hands over: one float per (frame, 512-point tile of either cloud)
    assert lib.pn2x_posed_chamfer_partial_floats(2048, 2048, 3) == 3 * 8
    assert lib.pn2x_posed_chamfer_partial_floats(1, 513, 5) == 5 * 3
    assert lib.pn2x_posed_chamfer_partial_floats(8, 8, 0) == 0 and lib.pn2x_posed_chamfer_partial_floats(-1, 8, 1) == -1
    assert call(2048, 2048, 3, floats=23) == -4                                         # scratch too small
    assert call(1 << 25, 8, 1) == -3                                                    # more tiles than a grid dimension holds


def test_obj_pose_metrics_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    one = vp(16)
    assert lib.pn2x_obj_pose_metrics(-1, one, one, one, one, 0, 0, one, None) == -1
    assert lib.pn2x_obj_pose_metrics(0, None, None, None, None, 0, 0, None, None) == 0
    for i in range(5):
        p = [None if j == i else one for j in range(5)]
        assert lib.pn2x_obj_pose_metrics(4, p[0], p[1], p[2], p[3], -1, 0, p[4], None) == -2
