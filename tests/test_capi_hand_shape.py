"""CPU: argument validation of pn2x_hand_shape_opt and the pn2x_hand_shape_opt_supported query (include/pn2_ext.h) --
rejected before anything touches the device."""
import ctypes


def test_hand_shape_opt_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    ci, vp, cd = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    lib.pn2x_hand_shape_opt_supported.argtypes = [ci] * 3
    assert lib.pn2x_hand_shape_opt_supported(5120, 10, 1) == 1
    assert lib.pn2x_hand_shape_opt_supported(8192, 16, 1024) == 1
    assert lib.pn2x_hand_shape_opt_supported(1, 1, 1) == 1
    assert lib.pn2x_hand_shape_opt_supported(8193, 10, 1) == 0   # more particles than LDS holds energies for
    assert lib.pn2x_hand_shape_opt_supported(5120, 17, 1) == 0   # more shape dimensions than the kernel carries
    assert lib.pn2x_hand_shape_opt_supported(5120, 10, 1025) == 0
    assert lib.pn2x_hand_shape_opt_supported(0, 10, 1) == 0
    assert lib.pn2x_hand_shape_opt_supported(5120, 0, 1) == 0
    assert lib.pn2x_hand_shape_opt_supported(5120, 10, 0) == 0

    lib.pn2x_hand_shape_opt.argtypes = [ci] * 4 + [vp] * 5 + [cd, cd, vp, vp, vp]
    f = lib.pn2x_hand_shape_opt
    one = 16  # never dereferenced: every call below is rejected (or a no-op) before any launch
    ok = [one] * 5
    assert f(5120, 10, 1, 20, *[None] * 5, 2000.0, 0.9, None, None, None) == -2   # NULL pointers
    assert f(5120, 10, 1, 20, *ok, 2000.0, 0.9, None, None, None) == -2           # NULL out
    assert f(5120, 10, 1, 20, one, None, one, one, one, 2000.0, 0.9, one, None, None) == -2
    assert f(5120, 10, 1, 0, *[None] * 5, 2000.0, 0.9, None, None, None) == 0     # no iterations: a no-op
    assert f(0, 10, 1, 20, *ok, 2000.0, 0.9, one, None, None) == -1              # P < 1
    assert f(5120, 0, 1, 20, *ok, 2000.0, 0.9, one, None, None) == -1            # D < 1
    assert f(5120, 10, 0, 20, *ok, 2000.0, 0.9, one, None, None) == -1           # T < 1
    assert f(5120, 10, 1, -1, *ok, 2000.0, 0.9, one, None, None) == -1           # iterations < 0
    assert f(8193, 10, 1, 20, *ok, 2000.0, 0.9, one, None, None) == -3           # P beyond 8192
    assert f(5120, 17, 1, 20, *ok, 2000.0, 0.9, one, None, None) == -3           # D beyond 16
    assert f(5120, 10, 1025, 20, *ok, 2000.0, 0.9, one, None, None) == -3        # T beyond 1024
    assert f(5120, 16, 1, 1 << 27, *ok, 2000.0, 0.9, one, one, None) == -3       # trace size beyond 2^31
