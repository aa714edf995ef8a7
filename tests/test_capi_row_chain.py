"""CPU: argument validation of pn2x_row_lists / pn2x_row_chain (include/pn2_ext.h) -- rejected before anything touches the device."""
import ctypes


def test_row_chain_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.pn2x_row_lists.argtypes = [ci] * 5 + [vp] * 5
    assert lib.pn2x_row_lists(2, 1024, 21, 64, 16, None, None, None, None, None) == -2     # NULL pointers
    assert lib.pn2x_row_lists(0, 1024, 21, 64, 16, None, None, None, None, None) == 0      # empty batch is a no-op
    assert lib.pn2x_row_lists(-1, 1024, 21, 64, 16, None, None, None, None, None) == -1    # b < 0
    assert lib.pn2x_row_lists(2, 1024, 21, 16, 64, None, None, None, None, None) == -1     # k_small > k_large
    assert lib.pn2x_row_lists(2, 16385, 21, 64, 16, None, None, None, None, None) == -3    # n beyond the LDS bitmap
    lib.pn2x_row_chain_supported.argtypes = [ci] * 4
    assert lib.pn2x_row_chain_supported(128, 128, 384, 512) == 1
    assert lib.pn2x_row_chain_supported(128, 128, 256, 512) == 0
    lib.pn2x_row_chain.argtypes = [ci, ci, vp, ci, vp, vp] + [vp] * 7 + [vp, ci, ci, vp]
    nul = [None] * 7
    assert lib.pn2x_row_chain(2, 1024, None, 132, None, None, *nul, None, 512, 0, None) == -2  # NULL pointers
    assert lib.pn2x_row_chain(0, 1024, None, 132, None, None, *nul, None, 512, 0, None) == 0   # empty batch is a no-op
    assert lib.pn2x_row_chain(2, 1024, None, 128, None, None, *nul, None, 512, 0, None) == -1  # ldx < 132
    assert lib.pn2x_row_chain(2, 1024, None, 132, None, None, *nul, None, 510, 0, None) == -1  # ldo < 512 / not a multiple of 4
    assert lib.pn2x_row_chain(2, 1024, None, 134, None, None, *nul, None, 512, 0, None) == -1  # ldx not a multiple of 4
    assert lib.pn2x_row_chain(2, 1024, None, 132, None, None, *nul, None, 512, -1, None) == -1  # grid < 0
    assert lib.pn2x_row_chain(1025, 1024, None, 132, None, None, *nul, None, 512, 0, None) == -3  # b beyond the LDS prefix arrays
