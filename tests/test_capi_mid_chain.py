"""CPU: argument validation of pn2x_sa3_chain / pn2x_fp3_chain (include/pn2_ext.h) -- rejected before anything touches the device."""
import ctypes


def test_mid_chain_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.pn2x_sa3_chain_supported.argtypes = [ci] * 5
    assert lib.pn2x_sa3_chain_supported(128, 128, 128, 128, 512) == 1
    assert lib.pn2x_sa3_chain_supported(192, 128, 128, 128, 512) == 1
    assert lib.pn2x_sa3_chain_supported(80, 128, 128, 128, 512) == 0    # a tile would span two clouds
    assert lib.pn2x_sa3_chain_supported(128, 256, 128, 128, 512) == 0   # widths the kernel does not implement
    assert lib.pn2x_sa3_chain_supported(128, 128, 128, 128, 1024) == 0
    lib.pn2x_fp3_chain_supported.argtypes = [ci] * 5
    assert lib.pn2x_fp3_chain_supported(128, 128, 512, 256, 256) == 1
    assert lib.pn2x_fp3_chain_supported(100, 128, 512, 256, 256) == 0
    assert lib.pn2x_fp3_chain_supported(96, 128, 512, 256, 256) == 1
    assert lib.pn2x_fp3_chain_supported(128, 128, 512, 256, 128) == 0
    assert lib.pn2x_fp3_chain_supported(0, 128, 512, 256, 256) == 0

    lib.pn2x_sa3_chain.argtypes = [ci, ci, vp, ci] + [vp] * 7 + [vp]
    nul = [None] * 6
    assert lib.pn2x_sa3_chain(2, 128, None, 132, *nul, None, None) == -2    # NULL pointers
    assert lib.pn2x_sa3_chain(0, 128, None, 132, *nul, None, None) == 0     # empty batch is a no-op
    assert lib.pn2x_sa3_chain(-1, 128, None, 132, *nul, None, None) == -1   # b < 0
    assert lib.pn2x_sa3_chain(2, 80, None, 132, *nul, None, None) == -1     # s not a multiple of the tile height
    assert lib.pn2x_sa3_chain(2, 0, None, 132, *nul, None, None) == -1      # s < 1
    assert lib.pn2x_sa3_chain(2, 128, None, 128, *nul, None, None) == -1    # ldx < 132
    assert lib.pn2x_sa3_chain(2, 128, None, 134, *nul, None, None) == -1    # ldx not a multiple of 4
    assert lib.pn2x_sa3_chain(1 << 24, 128, None, 132, *nul, None, None) == -3  # b * s beyond 2^31
    # misaligned pointers (never dereferenced: rejected before any launch)
    odd = [8, 16, 32, 48, 64, 80, 96]
    assert lib.pn2x_sa3_chain(2, 128, 4, 132, *odd[1:], 112, None) == -1

    lib.pn2x_fp3_chain.argtypes = [ci, ci, vp, ci] + [vp] * 6 + [vp, ci, vp]
    nul = [None] * 6
    assert lib.pn2x_fp3_chain(2, 128, None, 132, *nul, None, 256, None) == -2   # NULL pointers
    assert lib.pn2x_fp3_chain(0, 128, None, 132, *nul, None, 256, None) == 0    # empty batch is a no-op
    assert lib.pn2x_fp3_chain(-1, 128, None, 132, *nul, None, 256, None) == -1  # b < 0
    assert lib.pn2x_fp3_chain(2, 144, None, 132, *nul, None, 256, None) == -1   # s not a multiple of the tile height
    assert lib.pn2x_fp3_chain(2, 128, None, 124, *nul, None, 256, None) == -1   # ldx < 128
    assert lib.pn2x_fp3_chain(2, 128, None, 130, *nul, None, 256, None) == -1   # ldx not a multiple of 4
    assert lib.pn2x_fp3_chain(2, 128, None, 132, *nul, None, 252, None) == -1   # ldo < 256
    assert lib.pn2x_fp3_chain(2, 128, None, 132, *nul, None, 258, None) == -1   # ldo not a multiple of 4
    assert lib.pn2x_fp3_chain(1 << 24, 128, None, 132, *nul, None, 256, None) == -3  # b * s beyond 2^31
    assert lib.pn2x_fp3_chain(2, 128, 16, 132, 32, 48, 64, 80, 96, 100, 112, 256, None) == -1  # misaligned pointer
