"""CPU: the host side of FastEval.fold_interp (network/models/fast_eval.py) -- the weight split of fp1's first layer in prepare()
and the argument validation of pn2x_row_chain3 / pn2x_three_nn_interpolate_pm_rows_act (include/pn2_ext.h), which reject bad
arguments before anything touches the device."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
from _netinit import deterministic_init, make_cfg  # noqa: E402


def _prepared(fold):
    from models.fast_eval import FastEval
    from models.hand_network import HandTrackNet
    torch.manual_seed(0)
    net = HandTrackNet(make_cfg("cpu"))
    deterministic_init(net)
    net = net.eval()
    before = FastEval.fold_interp
    try:
        FastEval.fold_interp = fold
        return net, FastEval(net).prepare()
    finally:
        FastEval.fold_interp = before


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_prepare_splits_fp1_first_layer_and_keeps_every_other_entry():
    from hotrack_amd import ext
    from hotrack_amd.fused import fold_conv_bn
    net, P = _prepared(True)
    fi, rc = P["fold_interp"], P["row_chain"]
    assert fi is not None and rc is not None
    W, b = fold_conv_bn(net.bhand.fp1.mlp_convs[0], net.bhand.fp1.mlp_bns[0])  # the module's layer: input [xyz | interp]
    assert fi["wa_x"].shape == (W.shape[0], 3) and fi["wa_f"].shape == (W.shape[0], W.shape[1] - 3)
    assert torch.equal(torch.cat([fi["wa_x"], fi["wa_f"]], dim=1), W) and torch.equal(fi["ba"], b)
    # ... and, re-concatenated in the fast path's order, the four-layer chain's own first layer
    assert torch.equal(torch.cat([fi["wa_f"], fi["wa_x"]], dim=1), P["fp1"][0][0])
    assert torch.equal(ext.row_chain_pack(torch.cat([fi["wa_f"], fi["wa_x"]], dim=1)), rc["wa"])
    assert fi["wa_f"].is_contiguous() and fi["wa_x"].is_contiguous()
    # the switch changes which launches run, not what prepare() holds
    _, Q = _prepared(False)
    assert P.keys() == Q.keys()
    for k in P:
        assert _same(P[k], Q[k]), k


def test_row_chain3_and_interpolation_epilogue_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.pn2x_row_chain3_supported.argtypes = [ci] * 3
    assert lib.pn2x_row_chain3_supported(128, 384, 512) == 1
    assert lib.pn2x_row_chain3_supported(128, 256, 512) == 0 and lib.pn2x_row_chain3_supported(132, 384, 512) == 0
    lib.pn2x_row_chain3.argtypes = [ci, ci, vp, ci, vp, vp] + [vp] * 5 + [vp, ci, ci, vp]
    nul = [None] * 5
    assert lib.pn2x_row_chain3(2, 1024, None, 128, None, None, *nul, None, 512, 0, None) == -2  # NULL pointers
    assert lib.pn2x_row_chain3(0, 1024, None, 128, None, None, *nul, None, 512, 0, None) == 0   # empty batch is a no-op
    assert lib.pn2x_row_chain3(2, 1024, None, 124, None, None, *nul, None, 512, 0, None) == -1  # ldh < 128
    assert lib.pn2x_row_chain3(2, 1024, None, 130, None, None, *nul, None, 512, 0, None) == -1  # ldh not a multiple of 4
    assert lib.pn2x_row_chain3(2, 1024, None, 128, None, None, *nul, None, 510, 0, None) == -1  # ldo < 512 / not a multiple of 4
    assert lib.pn2x_row_chain3(2, 1024, None, 128, None, None, *nul, None, 512, -1, None) == -1  # grid < 0
    assert lib.pn2x_row_chain3(1025, 1024, None, 128, None, None, *nul, None, 512, 0, None) == -3  # b beyond the LDS prefix arrays
    lib.pn2x_three_nn_interpolate_pm_rows_act_supported.argtypes = [ci] * 6
    sup = lib.pn2x_three_nn_interpolate_pm_rows_act_supported
    assert sup(64, 1024, 256, 128, 128, 128) == 1 and sup(1, 7, 3, 4, 4, 4) == 1 and sup(1, 64, 4, 1024, 1024, 1024) == 1
    assert sup(1, 64, 4, 1028, 1028, 1028) == 0 and sup(1, 64, 4, 6, 8, 8) == 0 and sup(1, 64, 2, 4, 4, 4) == 0
    assert sup(1, 64, 2049, 4, 4, 4) == 0 and sup(65536, 64, 4, 4, 4, 4) == 0
    lib.pn2x_three_nn_interpolate_pm_rows_act.argtypes = [ci, ci, ci, ci, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp]
    act = lib.pn2x_three_nn_interpolate_pm_rows_act
    assert act(2, 64, 4, 8, None, None, None, 8, None, 8, None, None, None, None, 1, None) == -2  # NULL pointers
    assert act(0, 64, 4, 8, None, None, None, 8, None, 8, None, None, None, None, 1, None) == 0   # empty batch is a no-op
    assert act(2, 64, 2, 8, None, None, None, 8, None, 8, None, None, None, None, 1, None) == -1  # fewer than 3 known points
    assert act(2, 64, 4, 8, None, None, None, 4, None, 8, None, None, None, None, 1, None) == -1  # ldp < c
