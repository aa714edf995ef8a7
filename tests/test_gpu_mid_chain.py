"""GPU: sa3 and fp3 as row-tiled chains (pn2x_sa3_chain / pn2x_fp3_chain, hotrack_amd/csrc/mid_chain.hip) against fp64 torch,
and the fast path on the chain route against the library route."""
import os
import sys

import pytest
import torch

from _netinit import deterministic_init, make_cfg, synthetic_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
S = 128


def _lin(g, o, i):
    # BatchNorm-folded-like weights: a per-output-channel scale on top of 1/sqrt(fan-in)
    scale = 0.5 + torch.rand(o, 1, generator=g)
    return (torch.randn(o, i, generator=g) / i ** 0.5 * scale).cuda(), (torch.randn(o, generator=g) * 0.1).cuda()


def _weights(g):
    sa3 = [_lin(g, 128, 131), _lin(g, 128, 128), _lin(g, 512, 128)]
    wg, bg = _lin(g, 256, 512)
    wa, _ = _lin(g, 256, 128)
    wf, bf = _lin(g, 256, 256)
    return sa3, (wg, bg, wa, wf, bf)


def _inputs(g, B, tied=False):
    x = torch.randn(B, S, 132, generator=g)
    if tied:
        x[:, S // 2:] = x[:, : S - S // 2]  # duplicated rows: each maximum is reached twice
        x[0] = x[0, :1]                      # one cloud of one repeated row
    x[:, :, 131] = float("nan")  # the pad float is never read
    return x.cuda()


def _ref_sa3(x, sa3):
    h = x[..., :131].double()
    for W, b in sa3:
        h = torch.relu(h @ W.double().t() + b.double())
    return h  # (B, S, 512) per row


def _ref_fp3(x, l3, fp3):
    wg, bg, wa, wf, bf = (t.double() for t in fp3)
    g = l3.double() @ wg.t() + bg
    h = torch.relu(x[..., :128].double() @ wa.t() + g[:, None, :])
    return torch.relu(h @ wf.t() + bf)


def _run_sa3(x, sa3):
    from hotrack_amd import ext
    p = ext.row_chain_pack
    return ext.sa3_chain(x, *[t for W, b in sa3 for t in (p(W), b)])


def _run_fp3(x, part, fp3, out=None):
    from hotrack_amd import ext
    wg, bg, wa, wf, bf = fp3
    p = ext.row_chain_pack
    return ext.fp3_chain(x, part, wg.t().contiguous(), bg, p(wa), p(wf), bf, out=out)


@pytest.mark.parametrize("B,tied", [(1, False), (3, False), (64, False), (130, False), (5, True)])
def test_sa3_chain_matches_fp64(B, tied):
    g = torch.Generator().manual_seed(B * 7 + tied)
    sa3, _ = _weights(g)
    x = _inputs(g, B, tied)
    from hotrack_amd import ext
    T = ext.MID_CHAIN_TILE
    part = torch.full((B, S // T, 512), SENTINEL, device="cuda")
    ext.sa3_chain(x, *[t for W, b in sa3 for t in (ext.row_chain_pack(W), b)], part=part)
    torch.cuda.synchronize()
    y = _ref_sa3(x, sa3).view(B, S // T, T, 512).amax(dim=2).float()  # per-tile maxima
    assert torch.allclose(part, y, atol=2e-5, rtol=1e-5), float((part - y).abs().max())
    again = _run_sa3(x, sa3)
    assert torch.equal(part, again)  # two launches: bit-identical


@pytest.mark.parametrize("B,tied", [(1, False), (3, False), (64, False), (130, False), (5, True)])
def test_fp3_chain_matches_fp64(B, tied):
    g = torch.Generator().manual_seed(B * 11 + tied)
    sa3, fp3 = _weights(g)
    x = _inputs(g, B, tied)
    part = _run_sa3(x, sa3)
    l3 = part.double().amax(dim=1)
    ref = _ref_fp3(x, l3, fp3).float()
    ob = torch.full((B, S, 264), SENTINEL, device="cuda")  # wider row stride than needed
    out = _run_fp3(x, part, fp3, out=ob[:, :, :256])
    torch.cuda.synchronize()
    assert torch.allclose(out, ref, atol=2e-5, rtol=1e-5), float((out - ref).abs().max())
    assert bool((ob[:, :, 256:] == SENTINEL).all())  # columns past 256 untouched
    again = _run_fp3(x, part, fp3)
    assert torch.equal(out, again)  # two launches: bit-identical


def test_sa3_fp3_chain_end_to_end_against_fp64():
    """The two launches together, from sa3's input rows to fp3's output, against the fp64 chain with the exact max over rows."""
    g = torch.Generator().manual_seed(5)
    sa3, fp3 = _weights(g)
    x = _inputs(g, 64)
    out = _run_fp3(x, _run_sa3(x, sa3), fp3)
    ref = _ref_fp3(x, _ref_sa3(x, sa3).amax(dim=1), fp3).float()
    assert torch.allclose(out, ref, atol=2e-5, rtol=1e-5), float((out - ref).abs().max())


def _model():
    from hotrack_amd import pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    pointnet_utils.set_operator_backend(pointnet2_utils)
    torch.manual_seed(0)
    model = HandTrackNet(make_cfg("cuda"))
    deterministic_init(model)
    return model.cuda().eval()


@pytest.mark.parametrize("B,N,dup", [(64, 1024, False), (64, 1024, True), (33, 1024, False)])
def test_fast_path_mid_chain_matches_library_route(B, N, dup):
    from hotrack_amd import fused
    from models import pointnet_utils
    model = _model()
    d = synthetic_frames(700 + B, B, N)
    if dup:
        d["hand_points"][:, N // 2:] = d["hand_points"][:, : N - N // 2]
    d = {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in d.items()}
    flags = {"track_flag": False, "test_flag": True, "save_flag": False, "IKNet_flag": False}
    try:
        pointnet_utils.set_fused_backend(fused)
        with torch.no_grad():
            a = model(d, dict(flags))
            assert model._fast is not None and model._fast.P["mid_chain"] is not None
            model._fast.row_chain = False
            b = model(d, dict(flags))
            model._fast.row_chain = True
    finally:
        pointnet_utils.set_fused_backend(None)
    err = float((a["pred_kp"] - b["pred_kp"]).abs().max())
    assert err <= 2e-5, err
