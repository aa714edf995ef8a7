"""GPU: the per-point chain over the kNN-listed rows (pn2x_row_lists + pn2x_row_chain, hotrack_amd/csrc/row_chain.hip) against
fp64 torch, and the fast path with the chain against the fast path on the over-points route."""
import os
import sys

import pytest
import torch

from _netinit import deterministic_init, make_cfg, synthetic_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _weights(g):
    def lin(o, i, s):
        return (torch.randn(o, i, generator=g) * s).cuda(), (torch.randn(o, generator=g) * 0.1).cuda()
    wa, ba = lin(128, 131, 0.1)
    wb, bb = lin(128, 128, 0.1)
    wc, bc = lin(384, 128, 0.1)
    wq = (torch.randn(512, 384, generator=g) * 0.05).cuda()
    return wa, ba, wb, bb, wc, bc, wq


def _reference(x, wa, ba, wb, bb, wc, bc, wq):
    d = lambda t: t.double()
    h = torch.relu(d(x[..., :131]) @ d(wa).t() + d(ba))
    h = torch.relu(h @ d(wb).t() + d(bb))
    c = torch.relu(h @ d(wc).t() + d(bc))
    return c @ d(wq).t()


def _run_chain(x, lst, counts, W, out):
    from hotrack_amd import ext
    wa, ba, wb, bb, wc, bc, wq = W
    p = ext.row_chain_pack
    return ext.row_chain(x, lst, counts, p(wa), ba, p(wb), bb, p(wc), bc, p(wq), out=out)


def _lists_from_sets(B, N, small_sets, any_sets):
    lst = torch.full((B, N), -7, dtype=torch.int32)
    counts = torch.zeros((B, 2), dtype=torch.int32)
    for b in range(B):
        s = sorted(small_sets[b])
        o = sorted(set(any_sets[b]) - set(small_sets[b]))
        lst[b, :len(s) + len(o)] = torch.tensor(s + o, dtype=torch.int32)
        counts[b, 0], counts[b, 1] = len(s), len(s) + len(o)
    return lst.cuda(), counts.cuda()


@pytest.mark.parametrize("B,N,mode", [(1, 1024, "random"), (33, 2048, "random"), (64, 1024, "random"), (64, 4096, "random"),
                                      (3, 1024, "empty"), (2, 1024, "all"), (5, 1000, "all_small"), (4, 16384, "random")])
def test_row_chain_matches_fp64_on_listed_rows_only(B, N, mode):
    g = torch.Generator().manual_seed(B * 31 + N)
    W = _weights(g)
    x = torch.randn(B, N, 132, generator=g).cuda()
    x[:, :, 131] = float("nan")  # the pad float is never read
    small, anyr = [], []
    for b in range(B):
        if mode == "empty":
            s, a = [], []
        elif mode == "all":
            s, a = [], list(range(N))
        elif mode == "all_small":
            s = a = list(range(N))
        else:
            a = torch.randperm(N, generator=g)[: int(torch.randint(0, N, (1,), generator=g))].tolist()
            s = a[: len(a) // 3]
        small.append(s)
        anyr.append(a)
    lst, counts = _lists_from_sets(B, N, small, anyr)
    out = torch.full((B, N, 512), SENTINEL, device="cuda")
    _run_chain(x, lst, counts, W, out)
    torch.cuda.synchronize()
    ref = _reference(x, *W)
    out = out.cpu().double()
    ref = ref.cpu()
    mask = torch.zeros(B, N, 512, dtype=torch.bool)
    for b in range(B):
        if small[b]:
            mask[b, torch.tensor(small[b]), :] = True
        if anyr[b]:
            mask[b, torch.tensor(anyr[b]), 256:] = True
    scale = max(1.0, float(ref.abs().max()))
    if mask.any():
        err = float((out[mask] - ref[mask]).abs().max())
        assert err <= 2e-5 * scale, err
    assert bool((out[~mask] == SENTINEL).all())


def test_row_lists_match_torch_unique():
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(3)
    B, J, N = 37, 21, 1024
    pts = torch.rand(B, N, 3, generator=g)
    pts[5, N // 2:] = pts[5, : N - N // 2]  # duplicated points: tied kNN distances
    pts[6] = pts[6, :1]  # one point repeated
    kp = torch.rand(B, J, 3, generator=g)
    gi, gis = ext.knn_indices(64, kp.cuda(), pts.cuda(), k2=16)
    for small in (gis, None):
        lst, counts = ext.row_lists(gi, small, N)
        lst, counts, gc = lst.cpu(), counts.cpu(), gi.cpu()
        gsc = (gis if small is not None else gi).cpu()
        for b in range(B):
            s = torch.unique(gsc[b])
            a = torch.unique(gc[b])
            o = a[~torch.isin(a, s)]
            assert int(counts[b, 0]) == s.numel() and int(counts[b, 1]) == s.numel() + o.numel()
            assert torch.equal(lst[b, : s.numel()].long(), s.long())
            assert torch.equal(lst[b, s.numel(): s.numel() + o.numel()].long(), o.long())


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
def test_fast_path_row_chain_matches_over_points_route(B, N, dup):
    from hotrack_amd import fused
    from models import pointnet_utils
    model = _model()
    d = synthetic_frames(500 + B, B, N)
    if dup:
        d["hand_points"][:, N // 2:] = d["hand_points"][:, : N - N // 2]
    d = {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in d.items()}
    flags = {"track_flag": False, "test_flag": True, "save_flag": False, "IKNet_flag": False}
    try:
        pointnet_utils.set_fused_backend(fused)
        with torch.no_grad():
            a = model(d, dict(flags))
            assert model._fast is not None and model._fast.P["row_chain"] is not None
            model._fast.row_chain = False
            b = model(d, dict(flags))
            model._fast.row_chain = True
    finally:
        pointnet_utils.set_fused_backend(None)
    err = float((a["pred_kp"] - b["pred_kp"]).abs().max())
    assert err <= 2e-5, err
