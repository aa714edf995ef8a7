"""GPU: the search-and-blend launch of feature propagation over listed query rows only (ext.three_nn_interpolate_pm(rows=...),
pn2x_three_nn_interpolate_pm_rows; three_nn_interp_kernel<true> in hotrack_amd/csrc/nn_search.hip).

`out` is a column block of a wider buffer filled with a sentinel: every listed row must hold the bits the full launch writes
there, every other row and every column around the block must still hold the sentinel.  The lists have the layout of
ext.row_lists -- two ascending segments, the second starting below the end of the first -- with the entries past a cloud's count
set to a row number far outside the cloud, which the kernel must never read."""
import os
import sys

import pytest
import torch

from _netinit import deterministic_init, make_cfg, synthetic_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
UNWRITTEN = 1 << 30  # list entries past the count
PAD, OFF = 8, 4      # the block sits at columns OFF .. OFF + C of rows of C + PAD floats (16-byte aligned, as fp1_in's is)


def _problem(B, N, m, C, seed):
    g = torch.Generator().manual_seed(seed)
    unknown = torch.rand(B, N, 3, generator=g).cuda()
    known = torch.rand(B, m, 3, generator=g).cuda()
    points = torch.randn(B, m, C, generator=g).cuda()
    return unknown, known, points


def _two_segments(N, g, frac):
    """A row_lists-style list of about frac * N distinct rows: an ascending segment, then a second ascending segment whose
    first entry lies below the first segment's last."""
    k = max(1, min(N, int(round(frac * N))))
    rows = torch.randperm(N, generator=g)[:k]
    cut = k // 3
    first, second = rows[:cut].sort().values, rows[cut:].sort().values
    return torch.cat([first, second]), cut


def _lists(B, N, kinds, seed):
    """kinds[b] in {"none", "all", "two"} -> (lst (B,N), counts (B,2)) on the GPU and the listed rows per cloud."""
    g = torch.Generator().manual_seed(seed)
    lst = torch.full((B, N), UNWRITTEN, dtype=torch.int32)
    counts = torch.zeros((B, 2), dtype=torch.int32)
    listed = []
    for b, kind in enumerate(kinds):
        if kind == "none":
            rows, cut = torch.empty(0, dtype=torch.long), 0
        elif kind == "all":
            rows, cut = _two_segments(N, g, 1.0)
        else:
            rows, cut = _two_segments(N, g, 0.6)
        lst[b, :rows.numel()] = rows.int()
        counts[b, 0], counts[b, 1] = cut, rows.numel()
        listed.append(rows)
    return lst.cuda(), counts.cuda(), listed


def _buffer(B, N, C):
    return torch.full((B, N, C + PAD), SENTINEL, device="cuda")


def _compare(buf, full, listed, C, what):
    B, N, _ = buf.shape
    mask = torch.zeros((B, N), dtype=torch.bool)
    for b, rows in enumerate(listed):
        mask[b, rows] = True
    mask = mask.cuda()
    block = buf[:, :, OFF:OFF + C]
    assert torch.equal(block[mask], full[:, :, OFF:OFF + C][mask]), f"{what}: a listed row differs from the full launch"
    assert bool((block[~mask] == SENTINEL).all()), f"{what}: a row no list names was written"
    assert bool((buf[:, :, :OFF] == SENTINEL).all()) and bool((buf[:, :, OFF + C:] == SENTINEL).all()), f"{what}: columns around the block were written"


# B * N = 16384: from there the full launch is the one-launch kernel too (below it, search and blend are two launches)
SHAPES = [(B, N, m, C) for B in (1, 3) for N in (7, 64, 1000) for m in (5, 256) for C in (4, 128)] + [(16, 1024, 256, 128)]


@pytest.mark.parametrize("B,N,m,C", SHAPES)
def test_listed_rows_equal_the_full_launch_and_nothing_else_is_written(B, N, m, C):
    from hotrack_amd import ext
    unknown, known, points = _problem(B, N, m, C, 100 + B + N + m + C)
    full = _buffer(B, N, C)
    ext.three_nn_interpolate_pm(unknown, known, points, full[:, :, OFF:OFF + C])
    assert bool((full[:, :, OFF:OFF + C] != SENTINEL).all())
    # one cloud without a listed row, one with every row listed, one with a two-segment list; a single cloud takes each in turn
    base = ("none", "all", "two")
    mixes = [[k] for k in base] if B == 1 else [[base[(b + r) % 3] for b in range(B)] for r in range(3)]
    for r, kinds in enumerate(mixes):
        lst, counts, listed = _lists(B, N, kinds, 7 * r + N)
        buf = _buffer(B, N, C)
        out = ext.three_nn_interpolate_pm(unknown, known, points, buf[:, :, OFF:OFF + C], rows=(lst, counts))
        assert out.data_ptr() == buf[:, :, OFF:OFF + C].data_ptr()
        _compare(buf, full, listed, C, f"{(B, N, m, C)} {kinds}")


def test_capture_on_one_list_and_replay_on_another():
    from hotrack_amd import ext
    B, N, m, C = 3, 1000, 256, 128
    unknown, known, points = _problem(B, N, m, C, 5)
    full = _buffer(B, N, C)
    ext.three_nn_interpolate_pm(unknown, known, points, full[:, :, OFF:OFF + C])
    lst_s, cnt_s, _ = _lists(B, N, ["none", "none", "two"], 1)
    buf = _buffer(B, N, C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the kernel has run once before the capture
        ext.three_nn_interpolate_pm(unknown, known, points, buf[:, :, OFF:OFF + C], rows=(lst_s, cnt_s))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ext.three_nn_interpolate_pm(unknown, known, points, buf[:, :, OFF:OFF + C], rows=(lst_s, cnt_s))
    for r, kinds in enumerate((["all", "two", "none"], ["two", "all", "two"], ["none", "none", "none"])):
        lst, counts, listed = _lists(B, N, kinds, 50 + r)
        lst_s.copy_(lst)
        cnt_s.copy_(counts)
        buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        _compare(buf, full, listed, C, f"replay on {kinds}")


def test_fast_path_interpolates_the_listed_rows_only():
    """FastEval at 32 x 1024 with the deterministic weights, large-batch route: with fp1's interpolation over the listed rows the
    row chain's output on the listed rows and pred_kp equal, bit for bit, those of the same forward with the interpolation over
    every row; and pred_kp stays within the 2e-5 of tests/test_gpu_row_chain.py of the route without the row chain."""
    from hotrack_amd import ext, fused, pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    pointnet_utils.set_operator_backend(pointnet2_utils)
    torch.manual_seed(0)
    model = HandTrackNet(make_cfg("cuda"))
    deterministic_init(model)
    model = model.cuda().eval()
    B, Np = 32, 1024
    d = synthetic_frames(920, B, Np)
    d = {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in d.items()}
    flags = {"track_flag": False, "test_flag": True, "save_flag": False, "IKNet_flag": False}
    real_interp, real_chain = ext.three_nn_interpolate_pm, ext.row_chain
    seen, chains = [], []

    def interp(*a, rows=None, full=False, **kw):
        seen.append(rows is not None)
        return real_interp(*a, rows=None if full else rows, **kw)

    def chain(x, lst, counts, *a, **kw):
        out = real_chain(x, lst, counts, *a, **kw)
        chains.append((lst.clone(), counts.clone(), out.clone()))
        return out

    try:
        pointnet_utils.set_fused_backend(fused)
        ext.row_chain = chain
        with torch.no_grad():
            ext.three_nn_interpolate_pm = interp
            a = model(d, dict(flags))
            assert model._fast is not None and model._fast._large_batch(B, Np) and model._fast.P["row_chain"] is not None
            ext.three_nn_interpolate_pm = lambda *x, **kw: interp(*x, full=True, **kw)
            b = model(d, dict(flags))
            ext.three_nn_interpolate_pm = real_interp
            model._fast.row_chain = False
            c = model(d, dict(flags))
            model._fast.row_chain = True
    finally:
        ext.three_nn_interpolate_pm, ext.row_chain = real_interp, real_chain
        pointnet_utils.set_fused_backend(None)
    assert seen == [False, True, False, True], seen  # fp2 over every row, fp1 over the listed rows, in both forwards
    assert len(chains) == 2
    (lst, counts, out_a), (lst_b, counts_b, out_b) = chains
    assert torch.equal(counts, counts_b)
    mask = torch.zeros((B, Np), dtype=torch.bool, device="cuda")
    for i in range(B):
        mask[i, lst[i, :int(counts[i, 1])].long()] = True
    assert 0 < int(mask.sum()) < B * Np
    small = torch.zeros_like(mask)
    for i in range(B):
        small[i, lst[i, :int(counts[i, 0])].long()] = True
    # rows of a K = 16 list hold all four column blocks, the others the K = 64 scale's (the last half of the columns)
    half = out_a.shape[2] // 2
    assert torch.equal(out_a[small], out_b[small]) and torch.equal(out_a[mask][:, half:], out_b[mask][:, half:]), "a_all differs on listed rows"
    assert torch.equal(a["pred_kp"], b["pred_kp"]), float((a["pred_kp"] - b["pred_kp"]).abs().max())
    err = float((a["pred_kp"] - c["pred_kp"]).abs().max())
    assert err <= 2e-5, err
