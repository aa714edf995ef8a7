"""GPU: fp1's first layer taken before the interpolation (FastEval.fold_interp, network/models/fast_eval.py).

Interpolation is a convex combination of rows, so it commutes with a linear map: W (sum_i w_i f[n_i]) = sum_i w_i (W f)[n_i].
The folded route applies the feature block of fp1's first layer to the level-1 rows, lets the listed-rows interpolation finish the
layer in its epilogue (pn2x_three_nn_interpolate_pm_rows_act, hotrack_amd/csrc/nn_search.hip) and starts the row chain at fp1's
second layer (pn2x_row_chain3, hotrack_amd/csrc/row_chain.hip).

Order of the epilogue's sum, per channel: the blend as the plain listed-rows kernel forms it, fma(w2, p2, fma(w0, p0, w1 * p1));
then fma(Wx[ch][0], x, .), fma(Wx[ch][1], y, .), fma(Wx[ch][2], z, .); then + bias[ch]; then max(., 0) when relu is set.  With
Wx = 0 and bias = 0 every added term is an exact zero, so the result must equal the plain kernel's (torch.equal).

Bounds.  Both kernels against float64 at atol = rtol = 2e-5 x scale, scale = max(1, max |reference|): the bound of
tests/test_gpu_row_chain_bits.py.  row_chain3 fed with the float64 first layer (rounded once to float32) against the four-layer
ext.row_chain: each is within its own 2e-5 x scale of float64, so they are within 4e-5 x scale of each other.  Routes: the folded
route's worst |pred_kp - float64 module path| may be at most twice the unfolded route's (the spread between routes recorded in
profiles/r12_tail_perm.md, 2.5e-6 to 4.2e-6), and both stay below 2e-5."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
from _netinit import synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
UNWRITTEN = 1 << 30  # list entries past a cloud's count: a row far outside the cloud, never read
COUNTS = ((0, 0), (1, 0), (0, 1), (15, 17))  # (small, large-only) listed rows of a cloud; (N, 0) is added per shape


def _count_mixes(B, N):
    """Per-cloud (small, large-only) counts: a single cloud takes each pair in turn, three clouds take them three at a time."""
    ps = list(COUNTS) + [(N, 0)]
    if B == 1:
        return [(p,) for p in ps]
    return [tuple(ps[(r + b) % len(ps)] for b in range(B)) for r in (0, 2, 3)]  # every pair at least once, (N,0) next to (0,0)


def _lists(B, N, pairs, seed):
    """row_lists-style lists: cloud b names pairs[b] distinct random rows, each part ascending.  -> lst, counts, listed (B,N) bool,
    small (B,N) bool (CPU masks)."""
    g = torch.Generator().manual_seed(seed)
    lst = torch.full((B, N), UNWRITTEN, dtype=torch.int32)
    counts = torch.zeros((B, 2), dtype=torch.int32)
    listed, small = torch.zeros(B, N, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)
    for b, (ns, nl) in enumerate(pairs):
        perm = torch.randperm(N, generator=g)
        s, o = perm[:ns].sort().values, perm[ns:ns + nl].sort().values
        lst[b, :ns + nl] = torch.cat([s, o]).int()
        counts[b, 0], counts[b, 1] = ns, ns + nl
        listed[b, s], listed[b, o], small[b, s] = True, True, True
    return lst.cuda(), counts.cuda(), listed, small


# ---- the interpolation with the xyz / bias / ReLU epilogue ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _interp_problem(B, N, S, C):
    """Inputs on the GPU and the float64 result of every row with and without ReLU (CPU), computed once per shape.  Query 0 of
    every cloud coincides with known point S - 1 (distance exactly 0)."""
    g = torch.Generator().manual_seed(17 * B + N + 1000 * S + C)
    unknown = torch.rand(B, N, 3, generator=g)
    known = torch.rand(B, S, 3, generator=g)
    unknown[:, 0] = known[:, S - 1]
    points = torch.randn(B, S, C, generator=g)
    wx = torch.randn(C, 3, generator=g) * 0.5
    bias = torch.randn(C, generator=g) * 0.1
    u, k = unknown.double(), known.double()
    d2 = ((u[:, :, None, :] - k[:, None, :, :]) ** 2).sum(-1)
    d3, i3 = torch.sort(d2, dim=2, stable=True)  # ties keep the lower index
    d3, i3 = d3[:, :, :3], i3[:, :, :3]
    r = 1.0 / (d3.sqrt() + 1e-8)
    w = r / r.sum(dim=2, keepdim=True)
    rows = torch.gather(points.double()[:, None].expand(B, N, S, C), 2, i3[..., None].expand(B, N, 3, C))
    blend = (w[..., None] * rows).sum(dim=2)
    lin = blend + u @ wx.double().t() + bias.double()
    return (unknown.cuda(), known.cuda(), points.cuda(), wx.cuda(), bias.cuda()), blend, lin


def _close(out, ref, mask, what):
    if mask.any():
        scale = max(1.0, float(ref.abs().max()))
        err = float((out.double()[mask] - ref[mask]).abs().max())
        print(f"{what}: max |err| vs fp64 = {err:.3e} (bound {2e-5 * scale:.3e})")
        assert err <= 2e-5 * scale, (what, err)


@pytest.mark.parametrize("C", [4, 128, 132])
@pytest.mark.parametrize("S", [3, 4, 256])
@pytest.mark.parametrize("N", [64, 1000])
@pytest.mark.parametrize("B", [1, 3])
def test_interpolation_epilogue_against_fp64(B, N, S, C):
    from hotrack_amd import ext
    (unknown, known, points, wx, bias), blend, lin = _interp_problem(B, N, S, C)
    zero_w, zero_b = torch.zeros_like(wx), torch.zeros_like(bias)
    pos = points.abs()
    for r, pairs in enumerate(_count_mixes(B, N)):
        lst, counts, listed, _ = _lists(B, N, pairs, 31 * r + N + S)
        if any(ns + nl for ns, nl in pairs):  # the coincident query is a listed row wherever a cloud lists any
            for b, (ns, nl) in enumerate(pairs):
                if ns + nl and not listed[b, 0]:
                    listed[b, int(lst[b, 0])] = False
                    lst[b, 0] = 0
                    listed[b, 0] = True
        what = f"{(B, N, S, C)} {pairs}"
        for relu in (True, False):
            out = torch.full((B, N, C + 8), SENTINEL, device="cuda")  # a column block of wider rows
            got = ext.three_nn_interpolate_pm(unknown, known, points, out[:, :, 4:4 + C], rows=(lst, counts), wx=wx, bias=bias, relu=relu)
            assert got.data_ptr() == out[:, :, 4:4 + C].data_ptr()
            out = out.cpu()
            assert bool((out[:, :, 4:4 + C][~listed] == SENTINEL).all()), f"{what}: a row no list names was written"
            assert bool((out[:, :, :4] == SENTINEL).all()) and bool((out[:, :, 4 + C:] == SENTINEL).all()), f"{what}: columns around the block"
            _close(out[:, :, 4:4 + C], torch.relu(lin) if relu else lin, listed, f"{what} relu={relu}")
        # Wx = 0, bias = 0: the plain listed-rows kernel's floats -- without ReLU on any input, with ReLU on non-negative rows
        plain = torch.full((B, N, C), SENTINEL, device="cuda")
        ext.three_nn_interpolate_pm(unknown, known, points, plain, rows=(lst, counts))
        same = torch.full((B, N, C), SENTINEL, device="cuda")
        ext.three_nn_interpolate_pm(unknown, known, points, same, rows=(lst, counts), wx=zero_w, bias=zero_b, relu=False)
        assert torch.equal(same, plain), f"{what}: zero epilogue differs from the plain kernel"
        _close(plain.cpu(), blend, listed, f"{what} plain")
        ext.three_nn_interpolate_pm(unknown, known, pos, plain, rows=(lst, counts))
        ext.three_nn_interpolate_pm(unknown, known, pos, same, rows=(lst, counts), wx=zero_w, bias=zero_b, relu=True)
        assert torch.equal(same, plain), f"{what}: zero epilogue with ReLU differs from the plain kernel on non-negative rows"


@pytest.mark.parametrize("B,N,S,C", [(1, 64, 3, 4), (3, 1000, 256, 132), (3, 7, 4, 128)])
def test_epilogue_without_a_list_writes_every_row_with_the_listed_launch_s_floats(B, N, S, C):
    from hotrack_amd import ext
    if (B, N) == (3, 7):  # fewer queries than a workgroup's 64 entries; the cached problems have N in {64, 1000}
        g = torch.Generator().manual_seed(77)
        unknown, known = torch.rand(B, N, 3, generator=g).cuda(), torch.rand(B, S, 3, generator=g).cuda()
        points, wx, bias = torch.randn(B, S, C, generator=g).cuda(), torch.randn(C, 3, generator=g).cuda(), torch.randn(C, generator=g).cuda()
        lin = None
    else:
        (unknown, known, points, wx, bias), _, lin = _interp_problem(B, N, S, C)
    every = torch.full((B, N, C + 8), SENTINEL, device="cuda")
    ext.three_nn_interpolate_pm(unknown, known, points, every[:, :, 4:4 + C], wx=wx, bias=bias, relu=True)
    assert bool((every[:, :, :4] == SENTINEL).all()) and bool((every[:, :, 4 + C:] == SENTINEL).all())
    lst = torch.arange(N, dtype=torch.int32).repeat(B, 1).cuda()
    counts = torch.tensor([[0, N]] * B, dtype=torch.int32).cuda()
    listed = torch.full((B, N, C + 8), SENTINEL, device="cuda")
    ext.three_nn_interpolate_pm(unknown, known, points, listed[:, :, 4:4 + C], rows=(lst, counts), wx=wx, bias=bias, relu=True)
    assert torch.equal(every, listed)
    if lin is not None:
        _close(every[:, :, 4:4 + C].cpu(), torch.relu(lin), torch.ones(B, N, dtype=torch.bool), f"every row {(B, N, S, C)}")


def test_interpolation_epilogue_refuses_what_it_does_not_cover():
    from hotrack_amd import ext
    B, N, S, C = 1, 64, 4, 8
    (unknown, known, points, wx, bias), _, _ = _interp_problem(B, N, S, C)
    lst, counts, _, _ = _lists(B, N, ((15, 17),), 3)
    out = torch.full((B, N, C), SENTINEL, device="cuda")
    ok = dict(rows=(lst, counts), wx=wx, bias=bias, relu=True)
    ext.three_nn_interpolate_pm(unknown, known, points, out, **ok)
    with pytest.raises(ValueError):  # wx without bias
        ext.three_nn_interpolate_pm(unknown, known, points, out, rows=(lst, counts), wx=wx)
    with pytest.raises(ValueError):  # wx of another width
        ext.three_nn_interpolate_pm(unknown, known, points, out, **{**ok, "wx": torch.zeros(C + 4, 3, device="cuda")})
    off = torch.zeros(C * 3 + 1, device="cuda")[1:].view(C, 3)  # 4 bytes past a 16-byte boundary
    with pytest.raises(ValueError):
        ext.three_nn_interpolate_pm(unknown, known, points, out, **{**ok, "wx": off})
    offb = torch.zeros(C + 1, device="cuda")[1:]
    with pytest.raises(ValueError):
        ext.three_nn_interpolate_pm(unknown, known, points, out, **{**ok, "bias": offb})
    # the C entry itself refuses the misaligned pointers (PN2_ERANGE, as the plain listed-rows entry does) before any launch
    lib = ext._lib
    args = [B, N, S, C, unknown.data_ptr(), known.data_ptr(), points.data_ptr(), C, out.data_ptr(), C, lst.data_ptr(), counts.data_ptr()]
    assert lib.pn2x_three_nn_interpolate_pm_rows_act(*args, off.data_ptr(), bias.data_ptr(), 1, None) == -3
    assert lib.pn2x_three_nn_interpolate_pm_rows_act(*args, wx.data_ptr(), offb.data_ptr(), 1, None) == -3
    assert lib.pn2x_three_nn_interpolate_pm_rows_act(*args, None, bias.data_ptr(), 1, None) == -2
    # widths: multiples of 4 up to 1024 (Wx and the bias are held in LDS)
    sup = lib.pn2x_three_nn_interpolate_pm_rows_act_supported
    assert sup(B, N, S, 1024, 1024, 1024) == 1 and sup(B, N, S, 1028, 1028, 1028) == 0 and sup(B, N, S, 6, 8, 8) == 0
    big = torch.zeros(B, S, 1028, device="cuda")
    with pytest.raises(ValueError):
        ext.three_nn_interpolate_pm(unknown, known, big, torch.zeros(B, N, 1028, device="cuda"), rows=(lst, counts),
                                    wx=torch.zeros(1028, 3, device="cuda"), bias=torch.zeros(1028, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out[0, ~_lists(B, N, ((15, 17),), 3)[2][0].cuda()] == SENTINEL).all())


# ---- row_chain3 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights():
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(11)

    def lin(o, i, s):
        return (torch.randn(o, i, generator=g) * s).cuda(), (torch.randn(o, generator=g) * 0.1).cuda()
    wa, ba = lin(128, 131, 0.1)
    wb, bb = lin(128, 128, 0.1)
    wc, bc = lin(384, 128, 0.1)
    wq = (torch.randn(512, 384, generator=g) * 0.05).cuda()
    p = ext.row_chain_pack
    return (wa, ba, wb, bb, wc, bc, wq), (p(wa), ba, p(wb), bb, p(wc), bc, p(wq))


def _tail64(h1):
    _, _, wb, bb, wc, bc, wq = (t.double() for t in _weights()[0])
    h = torch.relu(h1.double() @ wb.t() + bb)
    c = torch.relu(h @ wc.t() + bc)
    return (c @ wq.t()).cpu()


@functools.lru_cache(maxsize=None)
def _chain_problem(B, N):
    """fp1_in rows [features | xyz | NaN pad], h1 = relu(first layer) in float64 rounded once to float32 in rows of 132 floats
    with NaN behind column 128, and the float64 chains over either (B, N, 512), computed once per shape."""
    g = torch.Generator().manual_seed(1000 * B + N)
    x = torch.randn(B, N, 132, generator=g).cuda()
    x[:, :, 131] = float("nan")
    wa, ba = (t.double() for t in _weights()[0][:2])
    h1_64 = torch.relu(x[..., :131].double() @ wa.t() + ba)
    h1 = torch.full((B, N, 132), float("nan"), device="cuda")
    h1[:, :, :128] = h1_64.float()
    return x, h1, _tail64(h1[..., :128]), _tail64(h1_64)


def _chain_mask(listed, small):
    mask = torch.zeros(*listed.shape, 512, dtype=torch.bool)
    mask[small] = True
    mask[:, :, 256:] |= listed[:, :, None]
    return mask


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _chain_cases():
    out = []
    for B in (1, 3):
        for N in (64, 1000):
            out += [(B, N, pairs) for pairs in _count_mixes(B, N)]
    out += [(1, 1000, ((17, 47),)), (3, 1000, ((65, 63), (0, 0), (16, 16)))]  # tiles of 1..4 groups, a share that crosses an empty cloud
    return out


@pytest.mark.parametrize("B,N,pairs", _chain_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_row_chain3_against_fp64_and_across_grids(B, N, pairs):
    from hotrack_amd import ext
    x, h1, ref, ref4 = _chain_problem(B, N)
    lst, counts, listed, small = _lists(B, N, pairs, 7 * N + B)
    mask = _chain_mask(listed, small)
    packed = _weights()[1]
    outs = []
    for grid in (1, 7, _cus()):
        out = torch.full((B, N, 512), SENTINEL, device="cuda")
        ext.row_chain3(h1[:, :, :128], lst, counts, *packed[2:], out=out, grid=grid)  # rows 132 floats apart, NaN behind them
        outs.append(out)
    four = torch.full((B, N, 512), SENTINEL, device="cuda")
    ext.row_chain(x, lst, counts, *packed, out=four, grid=1)
    torch.cuda.synchronize()
    o1 = outs[0].cpu()
    assert bool((o1[~mask] == SENTINEL).all()), f"{pairs}: wrote outside the listed rows / columns"
    _close(o1, ref, mask, f"row_chain3 grid 1 {pairs}")
    for grid, out in zip((7, _cus()), outs[1:]):
        assert torch.equal(out, outs[0]), f"grid {grid} differs from grid 1 for {pairs}"
    # the same rows through ext.row_chain's four layers: each within its own bound of float64
    if mask.any():
        scale = max(1.0, float(ref4.abs().max()))
        _close(four.cpu(), ref4, mask, f"row_chain grid 1 {pairs}")
        apart = float((o1[mask] - four.cpu()[mask]).abs().max())
        print(f"row_chain3 vs row_chain {pairs}: {apart:.3e} (bound {4e-5 * scale:.3e})")
        assert apart <= 4e-5 * scale, (pairs, apart)


def test_row_chain3_refuses_what_it_does_not_cover():
    from hotrack_amd import ext
    from hotrack_amd.pointnet2_hip import Pn2Error
    B, N = 1, 64
    _, h1, _, _ = _chain_problem(B, N)
    lst, counts, _, _ = _lists(B, N, ((15, 17),), 5)
    packed = _weights()[1][2:]
    out = torch.full((B, N, 512), SENTINEL, device="cuda")
    assert ext.row_chain3_supported(128, 384, 512) and not ext.row_chain3_supported(64, 384, 512)
    assert not ext.row_chain3_supported(128, 256, 512) and not ext.row_chain3_supported(128, 384, 256)
    with pytest.raises(Pn2Error):  # rows that start 4 bytes past a 16-byte boundary
        ext.row_chain3(h1[:, :, 1:129], lst, counts, *packed, out=out)
    with pytest.raises(ValueError):  # rows narrower than h1
        ext.row_chain3(h1[:, :, :124], lst, counts, *packed, out=out)
    with pytest.raises(Pn2Error):  # a row stride that is no multiple of 4 floats
        ext.row_chain3(torch.zeros(B, N, 130, device="cuda"), lst, counts, *packed, out=out)
    wb_off = torch.zeros(128 * 128 + 1, device="cuda")[1:]
    with pytest.raises(Pn2Error):
        ext.row_chain3(h1[:, :, :128], lst, counts, wb_off, *packed[1:], out=out)
    with pytest.raises(ValueError):
        ext.row_chain3(h1[:, :, :128], lst, counts, *packed, out=torch.empty(B, N, 256, device="cuda"))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_capture_on_one_list_and_replay_on_others():
    """Interpolation with the epilogue, then row_chain3 on what it wrote: captured on one list, replayed on two others."""
    from hotrack_amd import ext
    B, N, S = 3, 1000, 256
    (unknown, known, points, wx, bias), _, _ = _interp_problem(B, N, S, 128)
    packed = _weights()[1][2:]

    def run(lst, counts, h1, out):
        ext.three_nn_interpolate_pm(unknown, known, points, h1, rows=(lst, counts), wx=wx, bias=bias, relu=True)
        ext.row_chain3(h1, lst, counts, *packed, out=out)

    lst_s, cnt_s, _, _ = _lists(B, N, ((16, 16), (0, 0), (1, 0)), 1)
    h1 = torch.zeros((B, N, 128), device="cuda")
    buf = torch.full((B, N, 512), SENTINEL, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # both kernels have run once before the capture
        run(lst_s, cnt_s, h1, buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(lst_s, cnt_s, h1, buf)
    for r, pairs in enumerate((((65, 63), (N, 0), (17, 47)), ((0, 1), (64, 0), (15, 17)))):
        lst, counts, listed, small = _lists(B, N, pairs, 50 + r)
        lst_s.copy_(lst)
        cnt_s.copy_(counts)
        h1.zero_()
        buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        eager_h1 = torch.zeros((B, N, 128), device="cuda")
        eager = torch.full((B, N, 512), SENTINEL, device="cuda")
        run(lst, counts, eager_h1, eager)
        assert torch.equal(h1, eager_h1) and torch.equal(buf, eager), f"replay on {pairs} differs from the eager launches"
        assert bool((buf.cpu()[~_chain_mask(listed, small)] == SENTINEL).all())


# ---- the route --------------------------------------------------------------------------------------------------------------
def _fast(model, d, fold):
    """pred_kp of the point-major path with FastEval.fold_interp = fold."""
    from hotrack_amd import fused
    from models import pointnet_utils
    from models.fast_eval import FastEval
    from test_gpu_tail_perm import FLAGS
    before = FastEval.fold_interp
    try:
        FastEval.fold_interp = fold
        pointnet_utils.set_fused_backend(fused)
        with torch.no_grad():
            out = model(d, dict(FLAGS))["pred_kp"].clone()
        assert model._fast
        return out
    finally:
        FastEval.fold_interp = before
        pointnet_utils.set_fused_backend(None)


@pytest.mark.parametrize("B", [3, 32])
def test_both_routes_against_the_fp64_module_path(B):
    """B = 3: the small-batch route, which the switch does not reach (equal bits); B = 32: the smallest batch of the large route."""
    from hotrack_amd import ext
    from test_gpu_tail_perm import _model, _module64, _to_dev
    model = _model()
    frames = synthetic_frames(500 + B, B, 1024)
    d = _to_dev(frames)
    calls = []
    real = ext.row_chain3
    try:
        ext.row_chain3 = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        new, old = _fast(model, d, True), _fast(model, d, False)
    finally:
        ext.row_chain3 = real
    large = model._fast._large_batch(B, 1024)
    assert large == (B == 32) and len(calls) == (1 if large else 0), (large, calls)  # the folded forward, and only it, ran row_chain3
    ref = _module64(model, frames)
    e_new, e_old = float((new.double() - ref).abs().max()), float((old.double() - ref).abs().max())
    print(f"B={B}: |pred_kp - fp64 module path|: folded route {e_new:.3g}, unfolded route {e_old:.3g}; "
          f"routes apart {float((new - old).abs().max()):.3g}")
    if not large:
        assert torch.equal(new, old)
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert e_new <= 2e-5 and e_old <= 2e-5, (e_new, e_old)


def test_graph_capture_of_the_folded_route_replays_on_other_inputs():
    from hotrack_amd import fused
    from models import pointnet_utils
    from models.fast_eval import FastEval
    from test_gpu_tail_perm import FLAGS, _model, _to_dev
    assert FastEval.fold_interp is True
    model = _model()
    B = 32
    batches = [_to_dev(synthetic_frames(720 + i, B, 1024)) for i in range(3)]
    eager = [_fast(model, b, True) for b in batches]
    assert model._fast._large_batch(B, 1024) and model._fast.P["fold_interp"] is not None
    slot = _to_dev(synthetic_frames(720, B, 1024))
    try:
        pointnet_utils.set_fused_backend(fused)
        with torch.no_grad():
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = model(slot, dict(FLAGS))["pred_kp"]
            for i in (1, 2):
                for k in ("jittered_hand_kp", "hand_points"):
                    slot[k].copy_(batches[i][k])
                slot["gt_hand_pose"]["palm_template"].copy_(batches[i]["gt_hand_pose"]["palm_template"])
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager[i]), (i, float((out - eager[i]).abs().max()))
    finally:
        pointnet_utils.set_fused_backend(None)
