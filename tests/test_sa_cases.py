"""CPU: the reference and cases of tests/_sa_cases.py, before tests/test_gpu_sa_mlp_max.py rests on them.
reference_sa is anchored to the network's own set-abstraction scale in float64; every case of the GPU test's table is checked to
be a useful one (accepted layouts, finite outputs, a ReLU that bites without swamping the comparison, a float32 evaluation inside
the bound); the comparison is shown to fail for each way the kernel could be subtly wrong; the edge cases are shown to reach
their edges."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
import _sa_cases as C  # noqa: E402
from _netinit import deterministic_init  # noqa: E402


@pytest.mark.parametrize("D,D2", [(0, 0), (64, 0), (0, 64), (64, 64)])
def test_reference_is_the_networks_scale(D, D2):
    """PointNetSetAbstractionMsg_GivenCenterPoints._scale (group | xyz - centre | cat | [Conv2d 1x1 + BN + ReLU] x3 | max), eval
    mode, fused backend off, in float64 on the CPU with the plain-indexing operators of oracle/cpu_reference.py, against
    reference_sa fed from fused.fold_conv_bn and the W1 split fused.sa_scale performs."""
    from hotrack_amd import fused
    from models import pointnet_utils
    from models.pointnet_utils import PointNetSetAbstractionMsg_GivenCenterPoints
    from oracle import cpu_reference
    B, N, S, K = 2, 50, 11, 16
    m = PointNetSetAbstractionMsg_GivenCenterPoints([0.2], [K], [[64, 64, 128] if D else [32, 32, 64]], in_channel=D + 3 + D2, knn=True)
    deterministic_init(m)
    g = torch.Generator().manual_seed(D + 2 * D2 + 1)
    for p in m.parameters():
        p.data.add_(0.01 * torch.randn(p.shape, generator=g))
    m = m.double().eval()
    f64 = torch.float64
    xyz, new_xyz = torch.rand(B, 3, N, generator=g, dtype=f64), torch.rand(B, 3, S, generator=g, dtype=f64)
    pts = torch.randn(B, D, N, generator=g, dtype=f64) if D else None
    cf = torch.randn(B, D2, S, generator=g, dtype=f64) if D2 else None
    idx = torch.randint(0, N, (B, S, K), generator=g, dtype=torch.int32)
    ops_before, fused_before = pointnet_utils._OPS, pointnet_utils.fused_backend()
    try:
        pointnet_utils.set_operator_backend(cpu_reference)
        pointnet_utils.set_fused_backend(None)
        with torch.no_grad():
            want = m._scale(0, xyz, pts, new_xyz, idx, cf)
    finally:
        pointnet_utils.set_operator_backend(ops_before)
        pointnet_utils.set_fused_backend(fused_before)
    (W1, b1), (W2, b2), (W3, b3) = (fused.fold_conv_bn(c, n) for c, n in zip(m.conv_blocks[0], m.bn_blocks[0]))
    a1f = pts.transpose(1, 2) @ W1[:, :D].t() if D else None
    cadd = cf.transpose(1, 2) @ W1[:, D + 3:].t() if D2 else None
    got = C.reference_sa(f64, idx, a1f, xyz.transpose(1, 2), new_xyz.transpose(1, 2), W1[:, D:D + 3], b1, cadd, W2, b2, W3, b3)
    assert want.shape == (B, m.conv_blocks[0][2].weight.shape[0], S) and float(want.abs().max()) > 0.1
    assert float((got.transpose(1, 2) - want).abs().max()) <= 1e-10


def test_the_table_is_the_one_asked_for():
    specs = C.case_specs()
    inst = [n for n in specs if n.startswith("inst-")]
    assert len(inst) == 54 and len(set(C.CASES)) == len(C.CASES)
    assert {(specs[n]["widths"], specs[n]["K"], specs[n]["ops"]) for n in inst} == {(w, k, o) for w in C.WIDTHS for k in C.KS for o in C.OPERANDS}
    assert all((specs[n]["B"], specs[n]["N"], specs[n]["S"]) == (3, 50, 11) for n in inst)
    assert sum(not specs[n]["has_b1"] for n in inst) == 27
    for ops in C.OPERANDS:          # every operand set meets every output form and both b1 states at every width
        for w in C.WIDTHS:
            mine = [specs[n] for n in inst if specs[n]["ops"] == ops and specs[n]["widths"] == w]
            assert {s["form"] for s in mine} == set(C.FORMS) and {s["has_b1"] for s in mine} == {True, False}
    for widths, K in C.EDGE_CONFIGS:
        for edge in ("ends", "padded", "dup", "b3"):
            assert specs[f"edge-{edge}-{widths[0]}-K{K}"]["ops"] == "axc"
    for widths, K in C.GRID_CONFIGS:
        tag = f"{widths[0]}-K{K}"
        assert (specs[f"grid-1x1-{tag}"]["B"], specs[f"grid-1x1-{tag}"]["S"]) == (1, 1)
        assert (specs[f"grid-2x8-{tag}"]["B"], specs[f"grid-2x8-{tag}"]["S"]) == (2, 8)
        s = specs[f"grid-5x21-cu3-{tag}"]
        assert (s["B"], s["N"], s["S"], s["cus"]) == (5, 64, 21, 3)
    assert specs["grid-2x8-128-K16"]["S"] * specs["grid-2x8-128-K16"]["K"] == 128
    p = specs["production-33x1024x21-128-K64"]
    assert (p["B"], p["N"], p["S"], p["K"], p["widths"], p["ops"]) == (33, 1024, 21, 64, (128, 128, 192), "axc")


@pytest.mark.parametrize("name", C.CASES)
def test_every_table_case_is_a_useful_one(name):
    case = C.get_case(name)
    C1, C2, C3 = case.widths
    B, N, S, K = case.B, case.N, case.S, case.K
    kw = C.kernel_args(case)
    f32 = torch.float32
    assert kw["idx"].shape == (B, S, K) and kw["idx"].dtype == torch.int32 and kw["idx"].is_contiguous()
    assert int(kw["idx"].min()) >= 0 and int(kw["idx"].max()) < N
    assert (kw["a1f"] is not None) == ("a" in case.ops) and (kw["xyz"] is not None) == ("x" in case.ops) and (kw["cadd"] is not None) == ("c" in case.ops)
    assert kw["a1f"] is not None or kw["xyz"] is not None
    for key, rows in (("a1f", N), ("cadd", S)):  # rows of 16-byte quads: offset and row stride multiples of 4 floats
        t = kw[key]
        if t is not None:
            assert t.shape == (B, rows, C1) and t.dtype == f32 and t.stride(2) == 1 and t.stride(1) % 4 == 0 and t.stride(1) >= C1
            assert t.storage_offset() % 4 == 0 and t.stride(0) == rows * t.stride(1) and bool(torch.isfinite(t).all())
            wide = case.a1f_wide if key == "a1f" else case.cadd_wide
            if case.form == "block":  # a real column block, NaN around it
                assert t.storage_offset() > 0 and t.stride(1) > C1 and int(torch.isnan(wide).sum()) == B * rows * (wide.shape[2] - C1)
            else:
                assert t.is_contiguous()
    if kw["xyz"] is not None:
        assert kw["xyz"].shape == (B, N, 3) and kw["cxyz"].shape == (B, S, 3) and kw["wx"].shape == (C1, 3)
        assert all(kw[k].is_contiguous() and kw[k].dtype == f32 for k in ("xyz", "cxyz", "wx"))
        assert float(kw["xyz"].min()) >= 0 and float(kw["xyz"].max()) < 1
    else:
        assert kw["cxyz"] is None and kw["wx"] is None
    assert kw["b1"] is None or kw["b1"].shape == (C1,)
    assert kw["w2"].shape == (C2, C1) and kw["w3"].shape == (C3, C2) and kw["b2"].shape == (C2,) and kw["b3"].shape == (C3,)
    r64 = C.ref64(case)
    assert r64.shape == (B, S, C3) and r64.dtype == torch.float64 and bool(torch.isfinite(r64).all())
    zeros = float((r64 == 0).double().mean())
    print(f"{name}: {100 * zeros:.1f}% of the outputs are exactly zero, largest {float(r64.max()):.3f}")
    assert 0.02 <= zeros <= 0.60
    C.compare(C.reference_of(case, f32), r64, f"{name}: float32 torch evaluation")


@pytest.mark.parametrize("widths", C.WIDTHS)
def test_the_comparison_binds(widths):
    """Each way the kernel could be subtly wrong moves the outputs beyond the bound."""
    case = C.get_case(f"inst-{widths[0]}-K16-axc")
    assert case.b1 is not None and int((case.idx[case.B - 1] == case.N - 1).sum()) >= 1
    r64 = C.ref64(case)
    xyz0 = case.xyz.clone()
    xyz0[case.B - 1, case.N - 1] = 0
    w2_swapped = case.w2.clone()  # h1 with channel quad 0 and quad 1 exchanged = W2 with those columns exchanged
    w2_swapped[:, 0:4], w2_swapped[:, 4:8] = case.w2[:, 4:8], case.w2[:, 0:4]
    wrong = {"the last neighbour dropped from the max": dict(idx=case.idx[:, :, :-1]),
             "cxyz of centroid s + 1": dict(cxyz=case.cxyz.roll(-1, dims=1)),
             "cadd of centroid s + 1": dict(cadd=case.cadd.roll(-1, dims=1)),
             "cadd omitted": dict(cadd=None),
             "the last point of the last cloud at the origin": dict(xyz=xyz0),
             "b1 omitted": dict(b1=None),
             "a channel quad of h1 exchanged with its neighbour": dict(w2=w2_swapped)}
    for what, override in wrong.items():
        r = C.ratio(C.reference_of(case, **override), r64)
        print(f"{case.name}, {what}: {r:.1f} times the bound")
        with pytest.raises(AssertionError, match="times the bound"):
            C.compare(C.reference_of(case, **override), r64, what)
        assert r > 100  # 1e-2 against 2e-5 + 1e-5 |ref|: far outside, not marginally
    assert C.ratio(r64.float(), r64) <= 0.01  # ... and a correctly rounded result is far inside
    nan = r64.clone()
    nan[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        C.compare(nan, r64, "a NaN output")


@pytest.mark.parametrize("widths,K", C.EDGE_CONFIGS)
def test_the_edge_cases_reach_their_edges(widths, K):
    tag = f"{widths[0]}-K{K}"
    ends = C.get_case(f"edge-ends-{tag}")
    assert bool((ends.idx[ends.B - 1] == ends.N - 1).all()) and bool((ends.idx[0] == 0).all())
    last = C.get_case(f"edge-last-1cloud-{tag}")
    assert last.B == 1 and bool((last.idx[0, ::2] == last.N - 1).all()) and int((last.idx[0, 1::2] != last.N - 1).sum()) > 0
    padded = C.get_case(f"edge-padded-{tag}")
    distinct = torch.tensor([[len(set(padded.idx[b, s].tolist())) for s in range(padded.S)] for b in range(padded.B)])
    assert torch.equal(distinct, (1 + torch.arange(padded.S) % K).expand(padded.B, -1))
    assert int(distinct.min()) == 1 and int(distinct.max()) == K
    assert bool((padded.idx[:, 5, 6:] == padded.idx[:, 5, :1]).all())  # 6 distinct entries, the rest repeat entry 0
    dup = C.get_case(f"edge-dup-{tag}")
    half = K // 2
    assert bool((dup.idx[:, :, half:] != dup.idx[:, :, :half]).all())  # other points ...
    for t in (dup.a1f, dup.xyz):                                       # ... with the same rows: every maximum is reached twice
        assert torch.equal(C._rows(t, dup.idx[:, :, half:]), C._rows(t, dup.idx[:, :, :half]))
    assert torch.equal(C.reference_of(dup, idx=dup.idx[:, :, :half]), C.ref64(dup))
    b3 = C.get_case(f"edge-b3-{tag}")
    zero, pos = C.forced_channels(widths[2])
    assert int(zero.sum()) >= widths[2] // 3 and int(pos.sum()) >= widths[2] // 3 and not bool((zero & pos).any())
    r = C.ref64(b3)
    assert float(r[:, :, zero].abs().max()) == 0.0 and float(r[:, :, pos].min()) > 0.1
    pre = C.reference_of(b3, b3=torch.zeros_like(b3.b3))  # the layer-3 products alone are far below the forcing bias
    assert float(pre.max()) < 50


def test_pair_cases_share_points_and_split_one_buffer():
    for order in C.PAIR_ORDERS:
        for with_cadd in (False, True):
            p0, p1 = C.get_pair(order, with_cadd)
            assert (p0.K, p1.K) == order and p0.widths == p1.widths == (128, 128, 192) and (p0.B, p0.N, p0.S) == (2, 64, 21)
            assert p0.xyz is p1.xyz and p0.cxyz is p1.cxyz and p0.a1f_wide is p1.a1f_wide and (p0.a1f_off, p1.a1f_off) == (0, 128)
            assert (p0.cadd is not None) == (p1.cadd is not None) == with_cadd and not torch.equal(p0.w2, p1.w2)
            for p in (p0, p1):
                kw = C.kernel_args(p)
                assert kw["a1f"].stride(1) == 256 and kw["a1f"].storage_offset() % 4 == 0 and int(kw["idx"].max()) < p.N
                r64 = C.ref64(p)
                assert 0.02 <= float((r64 == 0).double().mean()) <= 0.60
                C.compare(C.reference_of(p, torch.float32), r64, f"{p.name}: float32 torch evaluation")
