"""GPU: the fused set-abstraction kernel without its ball-query padding (ext.sa_mlp_max_classes, ext.sa_class_lists and the hit
counts of ext.ball_query_picks / ext.fps_two_level; hotrack_amd/csrc/sa_fused.hip, ball_query.hip).

A centroid whose list has c hits is served with its first 8, 16 or 32 slots; the dropped slots repeat slot 0, so the output
must equal the fixed-K = 32 launch on the same inputs BIT FOR BIT, for every class mix, and stay within the fp64 bound of
tests/_sa_cases.py.  Index rows are built by hand with prescribed hit counts (1, 8, 9, 16, 17, 32 and the all-zero row of a
centroid without a hit, reported as 1); S = 37 leaves the last position group of every class short.  The class sizes live in
device memory only: a captured launch replayed on an input with another class mix (a class that was empty at capture) must give
that input's eager result."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sa_cases as C  # noqa: E402
from _netinit import deterministic_init, make_cfg, synthetic_frames  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
pytestmark = pytest.mark.gpu

W32, W64 = C.WIDTHS[0], C.WIDTHS[1]
K, N = 32, 64
# (widths, operands): the two levels' instances (sa1: coordinates only, sa2: features + coordinates), each also with cadd
CONFIGS = ((W32, "x"), (W32, "xc"), (W64, "ax"), (W64, "axc"))
# hit counts per centroid, cycled over the B * S centroids; 0 = a row without a hit (all zeros, reported as 1)
PATTERNS = {
    "all-1": (1,),                                   # one class (8) only
    "edges": (1, 8, 9, 16, 17, 32, 0),               # both sides of both class boundaries, a full list, a row without a hit
    "no-16": (3, 20, 8, 32, 17, 1, 0, 25),           # class 16 empty
    "only-16": (9, 16, 12, 10),                      # one class (16) only
    "all-32": (32,),                                 # every list full: today's work, through the class walk
    "no-32": (2, 9, 16, 8, 0, 5, 13),                # class 32 empty
}


def _counts(pattern, B, S, shift=0):
    p = PATTERNS[pattern]
    return torch.tensor([p[(i + shift) % len(p)] for i in range(B * S)], dtype=torch.int32).view(B, S)


def _index_rows(g, hits):
    """(B, S) hit counts -> ball-query lists (B, S, 32): `hits` distinct points, then copies of the first; no hit -> zeros."""
    B, S = hits.shape
    idx = torch.zeros(B, S, K, dtype=torch.int32)
    for b in range(B):
        for s in range(S):
            n = int(hits[b, s])
            if n:
                idx[b, s, :n] = torch.randperm(N, generator=g)[:n].int()
                idx[b, s, n:] = idx[b, s, 0]
    return idx


_CASES = {}


def _case(widths, ops, pattern, B=2, S=37, form="block", shift=0):
    key = (widths, ops, pattern, B, S, form, shift)
    if key not in _CASES:
        seed = 9000 + len(_CASES)
        c = C.make_case(f"classes-{widths[0]}-{ops}-{pattern}-{B}x{S}-{form}", widths, K, B, N, S, ops, True, form, seed)
        hits = _counts(pattern, B, S, shift)
        c.idx = _index_rows(torch.Generator().manual_seed(seed + 1), hits)
        c.counts = hits.clamp(min=1)
        c._ref64 = None
        _CASES[key] = c
    return _CASES[key]


def _launch(ext, case, kw, classes):
    """One launch in the case's output form -> (B, S, C3); classes None = the fixed-K launch."""
    C3 = case.widths[2]
    fn = (lambda **a: ext.sa_mlp_max(**a)) if classes is None else (lambda **a: ext.sa_mlp_max_classes(classes=classes, **a))
    if case.form == "block":
        buf = torch.full((case.B, case.S, C3 + C.OUT_PAD), C.SENTINEL, device="cuda")
        fn(out=buf[:, :, C.OUT_OFF:C.OUT_OFF + C3], **kw)
        keep = torch.ones(C3 + C.OUT_PAD, dtype=torch.bool, device="cuda")
        keep[C.OUT_OFF:C.OUT_OFF + C3] = False
        assert bool((buf[:, :, keep] == C.SENTINEL).all()), f"{case.name}: columns around the output block were written"
        return buf[:, :, C.OUT_OFF:C.OUT_OFF + C3]
    if case.form == "pm":
        return fn(point_major=True, **kw)
    return fn(**kw).transpose(1, 2)


def _both(ext, case):
    kw = C.kernel_args(case, "cuda")
    fixed = _launch(ext, case, kw, None)
    classes = ext.sa_class_lists(case.counts.cuda(), N)
    got = _launch(ext, case, kw, classes)
    return fixed, got, classes


@pytest.mark.parametrize("pattern", tuple(PATTERNS))
@pytest.mark.parametrize("widths,ops", CONFIGS)
def test_class_walk_is_bit_equal_to_fixed_k(widths, ops, pattern):
    from hotrack_amd import ext
    assert ext.sa_mlp_max_classes_supported(K, *widths)
    case = _case(widths, ops, pattern)
    fixed, got, classes = _both(ext, case)
    assert torch.equal(got, fixed), f"{case.name}: differs from the fixed-K launch by {float((got - fixed).abs().max())}"
    C.compare(got, C.ref64(case), case.name)
    ids, sizes = ext.sa_class_partition(case.counts)
    assert torch.equal(classes[1].cpu(), sizes) and torch.equal(classes[0][:, 0].cpu(), ids)


@pytest.mark.parametrize("form", ["cm", "pm"])
@pytest.mark.parametrize("widths,ops", CONFIGS)
def test_class_walk_other_layouts_one_centroid_and_cu_cap(widths, ops, form):
    """The channel-major and plain point-major outputs; one cloud of one centroid; several tiles per workgroup on 1 compute unit."""
    from hotrack_amd import ext
    case = _case(widths, ops, "edges", form=form, shift=3)
    fixed, got, _ = _both(ext, case)
    assert torch.equal(got, fixed)
    C.compare(got, C.ref64(case), case.name)
    try:
        ext.sa_set_compute_units(1)
        _, capped, _ = _both(ext, case)
    finally:
        ext.sa_set_compute_units(0)
    assert torch.equal(capped, fixed), f"{case.name}: differs on one compute unit"
    for pattern in ("no-16", "all-32", "only-16"):  # B = 1, S = 1: a centroid of class 8 (3 hits), 32, 16
        one = _case(widths, ops, pattern, B=1, S=1, form=form)
        fixed, got, classes = _both(ext, one)
        assert torch.equal(got, fixed), one.name
        C.compare(got, C.ref64(one), one.name)
        assert int(classes[1].sum()) == 1


def _lattice_clouds():
    """Two clouds of 64 points on a lattice of spacing 1/8 (squared distances are multiples of 1/64, exact in fp32, and none is
    near r^2 = 0.09); in cloud 1, 40 points share two neighbouring sites: their lists overflow 32."""
    g = torch.Generator().manual_seed(77)
    xyz = torch.randint(0, 8, (2, N, 3), generator=g).float() / 8
    xyz[1, :40] = torch.tensor([0.5, 0.5, 0.5])
    xyz[1, 10:20, 0] = 0.625
    return xyz


def _ball_reference(xyz, picks, radius):
    """Plain torch: (idx (B,S,32) with first-hit padding, counts = min(hits, 32), 1 without a hit)."""
    B, S = picks.shape
    c = torch.gather(xyz, 1, picks.long()[:, :, None].expand(B, S, 3))
    d2 = ((c[:, :, None, :] - xyz[:, None, :, :]) ** 2).sum(-1)
    r2 = (torch.tensor(radius, dtype=torch.float32) * torch.tensor(radius, dtype=torch.float32))
    hit = d2 < r2
    idx = torch.zeros(B, S, K, dtype=torch.int32)
    for b in range(B):
        for s in range(S):
            j = torch.nonzero(hit[b, s]).flatten()[:K].int()
            if j.numel():
                idx[b, s] = j[0]
                idx[b, s, :j.numel()] = j
    return idx, hit.sum(-1).clamp(min=1, max=K).int(), hit.sum(-1)


def test_ball_query_hit_counts_and_class_lists():
    from hotrack_amd import ext
    xyz = _lattice_clouds()
    S, radius = 37, 0.3
    picks = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(5 + b))[:S] for b in range(2)]).int()
    picks[1, :6] = torch.tensor([0, 5, 12, 15, 39, 41])  # centroids inside the crowded sites
    ref_idx, ref_cnt, hits = _ball_reference(xyz, picks, radius)
    assert int(hits.max()) > K and int(hits.min()) < 8, "the fixture must hold an overflowing list and a short one"
    idx, new_xyz, cnt = ext.ball_query_picks(radius, K, xyz.cuda(), picks.cuda(), counts=True)
    idx0, _ = ext.ball_query_picks(radius, K, xyz.cuda(), picks.cuda())
    assert torch.equal(idx.cpu(), ref_idx) and torch.equal(idx0.cpu(), ref_idx)
    assert torch.equal(cnt.cpu(), ref_cnt)
    # a radius nothing lies within: every row is all zeros and reports 1
    idx_z, _, cnt_z = ext.ball_query_picks(0.0, K, xyz.cuda(), picks.cuda(), counts=True)
    assert int(idx_z.abs().max()) == 0 and bool((cnt_z == 1).all())
    # the launch behind fps_two_level(query=...) at this batch size (sampling's tie check rides in it)
    i1, l1, i2, idx1, cnt1 = ext.fps_two_level(xyz.cuda(), S, 16, query=(radius, K), query_counts=True)
    r_idx, r_cnt, _ = _ball_reference(xyz, i1.cpu(), radius)
    assert torch.equal(idx1.cpu(), r_idx) and torch.equal(cnt1.cpu(), r_cnt)
    plain = ext.fps_two_level(xyz.cuda(), S, 16, query=(radius, K))
    assert torch.equal(plain[3], idx1) and torch.equal(plain[0], i1)
    # class lists of these counts, and of more centroids than the partition kernel has threads
    g = torch.Generator().manual_seed(3)
    big = torch.randint(1, 33, (3, 700), generator=g, dtype=torch.int32)
    big[0, :6] = torch.tensor([8, 9, 16, 17, 32, 1])
    for counts, n in ((cnt, N), (big.cuda(), 1024), (torch.full((2, 5), 20, dtype=torch.int32).cuda(), 9)):
        lst, sizes = ext.sa_class_lists(counts, n)
        ids, ref_sizes = ext.sa_class_partition(counts.cpu())
        B, S_ = counts.shape
        assert torch.equal(sizes.cpu(), ref_sizes) and int(sizes.sum()) == B * S_
        lst = lst.cpu()
        assert torch.equal(lst[:, 0], ids)
        b = torch.div(ids, S_, rounding_mode="floor")
        assert torch.equal(lst[:, 1], b * n) and torch.equal(lst[:, 2], b) and torch.equal(lst[:, 3], ids - b * S_)


@pytest.mark.parametrize("widths,ops", [CONFIGS[0], CONFIGS[3]])
def test_class_walk_capture_and_replay_on_another_class_mix(widths, ops):
    """Captured on lists of one hit each (classes 32 and 16 empty), replayed on a mix of all three classes and on full lists."""
    from hotrack_amd import ext
    first = _case(widths, ops, "all-1")
    kw = C.kernel_args(first, "cuda")
    C3 = widths[2]
    idx_s, cnt_s = kw["idx"].clone(), first.counts.cuda()
    out_s = torch.full((first.B, first.S, C3), C.SENTINEL, device="cuda")
    kw_s = dict(kw, idx=idx_s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # every kernel has run once before the capture
        ext.sa_mlp_max_classes(classes=ext.sa_class_lists(cnt_s, N), out=out_s, **kw_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ext.sa_mlp_max_classes(classes=ext.sa_class_lists(cnt_s, N), out=out_s, **kw_s)
    for pattern in ("all-1", "edges", "all-32", "no-32"):
        other = _case(widths, ops, pattern)
        idx_s.copy_(other.idx.cuda())
        cnt_s.copy_(other.counts.cuda())
        out_s.fill_(C.SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        eager = ext.sa_mlp_max(point_major=True, **dict(kw, idx=other.idx.cuda()))
        assert torch.equal(out_s, eager), f"replay on {pattern}: differs by {float((out_s - eager).abs().max())}"


def test_fast_path_class_route_is_bit_equal():
    """FastEval at the smallest batch of the large-batch route (32 x 1024): pred_kp and the features of both levels, class route
    against the fixed-K route."""
    from hotrack_amd import ext, fused, pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    pointnet_utils.set_operator_backend(pointnet2_utils)
    torch.manual_seed(0)
    model = HandTrackNet(make_cfg("cuda"))
    deterministic_init(model)
    model = model.cuda().eval()
    B, Np = 32, 1024
    d = synthetic_frames(900, B, Np)
    d = {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in d.items()}
    flags = {"track_flag": False, "test_flag": True, "save_flag": False, "IKNet_flag": False}
    feats = []
    real = (ext.sa_mlp_max, ext.sa_mlp_max_classes)

    def spy(fn, name):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            if a[0].shape[2] == 32:  # the two ball-query levels (the keypoint modules use 16 and 64 neighbours)
                feats.append((name, out.clone()))
            return out
        return wrapped

    try:
        pointnet_utils.set_fused_backend(fused)
        ext.sa_mlp_max, ext.sa_mlp_max_classes = spy(real[0], "fixed"), spy(real[1], "classes")
        with torch.no_grad():
            a = model(d, dict(flags))
            assert model._fast is not None and model._fast._large_batch(B, Np) and model._fast.sa_classes
            model._fast.sa_classes = False
            b = model(d, dict(flags))
            model._fast.sa_classes = True
    finally:
        ext.sa_mlp_max, ext.sa_mlp_max_classes = real
        pointnet_utils.set_fused_backend(None)
    assert [n for n, _ in feats] == ["classes", "classes", "fixed", "fixed"], [n for n, _ in feats]
    assert torch.equal(feats[0][1], feats[2][1]), "level-1 features differ"
    assert torch.equal(feats[1][1], feats[3][1]), "level-2 features differ"
    assert torch.equal(a["pred_kp"], b["pred_kp"]), float((a["pred_kp"] - b["pred_kp"]).abs().max())
