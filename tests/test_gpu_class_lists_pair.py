"""GPU: the partition launch of the class walk (ext.sa_class_lists / ext.sa_class_lists_pair; sa_class_lists2_kernel in
hotrack_amd/csrc/sa_fused.hip) against the plain-torch statement of the class rule, ext.sa_class_partition.  Equality is exact.

A thread of the one workgroup per problem owns a contiguous run of `per` centroids, per = ceil(M / 1024) rounded up to a multiple
of 4, read as 16-byte quads; up to M = 32768 the classes stay in registers, above that (the shapes (9, 4099) here, and any
problem paired with it) the second pass reads the counts again.  The shapes put M below, at and above the thread count, off
every multiple of 4 and of the run, and S off every divisor of the run, so the (cloud, centroid) carry crosses clouds inside a
run; the count patterns put class changes on the run and quad boundaries."""
import os
import sys

import pytest
import torch

from _netinit import deterministic_init, make_cfg, synthetic_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
pytestmark = pytest.mark.gpu

EDGES = torch.tensor([1, 8, 9, 16, 17, 32], dtype=torch.int32)  # both sides of both class boundaries, and the two ends
# (B, S, n) of the first problem, (B, S, n) of the second: another shape and another n
PAIRS = [
    ((1, 1, 7), (3, 5, 64)),
    ((1, 3, 64), (9, 4099, 5000)),      # a small problem next to one beyond the register-resident size: both take the re-reading path
    ((3, 5, 9), (1, 1, 1)),
    ((1, 1023, 2048), (2, 37, 100)),
    ((1, 1024, 2048), (1, 1023, 4096)),
    ((1, 1025, 4096), (1, 3, 5)),
    ((2, 37, 64), (64, 256, 1024)),
    ((5, 4099, 8192), (1, 1025, 1500)),
    ((64, 256, 1024), (64, 128, 256)),  # the two levels of the 64-cloud serving batch
    ((9, 4099, 5000), (5, 4099, 4100)),
]


def _per(M):
    """The run of centroids one thread owns (sa_class_lists2_kernel)."""
    return ((M + 1023) // 1024 + 3) // 4 * 4


def _patterns(B, S, seed):
    """name -> (B,S) int32 counts: random edge values; class changes on the thread-run boundaries; on the quad boundaries."""
    M = B * S
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(M)
    by_class = torch.tensor([20, 12, 3], dtype=torch.int32)
    return {
        "random": EDGES[torch.randint(0, len(EDGES), (M,), generator=g)].view(B, S),
        "run-boundaries": by_class[(i // _per(M)) % 3].view(B, S),
        "quad-boundaries": by_class[(i // 4) % 3].view(B, S),
    }


def _reference(counts, n):
    """(records (B*S,4) {id, b*n, b, s}, sizes (3,)) from the class rule in plain torch, on the CPU."""
    counts = counts.cpu()
    B, S = counts.shape
    ids, sizes = ext_mod().sa_class_partition(counts)
    b = torch.div(ids, S, rounding_mode="floor")
    return torch.stack([ids, b * n, b, ids - b * S], dim=1).to(torch.int32), sizes


def ext_mod():
    from hotrack_amd import ext
    return ext


def _check(got, counts, n, what):
    lst, sizes = got
    ref_lst, ref_sizes = _reference(counts, n)
    assert lst.dtype == torch.int32 and tuple(lst.shape) == (counts.numel(), 4) and tuple(sizes.shape) == (3,)
    assert torch.equal(sizes.cpu(), ref_sizes), f"{what}: sizes {sizes.tolist()} != {ref_sizes.tolist()}"
    assert torch.equal(lst.cpu(), ref_lst), f"{what}: records differ"


@pytest.mark.parametrize("pa,pb", PAIRS, ids=lambda p: "%dx%d" % p[:2])
def test_pair_launch_matches_the_class_rule(pa, pb):
    ext = ext_mod()
    (Ba, Sa, na), (Bb, Sb, nb) = pa, pb
    for (name, ca), cb in zip(_patterns(Ba, Sa, 11).items(), _patterns(Bb, Sb, 12).values()):
        ca, cb = ca.cuda(), cb.cuda()
        got_a, got_b = ext.sa_class_lists_pair(ca, na, cb, nb)
        _check(got_a, ca, na, f"{name} first {pa}")
        _check(got_b, cb, nb, f"{name} second {pb}")
        one = ext.sa_class_lists(ca, na)  # the one-problem launch is the matching half of the pair
        assert torch.equal(one[0], got_a[0]) and torch.equal(one[1], got_a[1]), f"{name}: one-problem launch differs"
        one = ext.sa_class_lists(cb, nb)
        assert torch.equal(one[0], got_b[0]) and torch.equal(one[1], got_b[1]), f"{name}: one-problem launch differs"


@pytest.mark.parametrize("B,S", [(3, 5), (1, 1025), (5, 4099), (9, 4099)])
def test_single_classes_and_an_empty_class(B, S):
    ext = ext_mod()
    g = torch.Generator().manual_seed(5)
    M = B * S
    cases = {"all-32": torch.full((M,), 20), "all-16": torch.full((M,), 12), "all-8": torch.full((M,), 3)}
    for name, vals in (("no-32", (1, 8, 9, 16)), ("no-16", (1, 8, 17, 32)), ("no-8", (9, 16, 17, 32))):
        v = torch.tensor(vals)
        cases[name] = v[torch.randint(0, len(v), (M,), generator=g)]
    other = EDGES[torch.randint(0, len(EDGES), (2 * 37,), generator=g)].view(2, 37).cuda()
    for name, c in cases.items():
        c = c.to(torch.int32).view(B, S).cuda()
        got, got_other = ext.sa_class_lists_pair(c, 777, other, 64)
        _check(got, c, 777, name)
        _check(got_other, other, 64, name + " partner")
        assert int((got[1] == 0).sum()) == (2 if name.startswith("all") else 1)
        _check(ext.sa_class_lists_pair(other, 64, c, 777)[1], c, 777, name + " as second problem")


def test_empty_batch_gives_zero_sizes():
    ext = ext_mod()
    empty = torch.empty((0, 37), dtype=torch.int32, device="cuda")
    other = EDGES.repeat(10).view(3, 20).cuda()
    lst, sizes = ext.sa_class_lists(empty, 64)
    assert tuple(lst.shape) == (0, 4) and sizes.tolist() == [0, 0, 0]
    (la, sa), got_b = ext.sa_class_lists_pair(empty, 64, other, 99)
    assert tuple(la.shape) == (0, 4) and sa.tolist() == [0, 0, 0]
    _check(got_b, other, 99, "partner of an empty problem")
    got_a, (lb, sb) = ext.sa_class_lists_pair(other, 99, empty, 64)
    assert sb.tolist() == [0, 0, 0]
    _check(got_a, other, 99, "first problem next to an empty one")


def test_capture_and_replay_on_other_counts():
    """The lists are a function of the counts in device memory alone: a captured launch replayed on two other sets of counts
    gives their lists."""
    ext = ext_mod()
    (Ba, Sa, na), (Bb, Sb, nb) = (5, 4099, 8192), (2, 37, 64)
    sets = [(_patterns(Ba, Sa, 20 + i)[k], _patterns(Bb, Sb, 30 + i)[k])
            for i, k in enumerate(("random", "run-boundaries", "quad-boundaries"))]
    sets.append((torch.full((Ba, Sa), 3, dtype=torch.int32), torch.full((Bb, Sb), 20, dtype=torch.int32)))  # classes empty at capture appear
    ca, cb = sets[-1][0].cuda(), sets[-1][1].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the kernel has run once before the capture
        ext.sa_class_lists_pair(ca, na, cb, nb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_a, got_b = ext.sa_class_lists_pair(ca, na, cb, nb)
    for i, (xa, xb) in enumerate(sets):
        ca.copy_(xa)
        cb.copy_(xb)
        got_a[0].fill_(-1)
        got_b[0].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        _check(got_a, xa, na, f"replay {i}, first problem")
        _check(got_b, xb, nb, f"replay {i}, second problem")


def test_fast_path_with_the_early_ball_query_is_bit_equal():
    """FastEval at 32 x 1024 with the deterministic weights: on the class route level 2's ball query runs before sa1 and one
    launch partitions both levels; pred_kp and the features of both levels equal the fixed-K route bit for bit."""
    from hotrack_amd import ext, fused, pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    pointnet_utils.set_operator_backend(pointnet2_utils)
    torch.manual_seed(0)
    model = HandTrackNet(make_cfg("cuda"))
    deterministic_init(model)
    model = model.cuda().eval()
    B, Np = 32, 1024
    d = synthetic_frames(910, B, Np)
    d = {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()}) for k, v in d.items()}
    flags = {"track_flag": False, "test_flag": True, "save_flag": False, "IKNet_flag": False}
    feats, calls = [], []
    real = (ext.sa_mlp_max, ext.sa_mlp_max_classes, ext.sa_class_lists_pair, ext.sa_class_lists)

    def spy(fn, name):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            if a[0].shape[2] == 32:  # the two ball-query levels (the keypoint modules use 16 and 64 neighbours)
                feats.append((name, out.clone()))
            return out
        return wrapped

    def count(fn, name):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped

    try:
        pointnet_utils.set_fused_backend(fused)
        ext.sa_mlp_max, ext.sa_mlp_max_classes = spy(real[0], "fixed"), spy(real[1], "classes")
        ext.sa_class_lists_pair, ext.sa_class_lists = count(real[2], "pair"), count(real[3], "single")
        with torch.no_grad():
            a = model(d, dict(flags))
            assert model._fast is not None and model._fast._large_batch(B, Np) and model._fast.sa_classes
            model._fast.sa_classes = False
            b = model(d, dict(flags))
            model._fast.sa_classes = True
    finally:
        ext.sa_mlp_max, ext.sa_mlp_max_classes, ext.sa_class_lists_pair, ext.sa_class_lists = real
        pointnet_utils.set_fused_backend(None)
    assert calls == ["pair"], calls  # one partition launch per forward, none on the fixed-K route
    assert [n for n, _ in feats] == ["classes", "classes", "fixed", "fixed"], [n for n, _ in feats]
    assert torch.equal(feats[0][1], feats[2][1]), "level-1 features differ"
    assert torch.equal(feats[1][1], feats[3][1]), "level-2 features differ"
    assert torch.equal(a["pred_kp"], b["pred_kp"]), float((a["pred_kp"] - b["pred_kp"]).abs().max())
