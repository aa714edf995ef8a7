"""GPU: rearrange_module's slot sum taken after its product (hotrack_amd/csrc/tail.hip: pn2x_perm_sum_rows,
pn2x_add_layernorm_perm) against float64, and the FastEval route built on them (FastEval.fold_rearrange) against the route it
replaces.

Bounds.  perm_sum_rows adds re = 5 float32 summands of magnitude <= s in order: four roundings of partial sums of magnitude
<= 5 s give |err| <= 4 * 2^-24 * 5 * s; the inputs are drawn uniformly from [-1, 1], so s = 1.  add_layernorm_perm: 2e-5 absolute
and relative, the bound of tests/test_gpu_tail_kernels.py for add_layernorm against float64.  Route equality: both routes are
orders of the same float32 sums, so the new route's distance from the float64 module path may be at most twice the old route's
plus 1e-6."""
import copy
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
from _netinit import deterministic_init, make_cfg, synthetic_frames  # noqa: E402

pytestmark = pytest.mark.gpu
J, RE = 21, 5
CS = (4, 128, 256, 384)
BS = (1, 3)
PAD = 8  # extra floats per z row in the ldz > re*c cases
SENTINEL = -12345.0
FLAGS = {"track_flag": False, "test_flag": True, "save_flag": False, "IKNet_flag": False}
_CACHE = {}


def _tables():
    """The model's own table and one with repeated and self-referencing entries, (J, RE) int32 on the CPU."""
    if "tables" not in _CACHE:
        from models.blocks import rearrange_module
        own = rearrange_module(channel=8)._perm.t().contiguous().to(torch.int32)
        odd = torch.tensor([[t, t, 0, J - 1, (7 * t) % J] for t in range(J)], dtype=torch.int32)
        assert own.shape == odd.shape == (J, RE)
        _CACHE["tables"] = {"model": own, "repeats": odd}
    return _CACHE["tables"]


def _sum64(z, perm, B, c):
    """float64: out[b,t,:] = sum_r z[b, perm[t,r], r*c:(r+1)*c] for CPU z (B*J, >= RE*c)."""
    z3 = z.double().view(B, J, -1)
    return sum(z3[:, perm[:, r].long(), r * c:(r + 1) * c] for r in range(RE))


def _norms(C):
    if ("ln", C) not in _CACHE:
        g = torch.Generator().manual_seed(9000 + C)
        ln1, ln2 = nn.LayerNorm(C), nn.LayerNorm(C, eps=1e-6)
        with torch.no_grad():
            for ln in (ln1, ln2):
                ln.weight.copy_(torch.randn(C, generator=g))
                ln.bias.copy_(torch.randn(C, generator=g))
        _CACHE[("ln", C)] = (ln1, ln2, copy.deepcopy(ln1).cuda().requires_grad_(False), copy.deepcopy(ln2).cuda().requires_grad_(False))
    return _CACHE[("ln", C)]


def _ln64(u, ln):
    return F.layer_norm(u, (u.shape[-1],), ln.weight.detach().double(), ln.bias.detach().double(), ln.eps)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _raw_sum(ext, B, c, z, ldz, perm, out, j=J, re=RE):
    return ext._lib.pn2x_perm_sum_rows(B, j, re, c, _p(z), ldz, _p(perm), _p(out), None)


def _raw_ln(ext, B, c, z, ldz, perm, bias, d1, d2, out, j=J, re=RE):
    return ext._lib.pn2x_add_layernorm_perm(B, j, re, c, _p(z), ldz, _p(perm), _p(bias), _p(d1.weight), _p(d1.bias), d1.eps,
                                            _p(None if d2 is None else d2.weight), _p(None if d2 is None else d2.bias),
                                            0.0 if d2 is None else d2.eps, _p(out), None)


def _out_with_sentinel(B, c):
    return torch.full((B * J + 2, c), SENTINEL, device="cuda")


@pytest.mark.parametrize("table", ["model", "repeats"])
@pytest.mark.parametrize("c", CS)
def test_perm_sum_rows_matches_fp64(c, table):
    from hotrack_amd import ext
    perm = _tables()[table]
    g = torch.Generator().manual_seed(100 + c)
    bound = 4 * 2.0 ** -24 * 5 * 1.0
    worst = 0.0
    for B in BS:
        for pad in (0, PAD):
            z = torch.rand(B * J, RE * c + pad, generator=g) * 2 - 1
            ref = _sum64(z[:, :RE * c], perm, B, c)
            out = _out_with_sentinel(B, c)
            with torch.cuda.device(0):
                assert _raw_sum(ext, B, c, z.cuda(), RE * c + pad, perm, out) == 0
            got = out.cpu()
            assert bool((got[B * J:] == SENTINEL).all()), "rows past the last token were written"
            err = float((got[:B * J].double().view(B, J, c) - ref).abs().max())
            worst = max(worst, err)
            assert err <= bound, f"c={c} B={B} pad={pad}: {err:.3g} > {bound:.3g}"
            if pad:  # the binding: a column block of a wider buffer, same bits
                assert torch.equal(ext.perm_sum_rows(z.cuda()[:, :RE * c], perm, c).view(B * J, c), out[:B * J])
    print(f"perm_sum_rows c={c} {table}: worst |got - ref64| = {worst:.3g} (bound {bound:.3g})")


@pytest.mark.parametrize("table", ["model", "repeats"])
@pytest.mark.parametrize("c", CS)
def test_add_layernorm_perm_matches_fp64(c, table):
    from hotrack_amd import ext
    perm = _tables()[table]
    ln1, ln2, d1, d2 = _norms(c)
    g = torch.Generator().manual_seed(200 + c)
    worst = 0.0
    for B in BS:
        for pad in (0, PAD):
            z = torch.randn(B * J, RE * c + pad, generator=g) * 1.3 + 0.45
            bias = torch.randn(c, generator=g)
            zs = _sum64(z[:, :RE * c], perm, B, c).view(B * J, c)
            for use_ln2 in (False, True):
                for use_bias in (False, True):
                    ref = _ln64(zs + bias.double() if use_bias else zs, ln1)
                    if use_ln2:
                        ref = _ln64(ref, ln2)
                    out = _out_with_sentinel(B, c)
                    with torch.cuda.device(0):
                        assert _raw_ln(ext, B, c, z.cuda(), RE * c + pad, perm, bias.cuda() if use_bias else None, d1,
                                       d2 if use_ln2 else None, out) == 0
                    got = out.cpu()
                    assert bool((got[B * J:] == SENTINEL).all()), "rows past the last token were written"
                    got = got[:B * J].double()
                    assert bool(torch.isfinite(got).all())
                    r = float(((got - ref).abs() / (2e-5 + 2e-5 * ref.abs())).max())
                    worst = max(worst, r)
                    assert r <= 1.0, f"c={c} B={B} pad={pad} ln2={use_ln2} bias={use_bias}: {r:.3g} times the bound atol = rtol = 2e-5"
                    if pad:
                        via = ext.add_layernorm_perm(z.cuda()[:, :RE * c], perm, d1, bias=bias.cuda() if use_bias else None,
                                                     ln2=d2 if use_ln2 else None)
                        assert torch.equal(via, out[:B * J])
    print(f"add_layernorm_perm c={c} {table}: worst |got - ref64| / (2e-5 + 2e-5 |ref64|) = {worst:.4f}")


def test_bad_arguments_return_the_error_code_and_launch_nothing():
    from hotrack_amd import ext
    EINVAL, ENULL = -1, -2
    B, c = 2, 128
    perm = _tables()["model"]
    _, _, d1, d2 = _norms(c)
    z = torch.randn(B * J, RE * c, device="cuda")
    z6 = torch.randn(B * J, RE * 6, device="cuda")
    out = _out_with_sentinel(B, c)
    high, low = perm.clone(), perm.clone()
    high[J - 1, RE - 1] = J
    low[0, 2] = -1
    with torch.cuda.device(0):
        for bad in (high, low):
            assert _raw_sum(ext, B, c, z, RE * c, bad, out) == EINVAL
            assert _raw_ln(ext, B, c, z, RE * c, bad, None, d1, d2, out) == EINVAL
        assert _raw_sum(ext, B, 6, z6, RE * 6, perm, out) == EINVAL  # c % 4
        assert _raw_ln(ext, B, 6, z6, RE * 6, perm, None, d1, None, out) == EINVAL
        assert _raw_sum(ext, B, c, z, RE * c - 4, perm, out) == EINVAL  # ldz < re * c
        assert _raw_ln(ext, B, c, z, RE * c - 4, perm, None, d1, None, out) == EINVAL
        assert _raw_sum(ext, B, c, None, RE * c, perm, out) == ENULL
        assert _raw_sum(ext, B, c, z, RE * c, None, out) == ENULL
        assert _raw_sum(ext, B, c, z, RE * c, perm, None) == ENULL
        assert _raw_ln(ext, B, c, None, RE * c, perm, None, d1, None, out) == ENULL
        assert _raw_ln(ext, B, c, z, RE * c, None, None, d1, None, out) == ENULL
        assert _raw_ln(ext, B, c, z, RE * c, perm, None, d1, None, None) == ENULL
        assert ext._lib.pn2x_add_layernorm_perm(B, J, RE, c, _p(z), RE * c, _p(perm), None, None, _p(d1.bias), d1.eps, None, None, 0.0,
                                                _p(out), None) == ENULL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote its output"
    with pytest.raises(TypeError):
        ext.perm_sum_rows(z, perm.cuda(), c)  # the table is read on the host


# ---- the FastEval route ------------------------------------------------------------------------------------------------------


class _F64Ops:
    """The operator namespace for a float64 run of the module path on the GPU: index decisions by the HIP operators on the
    float32 coordinates (what every float32 route sees), gathers and interpolation as plain float64 indexing."""

    @staticmethod
    def _hip():
        from hotrack_amd import pointnet2_utils
        return pointnet2_utils

    @classmethod
    def furthest_point_sample(cls, xyz, n):
        return cls._hip().furthest_point_sample(xyz.to(torch.float32).contiguous(), n)

    @classmethod
    def ball_query(cls, r, k, xyz, new):
        return cls._hip().ball_query(r, k, xyz.to(torch.float32).contiguous(), new.to(torch.float32).contiguous())

    @staticmethod
    def _dist(u, kn, idx):
        B, n, k = idx.shape
        pick = torch.gather(kn.unsqueeze(1).expand(-1, n, -1, -1), 2, idx.long().unsqueeze(-1).expand(-1, -1, -1, 3))
        return (u.unsqueeze(2) - pick).norm(dim=-1)

    @classmethod
    def knn(cls, k, u, kn):
        _, idx = cls._hip().knn(k, u.to(torch.float32).contiguous(), kn.to(torch.float32).contiguous())
        return cls._dist(u, kn, idx), idx

    @classmethod
    def three_nn(cls, u, kn):
        _, idx = cls._hip().three_nn(u.to(torch.float32).contiguous(), kn.to(torch.float32).contiguous())
        return cls._dist(u, kn, idx), idx

    @staticmethod
    def three_interpolate(points, idx, weight):
        B, C, _ = points.shape
        n = idx.shape[1]
        g = torch.gather(points.unsqueeze(2).expand(-1, -1, n, -1), 3, idx.long().unsqueeze(1).expand(-1, C, -1, -1))
        return (g * weight.unsqueeze(1)).sum(dim=-1)

    @staticmethod
    def gather_operation(feature, idx):
        return torch.gather(feature, 2, idx.long().unsqueeze(1).expand(-1, feature.shape[1], -1))

    @staticmethod
    def grouping_operation(feature, idx):
        B, S, K = idx.shape
        C = feature.shape[1]
        return torch.gather(feature, 2, idx.long().reshape(B, 1, S * K).expand(-1, C, -1)).view(B, C, S, K)


def _to_dev(d, dtype=None):
    def mv(v):
        v = v.cuda()
        return v.to(dtype) if dtype is not None and v.is_floating_point() else v
    return {k: (mv(v) if torch.is_tensor(v) else _to_dev(v, dtype)) for k, v in d.items()}


def _model():
    from hotrack_amd import pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    pointnet_utils.set_operator_backend(pointnet2_utils)
    torch.manual_seed(0)
    model = HandTrackNet(make_cfg("cuda"))
    deterministic_init(model)
    return model.cuda().eval()


def _fast(model, d, fold):
    """pred_kp of the point-major path with FastEval.fold_rearrange = fold."""
    from hotrack_amd import fused
    from models import pointnet_utils
    from models.fast_eval import FastEval
    before = FastEval.fold_rearrange
    try:
        FastEval.fold_rearrange = fold
        pointnet_utils.set_fused_backend(fused)
        with torch.no_grad():
            out = model(d, dict(FLAGS))["pred_kp"].clone()
        assert model._fast
        return out
    finally:
        FastEval.fold_rearrange = before
        pointnet_utils.set_fused_backend(None)


def _module64(model, d):
    """pred_kp of the module path in float64 (fused backend off)."""
    from hotrack_amd import pointnet2_utils
    from models import pointnet_utils
    m64 = copy.deepcopy(model)
    m64._fast = None
    m64 = m64.double().eval()
    from hotrack_amd import ext
    keep, keep_kabsch = torch.Tensor.float, ext.kabsch

    def kabsch64(x, y):
        """ext.kabsch's fit (hand_utils.solve_rot_and_trans) in its SVD form, float64 on the host."""
        x, y = x.double().cpu(), y.double().cpu()
        x = (x.unsqueeze(0) if x.dim() == 2 else x).expand(y.shape[0], -1, -1)
        cx, cy = x.mean(dim=1, keepdim=True), y.mean(dim=1, keepdim=True)
        u, _, vh = torch.linalg.svd(torch.bmm((x - cx).transpose(-1, -2), y - cy))
        v = vh.transpose(-1, -2)
        fix = torch.eye(3, dtype=torch.float64).repeat(y.shape[0], 1, 1)
        fix[:, 2, 2] = torch.det(torch.bmm(v, u.transpose(-1, -2)))
        R = torch.bmm(torch.bmm(v, fix), u.transpose(-1, -2))
        t = cy - torch.bmm(cx, R.transpose(-1, -2))
        return R.cuda(), t.transpose(-1, -2).cuda()

    try:
        torch.Tensor.float = lambda self: self  # the forward casts its inputs with .float(); keep float64 for this run
        torch.set_default_dtype(torch.float64)
        ext.kabsch = kabsch64
        pointnet_utils.set_operator_backend(_F64Ops)
        pointnet_utils.set_fused_backend(None)
        with torch.no_grad():
            out = m64(_to_dev(d, torch.float64), dict(FLAGS))["pred_kp"]
    finally:
        torch.Tensor.float, ext.kabsch = keep, keep_kabsch
        torch.set_default_dtype(torch.float32)
        pointnet_utils.set_operator_backend(pointnet2_utils)
    assert out.dtype == torch.float64
    return out


@pytest.mark.parametrize("B", [3, 32])
def test_both_routes_against_the_fp64_module_path(B):
    """B = 3: the small-batch route (large-route kernels off); B = 32: the smallest batch of the large route."""
    model = _model()
    frames = synthetic_frames(500 + B, B, 1024)
    d = _to_dev(frames)
    new, old = _fast(model, d, True), _fast(model, d, False)
    assert model._fast._large_batch(B, 1024) == (B == 32)
    ref = _module64(model, frames)
    e_new, e_old = float((new.double() - ref).abs().max()), float((old.double() - ref).abs().max())
    print(f"B={B}: |pred_kp - fp64 module path|: folded route {e_new:.3g}, gather route {e_old:.3g}; "
          f"routes apart {float((new - old).abs().max()):.3g}")
    assert e_new <= 2 * e_old + 1e-6


def test_graph_capture_of_the_folded_route_replays_on_other_inputs():
    from hotrack_amd import fused
    from models import pointnet_utils
    from models.fast_eval import FastEval
    assert FastEval.fold_rearrange is True
    model = _model()
    B = 3
    batches = [_to_dev(synthetic_frames(700 + i, B, 1024)) for i in range(3)]
    eager = [_fast(model, b, True) for b in batches]
    slot = _to_dev(synthetic_frames(700, B, 1024))
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


def test_in_place_edit_of_r1_refolds_the_products():
    model = _model()
    d = _to_dev(synthetic_frames(900, 3, 1024))
    before = _fast(model, d, True)
    r1c = model._fast.P["r1c"].clone()
    b1r = model._fast.P["q"][("q2", 0)]["b1r"].clone()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        model.r1.linear.weight.add_(0.05 * torch.randn(model.r1.linear.weight.shape, generator=g).cuda())
        model.r1.linear.bias.add_(0.05 * torch.randn(model.r1.linear.bias.shape, generator=g).cuda())
    after = _fast(model, d, True)
    assert not torch.equal(model._fast.P["r1c"], r1c) and not torch.equal(model._fast.P["q"][("q2", 0)]["b1r"], b1r)
    assert float((after - before).abs().max()) > 1e-5, "the edited r1 did not reach the output"
    model._fast = None  # a fresh FastEval on the edited network
    assert torch.equal(_fast(model, d, True), after)
