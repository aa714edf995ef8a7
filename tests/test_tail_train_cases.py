"""CPU: tests/_tail_train_cases.py itself -- the dropout keep-mask restated on the host against a known answer and against plain
Python integers, its thresholds and keep rates, and the float64 references at p = 0 against the plain torch compositions they
restate (nn.LayerNorm, relu, decanonicalize, and the module tail of test_gpu_train.py::test_fast_tail_equals_module_tail)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tail_train_cases as TC  # noqa: E402

f64 = torch.float64


def test_hash_known_answer_is_splitmix64():
    """seed 1, site 0, element 0 is SplitMix64's state after one step from 0: its first output."""
    z = TC.mix64(1, 0, np.zeros(1, dtype=np.uint64))
    assert int(z[0]) == 0xE220A8397B1DCDAF and int(z[0]) >> 32 == 0xE220A839
    assert TC.mix64_int(1, 0, 0) == 0xE220A8397B1DCDAF


def test_numpy_hash_equals_python_integers():
    rng = random.Random(0)
    seeds = [0, 1, 5, (1 << 32) - 1, 1 << 32, (1 << 33) + 7, (1 << 62) - 1, (1 << 62) - 2, (1 << 63) - 1, -1]
    seeds += [rng.getrandbits(62) for _ in range(10)]
    elems = [0, 1, 63, 64, 672 * 1024 - 1, (1 << 31) - 1, 1 << 31, (1 << 40) - 1, 1 << 40] + [rng.getrandbits(30) for _ in range(6)]
    n = 0
    for seed in seeds:
        for site in (0, 1, 2, 3, 4):
            got = TC.mix64(seed, site, np.array(elems, dtype=np.uint64))
            for i, g in zip(elems, got):
                assert int(g) == TC.mix64_int(seed, site, i), (seed, site, i)
                n += 1
    assert n >= 300
    # keep_mask is the high word of that hash against the threshold, element by element
    for seed, site, p in ((5, 1, 0.1), ((1 << 33) + 7, 4, 0.5), ((1 << 62) - 1, 3, 0.1)):
        m = TC.keep_mask(seed, site, 257, p)
        want = [(TC.mix64_int(seed, site, i) >> 32) >= TC.drop_threshold(p) for i in range(257)]
        assert m.dtype == np.bool_ and m.tolist() == want


def test_thresholds_and_keep_rates():
    assert TC.drop_threshold(0.0) == 0 and TC.drop_threshold(-0.5) == 0
    assert TC.drop_threshold(0.5) == 1 << 31
    assert TC.drop_threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32) == 429496736   # float32(0.1) = 0.100000001490116...
    assert TC.keep_mask(9, 2, 4096, 0.0).all()
    n = 1 << 20
    for p in (0.1, 0.5):
        rate = TC.keep_mask(77, 1, n, p).mean()
        tol = 4 * (p * (1 - p) / n) ** 0.5
        print(f"p={p}: keep rate {rate:.6f}, |rate - (1 - p)| = {abs(rate - (1 - p)):.2e} <= {tol:.2e}")
        assert abs(rate - (1 - p)) <= tol
    for p in (0.1, 0.5):
        base = TC.keep_mask(77, 1, n, p)
        for other in (TC.keep_mask(77, 2, n, p), TC.keep_mask(77, 3, n, p), TC.keep_mask(78, 1, n, p), TC.keep_mask(76, 1, n, p)):
            assert (base ^ other).mean() > 0.05
    assert TC.scale32(0.1).dtype == np.float32 and TC.scale32(0.5) == 2.0
    assert abs(TC.scale64(0.1) - 1 / (1 - float(np.float32(0.1)))) == 0


def _randn(g, *s):
    return torch.randn(*s, generator=g)


@pytest.mark.parametrize("rows,C,two,with_y,with_bias", [(9, 100, True, True, True), (7, 129, False, True, False), (3, 64, True, False, False)])
def test_ln_reference_without_dropout_is_torch_layernorm(rows, C, two, with_y, with_bias):
    g = torch.Generator().manual_seed(rows * C)
    x, y, bias, go = _randn(g, rows, C), _randn(g, rows, C), _randn(g, C), _randn(g, rows, C)
    na, nb = torch.nn.LayerNorm(C, eps=1e-5).double(), torch.nn.LayerNorm(C, eps=3e-5).double()
    with torch.no_grad():
        for m in (na, nb):
            m.weight.copy_(1 + 0.3 * _randn(g, C).float().double())
            m.bias.copy_(0.2 * _randn(g, C).float().double())
    ref = TC.ln_reference(x, na.weight, na.bias, na.eps, nb.weight if two else None, nb.bias if two else None, nb.eps,
                          y=y if with_y else None, bias=bias if with_bias else None, p=0.0, site=2, seed=123, go=go)
    xd, yd, bd = (t.double().requires_grad_(True) for t in (x, y, bias))
    u = xd + ((yd + bd if with_bias else yd) if with_y else 0)
    out = nb(na(u)) if two else na(u)
    out.backward(go.double())
    assert ref["mask"].all()
    want = {"out": out.detach(), "dx": xd.grad, "dy": yd.grad if with_y else None, "dbias": bd.grad if with_bias else None,
            "dga": na.weight.grad, "dba": na.bias.grad, "dgb": nb.weight.grad if two else None, "dbb": nb.bias.grad if two else None}
    for k, w in want.items():
        if w is None:
            assert ref[k] is None, k
        else:
            assert float((ref[k] - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), k


def test_ln_reference_applies_mask_and_scale():
    """With p > 0: dropped elements of y do not reach the output and get no gradient; kept ones carry 1 / (1 - p)."""
    g = torch.Generator().manual_seed(4)
    rows, C, p = 5, 100, 0.5
    x, y, go = _randn(g, rows, C), _randn(g, rows, C), _randn(g, rows, C)
    ga, ba = torch.ones(C), torch.zeros(C)
    ref = TC.ln_reference(x, ga, ba, 1e-5, y=y, p=p, site=4, seed=11, go=go)
    m = ref["mask"]
    assert m.shape == (rows, C) and m.flatten().tolist() == TC.keep_mask(11, 4, rows * C, p).tolist() and 0.3 < m.float().mean() < 0.7
    assert (ref["dy"][~m] == 0).all() and torch.equal(ref["dy"][m], ref["dx"][m] * 2.0)
    want = torch.nn.functional.layer_norm(x.double() + torch.where(m, 2.0 * y.double(), torch.zeros((), dtype=f64)), (C,), None, None, 1e-5)
    assert float((ref["out"] - want).abs().max()) <= 1e-12


def test_relu_drop_reference():
    g = torch.Generator().manual_seed(5)
    z, bias, dh = _randn(g, 6, 8), _randn(g, 8), _randn(g, 6, 8)
    ref = TC.relu_drop_reference(z, bias, 0.0, 1, 3, dh=dh)
    zd, bd = z.double().requires_grad_(True), bias.double().requires_grad_(True)
    out = torch.relu(zd + bd)
    out.backward(dh.double())
    assert torch.equal(ref["out"], out.detach()) and torch.equal(ref["dz"], zd.grad)
    assert float((ref["dbias"] - bd.grad).abs().max()) <= 1e-14
    assert bool((ref["dbias_abs"] >= ref["dbias"].abs() - 1e-14).all())
    ref = TC.relu_drop_reference(z, None, 0.5, 3, 9, dh=dh)
    m = torch.from_numpy(TC.keep_mask(9, 3, 48, 0.5)).view(6, 8)
    assert ref["dbias"] is None and torch.equal(ref["out"], torch.where(m, 2.0 * torch.relu(z.double()), torch.zeros((), dtype=f64)))
    assert torch.equal(ref["dz"], torch.where(m & (z > 0), 2.0 * dh.double(), torch.zeros((), dtype=f64)))


@pytest.mark.parametrize("B,J,C,per_cloud", [(2, 5, 100, True), (3, 21, 16, False), (1, 1, 1, True)])
def test_pose_head_reference_is_linear_plus_decanonicalize(B, J, C, per_cloud):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "network"))
    from models.hand_utils import decanonicalize
    g = torch.Generator().manual_seed(B * J + C)
    h, w, bias, xyz1 = _randn(g, B * J, C), _randn(g, 3, C), _randn(g, 3), _randn(g, B, 3, J)
    R, t = torch.linalg.qr(_randn(g, B, 3, 3))[0], _randn(g, B, 3, 1)
    scale = 0.5 + torch.rand(B if per_cloud else 1, generator=g)
    gh, gc = _randn(g, B, 3, J), _randn(g, B, J, 3)
    ref = TC.pose_head_reference(h, w, bias, xyz1, R, t, scale, gh, gc)
    hd, wd, bd = (v.double().requires_grad_(True) for v in (h, w, bias))
    feat = hd.view(B, J, C).transpose(1, 2)                                             # (B, C, J), as the module sees it
    hf = torch.nn.functional.conv1d(feat, wd.unsqueeze(-1), bd) + xyz1.double()
    canon = {"scale": scale.double().expand(B) if not per_cloud else scale.double(), "rotation": R.double(), "translation": t.double()}
    kp = decanonicalize(hf, canon).transpose(2, 1)
    ((hf * gh.double()).sum() + (kp * gc.double()).sum()).backward()
    for k, want in (("kp_hand", hf.detach()), ("kp_cam", kp.detach()), ("dh", hd.grad), ("dw", wd.grad), ("dbias", bd.grad)):
        assert ref[k].shape == want.shape, k
        assert float((ref[k] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k
        assert bool((ref["abs"][k] >= ref[k].abs() * (1 - 1e-12)).all()), k                 # |sum| <= sum of |terms|
    bounds, K = TC.pose_head_bounds(B, J, C, ref, cam_grad=True)
    assert K == {"kp_hand": 2 * (C + 2), "kp_cam": 2 * (C + 9), "dh": 24, "dw": 2 * (7 + B * J), "dbias": 2 * (6 + B * J)}
    assert set(bounds) == set(K) and all(bounds[k].shape == ref[k].shape for k in K)


def test_tail_reference_without_dropout_is_the_module_tail():
    """tail_reference with every Dropout at p = 0 against TransT -> c3 -> final_mlp -> decanonicalize in float64 (the composition of
    test_fast_tail_equals_module_tail): outputs, the input gradient and every parameter gradient to 1e-12."""
    from _netinit import deterministic_init, make_cfg
    from models.hand_network import HandTrackNet
    from models.hand_utils import decanonicalize
    import torch.nn.functional as F
    torch.manual_seed(0)
    net = HandTrackNet(make_cfg("cpu"))
    deterministic_init(net)
    net = net.double().train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    g = torch.Generator().manual_seed(1)
    B, J = 2, 21
    C = net.transt.c11.norm1.normalized_shape[0]
    rows, xyz1 = _randn(g, B * J, C), _randn(g, B, 3, J)
    canon = {"scale": 0.2 * torch.ones(1), "rotation": torch.linalg.qr(_randn(g, B, 3, 3))[0], "translation": _randn(g, B, 3, 1)}

    def loss(hf, kp):
        return ((hf * torch.cos(torch.arange(hf.numel()).view_as(hf) * 0.1)).sum()
                + (kp * torch.sin(torch.arange(kp.numel()).view_as(kp) * 0.3)).sum())

    hf_r, kp_r, leaves = TC.tail_reference(net, rows, xyz1, canon, seed=7)
    loss(hf_r, kp_r).backward()
    r_ = rows.double().requires_grad_(True)
    f14 = r_.view(B, J, C).transpose(1, 2)
    f15, f251 = net.transt(src1=f14, pos1=None, src2=None, pos2=None, attn=False, elide_dead=True, need_result2=False)
    fused = net.c3(f15, None, f251, None, attn=False, elide_dead=True)
    lin = lambda conv, x: F.linear(x.transpose(1, 2), conv.weight.squeeze(-1), conv.bias).transpose(1, 2)
    hf = lin(net.final_mlp[2], F.relu(lin(net.final_mlp[0], fused))) + xyz1.double()
    kp = decanonicalize(hf, {k: v.double() for k, v in canon.items()}).transpose(2, 1)
    net.zero_grad()
    loss(hf, kp).backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert hf_r.shape == hf.shape and kp_r.shape == kp.shape and close(hf_r.detach(), hf.detach()) and close(kp_r.detach(), kp.detach())
    assert close(leaves["rows"].grad, r_.grad)
    want = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert set(want) == set(leaves) - {"rows"} and len(want) > 15
    for k, w in want.items():
        assert leaves[k].grad.shape == w.shape and close(leaves[k].grad, w), k
