"""GPU: the training tail (csrc/tail_train.hip through hotrack_amd/tail_train.py and models.fast_train.FastTail) with its dropouts
ON, against the float64 references of tests/_tail_train_cases.py under the very masks the kernels draw -- the mask is an integer
function of (seed, site, element), restated on the host, so "statistically equivalent to torch" becomes an exact statement.

Bounds.  LayerNorm: what test_gpu_train.py::test_tail_ln_matches_torch holds with dropout off (out rtol = atol = 1e-5, each gradient
1e-4 of the reference's largest element).  relu_dropout's forward and dz, and the LayerNorm's dy against its dx: bit for bit.  Column
sums and the pose head: the running bounds K u A of _tail_train_cases.py (operation counts there), capped by the project's ceilings
(pose-head outputs rtol = atol = 1e-5, gradients 1e-4 of the largest element) -- the smaller of the two holds, element by element.
FastTail: test_fast_tail_equals_module_tail's bounds.  Every comparison prints `case quantity: err <e> bound <b> ratio <r>`."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tail_train_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
DEV = "cuda"
SEEDS = (5, (1 << 33) + 7, (1 << 62) - 1)
RATIOS = {}  # kernel -> largest error / bound seen (printed by each test for the log)


def _hold(kernel, case, name, got, want, bound):
    ratio, err, b = TC.worst(got, want, bound)
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print(f"{case} {name}: err {err:.3g} bound {b:.3g} ratio {ratio:.3g}")
    assert ratio <= 1.0, (case, name, err, b)
    return ratio


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _grad_ceiling(want):
    return 1e-4 * (float(want.abs().max()) + 1e-12)


# ---- dropout(relu(z + bias)) ---------------------------------------------------------------------------------------------------------
def _relu_expected(z, bias, mask, p, dh=None):
    """The kernel's float32 arithmetic on the host: fp32(z + b), relu, fp32(. * scale32) where kept; dz likewise from dh."""
    v = z.numpy() + (bias.numpy() if bias is not None else np.float32(0))
    assert v.dtype == np.float32
    s = TC.scale32(p)
    out = np.where(mask.numpy(), np.where(v > 0, v, np.float32(0)) * s, np.float32(0)).astype(np.float32)
    dz = None if dh is None else np.where(mask.numpy() & (v > 0), dh.numpy() * s, np.float32(0)).astype(np.float32)
    return torch.from_numpy(out), (None if dz is None else torch.from_numpy(dz)), torch.from_numpy(v > 0)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,C", [(1, 4), (5, 260), (17, 1024), (33, 8)])
def test_relu_dropout_under_its_own_mask(rows, C, p):
    """Forward and dz bit for bit under keep_mask, dbias within 2 rows u sum|terms| (and the 1e-4 ceiling): every seed, site 1 and 3,
    with and without bias."""
    from hotrack_amd import tail_train as T
    g = torch.Generator().manual_seed(rows * C)
    # 60 % of z + bias positive by construction, |z + bias| >= 0.05: the forward shows the mask only there
    sign = torch.where((torch.arange(rows * C) * 7 % 5) < 3, 1.0, -1.0).view(rows, C)
    target = sign * (0.05 + torch.randn(rows, C, generator=g).abs())
    b0 = torch.randn(C, generator=g)
    dh = torch.randn(rows, C, generator=g)
    for seed in SEEDS:
        for site in (1, 3):
            for with_bias in (True, False):
                case = f"relu_drop rows={rows} C={C} p={p} seed={seed} site={site} bias={with_bias}"
                bias = b0 if with_bias else None
                z = (target - b0) if with_bias else target
                mask = TC.mask_tensor(seed, site, (rows, C), p)
                want_out, want_dz, pos = _relu_expected(z, bias, mask, p, dh)
                assert float(pos.float().mean()) >= 0.4, case
                zc = z.to(DEV).requires_grad_(True)
                bc = None if bias is None else bias.to(DEV).requires_grad_(True)
                grads = T.TailGrads(DEV, 2 * C)
                out = T.relu_dropout(zc, bc, p, site, _seed(seed), grads)
                out.backward(dh.to(DEV))
                assert torch.equal(_bits(out), _bits(want_out)), case
                assert torch.equal(_bits(zc.grad), _bits(want_dz)), case
                ref = TC.relu_drop_reference(z, bias, p, site, seed, dh=dh)
                # the two host forms agree: one rounding each for z + b, scale32 and the product, of terms |z| + |b| at the most
                assert float((want_out.double() - ref["out"]).abs().max()) <= 4 * TC.U * TC.scale64(p) * float(z.abs().max() + b0.abs().max()), case
                if with_bias:
                    bound = torch.minimum(TC.relu_drop_dbias_bound(rows, ref["dbias_abs"]), torch.full((C,), _grad_ceiling(ref["dbias"]), dtype=f64))
                    _hold("relu_dropout", case, f"dbias (K={2 * rows})", bc.grad, ref["dbias"], bound)
                    assert grads.used == C and not bool(grads.buf[C:].any())
                else:
                    assert grads.used == 0 and not bool(grads.buf.any())
    print(f"relu_dropout: largest error / bound so far {RATIOS.get('relu_dropout', 0.0):.3g}")


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_relu_dropout_signed_zeros(p):
    """z + bias exactly +0 and -0: 0 forward, 0 gradient, whatever the mask says."""
    from hotrack_amd import tail_train as T
    rows, C = 3, 8
    g = torch.Generator().manual_seed(8)
    bias = torch.randn(C, generator=g)
    bias[5] = -0.0
    z = torch.randn(rows, C, generator=g) - bias
    z[0, 1], z[1, 2], z[2, 7] = -bias[1], -bias[2], -bias[7]            # x + (-x) = +0
    z[:, 5] = torch.tensor([-0.0, 0.0, -0.0])                             # -0 + -0 = -0;  +0 + -0 = +0
    zero = torch.zeros(rows, C, dtype=torch.bool)
    zero[0, 1] = zero[1, 2] = zero[2, 7] = True
    zero[:, 5] = True
    v = (z + bias).numpy()
    assert (v[zero.numpy()] == 0).all() and np.signbit(v[0, 5]) and not np.signbit(v[1, 5]) and not np.signbit(v[0, 1])
    for with_bias in (True, False):
        zz = z if with_bias else (z + bias)
        zc = zz.to(DEV).requires_grad_(True)
        bc = bias.to(DEV).requires_grad_(True) if with_bias else None
        grads = T.TailGrads(DEV, C)
        out = T.relu_dropout(zc, bc, p, 1, _seed(5) if p else None, grads)
        dh = torch.randn(rows, C, generator=g)
        out.backward(dh.to(DEV))
        assert bool((_bits(out)[zero] == 0).all()) and bool((_bits(zc.grad)[zero] == 0).all()), (p, with_bias)
        mask = TC.mask_tensor(5, 1, (rows, C), p)
        want_out, want_dz, _ = _relu_expected(zz, bias if with_bias else None, mask, p, dh)
        assert torch.equal(_bits(out), _bits(want_out)) and torch.equal(_bits(zc.grad), _bits(want_dz))


# ---- LN_b(LN_a(x + dropout(y + bias))) ----------------------------------------------------------------------------------------------
LN_SHAPES = [(1, 64), (1, 100), (1, 512), (7, 64), (7, 129), (7, 384), (9, 100), (9, 129), (9, 512), (672, 64), (672, 384), (672, 512)]


def _ln_inputs(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(rows, C), "y": r(rows, C), "bias": r(C), "ga": 1 + 0.3 * r(C), "ba": 0.2 * r(C), "gb": 1 + 0.3 * r(C), "bb": 0.2 * r(C),
            "go": r(rows, C)}


def _ln_modules(C, d, eps_b=1e-5):
    na, nb = torch.nn.LayerNorm(C).to(DEV), torch.nn.LayerNorm(C, eps=eps_b).to(DEV)
    with torch.no_grad():
        na.weight.copy_(d["ga"]); na.bias.copy_(d["ba"]); nb.weight.copy_(d["gb"]); nb.bias.copy_(d["bb"])
    return na, nb


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,C", LN_SHAPES)
def test_ln_with_dropout_matches_fp64_under_its_mask(rows, C, p):
    """One and two LayerNorms, y with and without bias, sites 2 and 4: out and every gradient at the dropout-off bounds; dy is +0
    where the mask drops and fp32(dx * scale32) where it keeps, bit for bit (the backward regenerates the forward's mask and scale)."""
    from hotrack_amd import tail_train as T
    d = _ln_inputs(rows, C, rows * 1000 + C)
    s32 = torch.tensor(float(TC.scale32(p)), dtype=torch.float32)
    k = 0
    for two in (True, False):
        for with_bias in (True, False):
            for site in (2, 4):
                seed = SEEDS[k % 3]
                k += 1
                case = f"ln rows={rows} C={C} p={p} two={two} bias={with_bias} site={site} seed={seed}"
                na, nb = _ln_modules(C, d)
                x, y = d["x"].to(DEV).requires_grad_(True), d["y"].to(DEV).requires_grad_(True)
                bias = d["bias"].to(DEV).requires_grad_(True) if with_bias else None
                grads = T.TailGrads(DEV, 8 * C)
                out = T.ln(x, na, nb if two else None, grads, y=y, bias=bias, p=p, site=site, seed_in=_seed(seed))
                out.backward(d["go"].to(DEV))
                ref = TC.ln_reference(d["x"], d["ga"], d["ba"], na.eps, d["gb"] if two else None, d["bb"] if two else None, nb.eps,
                                      y=d["y"], bias=d["bias"] if with_bias else None, p=p, site=site, seed=seed, go=d["go"])
                _hold("ln", case, "out", out, ref["out"], 1e-5 + 1e-5 * ref["out"].abs())
                got = {"dx": x.grad, "dy": y.grad, "dbias": None if bias is None else bias.grad, "dga": na.weight.grad, "dba": na.bias.grad,
                       "dgb": nb.weight.grad, "dbb": nb.bias.grad}
                for name, a in got.items():
                    if ref[name] is None:
                        assert a is None, (case, name)
                        continue
                    assert a is not None, (case, name)
                    _hold("ln", case, name, a, ref[name], _grad_ceiling(ref[name]))
                # exact: the backward's mask and scale are the forward's
                m = ref["mask"]
                dy, dx = y.grad.cpu(), x.grad.cpu()
                assert bool((_bits(dy)[~m] == 0).all()), case                       # +0.0, not -0.0, not a small number
                assert torch.equal(_bits(dy)[m], _bits(dx * s32)[m]), case
                assert rows * C < 512 or 0 < int(m.sum()) < m.numel()
                # accumulators: a, b of each LayerNorm, dbias only with a bias; nothing written past them
                assert grads.used == (2 + 2 * two + with_bias) * C and not bool(grads.buf[grads.used:].any()), case
    print(f"ln: largest error / bound so far {RATIOS.get('ln', 0.0):.3g}")


@pytest.mark.parametrize("C", [513, 1024])
def test_ln_wide_rows_forward_only(C):
    """C in 513 .. 1024 has a forward (16 elements per lane) and no backward: the forward matches float64 with dropout off and on;
    a call that would need the backward is refused up front, and the C entry returns PN2_EINVAL and writes nothing."""
    from hotrack_amd import tail_train as T
    from hotrack_amd.pointnet2_hip import Pn2Error
    rows = 9
    d = _ln_inputs(rows, C, C)
    na, nb = _ln_modules(C, d)
    with torch.no_grad():
        for p, with_y, two in ((0.0, False, True), (0.0, True, False), (0.1, True, True), (0.5, True, False)):
            grads = T.TailGrads(DEV, 8 * C)
            out = T.ln(d["x"].to(DEV), na, nb if two else None, grads, y=d["y"].to(DEV) if with_y else None, bias=d["bias"].to(DEV) if with_y else None,
                       p=p, site=2, seed_in=_seed(SEEDS[1]) if with_y else None)
            ref = TC.ln_reference(d["x"], d["ga"], d["ba"], na.eps, d["gb"] if two else None, d["bb"] if two else None, nb.eps,
                                  y=d["y"] if with_y else None, bias=d["bias"] if with_y else None, p=p, site=2, seed=SEEDS[1])
            _hold("ln", f"ln forward rows={rows} C={C} p={p} y={with_y} two={two}", "out", out, ref["out"], 1e-5 + 1e-5 * ref["out"].abs())
    grads = T.TailGrads(DEV, 8 * C)
    with pytest.raises(Pn2Error, match="512"):
        T.ln(d["x"].to(DEV).requires_grad_(True), na, None, grads)
    with pytest.raises(Pn2Error, match="512"):
        T.ln(d["x"].to(DEV), na, nb, grads)                               # the LayerNorms' own parameters require grad
    assert grads.used == 0 and not bool(grads.buf.any())
    # the C entry
    lib = T._lib
    t = lambda *s: torch.full(s, 7.0, device=DEV)
    x, stats, dout = d["x"].to(DEV), t(rows, 4), d["go"].to(DEV)
    outs = [t(rows, C), t(C), t(C)]
    rc = lib.pn2x_tail_ln_bwd(rows, C, x.data_ptr(), None, None, 0.0, 0, None, na.weight.data_ptr(), na.bias.data_ptr(), 1e-5, None, None, 0.0,
                              stats.data_ptr(), dout.data_ptr(), outs[0].data_ptr(), None, outs[1].data_ptr(), outs[2].data_ptr(), None, None, None, None)
    torch.cuda.synchronize()
    assert rc == -1 and all(bool((o == 7.0).all()) for o in outs)


# ---- the training pose head ------------------------------------------------------------------------------------------------------
class _Unused(torch.autograd.Function):
    """A consumer of both outputs that sends no gradient to either."""

    @staticmethod
    def forward(ctx, a, b):
        return a.sum() + b.sum()

    @staticmethod
    def backward(ctx, g):
        return None, None


@pytest.mark.parametrize("B,J,C", [(1, 1, 1), (2, 5, 100), (3, 21, 384), (5, 21, 384), (2, 33, 257)])
def test_pose_head_training_matches_fp64(B, J, C):
    """kp_hand, kp_cam, dh, dw, dbias within the running bounds (capped by the ceilings) for one scale and a scale per cloud, with
    the backward through kp_hand alone, kp_cam alone and both; h's gradient is zeros when neither output sends one."""
    from hotrack_amd import tail_train as T
    g = torch.Generator().manual_seed(B * 100 + J + C)
    r = lambda *s: torch.randn(*s, generator=g)
    h0, w0, b0, xyz1 = torch.relu(r(B * J, C)) + 0.1 * r(B * J, C), r(3, C) / math.sqrt(C), 0.1 * r(3), 0.4 * r(B, 3, J)
    R, t = torch.linalg.qr(r(B, 3, 3))[0].contiguous(), 0.1 * r(B, 3, 1) + torch.tensor([0.0, 0.0, 0.5]).view(1, 3, 1)
    gh, gc = r(B, 3, J), r(B, J, 3)
    for scale in (torch.tensor([0.2]), 0.1 + 0.3 * torch.rand(B, generator=g)):
        for mode in ("hand", "cam", "both"):
            case = f"pose_head B={B} J={J} C={C} scale{tuple(scale.shape)} grad={mode}"
            h, w, bias = (v.to(DEV).requires_grad_(True) for v in (h0, w0, b0))
            grads = T.TailGrads(DEV, 3 * C + 3 + 5)
            kh, kc = T.pose_head(h, w, bias, xyz1.to(DEV), R.to(DEV), t.to(DEV), scale.to(DEV), grads)
            assert kh.shape == (B, 3, J) and kc.shape == (B, J, 3)
            use_h, use_c = mode in ("hand", "both"), mode in ("cam", "both")
            sum(((o * g_.to(DEV)).sum() for o, g_, used in ((kh, gh, use_h), (kc, gc, use_c)) if used)).backward()
            ref = TC.pose_head_reference(h0, w0, b0, xyz1, R, t, scale, gh if use_h else None, gc if use_c else None)
            bounds, K = TC.pose_head_bounds(B, J, C, ref, cam_grad=use_c)
            for name, got in (("kp_hand", kh), ("kp_cam", kc), ("dh", h.grad), ("dw", w.grad), ("dbias", bias.grad)):
                want = ref[name]
                assert got.shape == want.shape, (case, name)
                ceiling = (1e-5 + 1e-5 * want.abs()) if name.startswith("kp") else torch.full_like(want, _grad_ceiling(want))
                _hold("pose_head", case, f"{name} (K={K[name]})", got, want, torch.minimum(bounds[name], ceiling))
            assert not bool(grads.buf[3 * C + 3:].any())
    h = h0.to(DEV).requires_grad_(True)
    w = w0.to(DEV).requires_grad_(True)
    kh, kc = T.pose_head(h, w, b0.to(DEV), xyz1.to(DEV), R.to(DEV), t.to(DEV), torch.tensor([0.2], device=DEV), T.TailGrads(DEV, 3 * C + 3))
    _Unused.apply(kh, kc).backward()
    assert h.grad is not None and h.grad.shape == h.shape and not bool(h.grad.any())
    assert w.grad is None or not bool(w.grad.any())
    print(f"pose_head: largest error / bound so far {RATIOS.get('pose_head', 0.0):.3g}")


# ---- FastTail with its dropouts on ---------------------------------------------------------------------------------------------------
def test_fast_tail_with_dropout_matches_fp64_and_resumes():
    """FastTail.forward + backward under the modules' own p against tail_reference at the counter value the forward used; the counter
    advances by one per forward, rewinds in place, and a fresh FastTail given dropout_state() continues the stream."""
    from _netinit import deterministic_init, make_cfg
    from models.hand_network import HandTrackNet
    from models.fast_train import FastTail
    torch.manual_seed(0)
    net = HandTrackNet(make_cfg("cuda"))
    deterministic_init(net)
    net = net.cuda().train()
    drops = [net.transt.c11.dropout2, net.transt.c11.dropout3, net.c3.dropout2, net.c3.dropout3]
    for m in drops:
        if m.p == 0:
            m.p = 0.1
    assert all(0 < m.p < 1 and m.training for m in drops)
    g = torch.Generator(device="cuda").manual_seed(1)
    B, J, C = 5, 21, 384
    rows = torch.randn(B * J, C, device="cuda", generator=g)
    xyz1 = torch.randn(B, 3, J, device="cuda", generator=g)
    rot = torch.linalg.qr(torch.randn(B, 3, 3, device="cuda", generator=g))[0]
    canon = {"scale": 0.2 * torch.ones(1, device="cuda"), "rotation": rot, "translation": torch.randn(B, 3, 1, device="cuda", generator=g)}
    assert FastTail.supported(net)

    def loss(hf, kp):
        return ((hf * torch.cos(torch.arange(hf.numel(), device=hf.device).view_as(hf) * 0.1)).sum()
                + (kp * torch.sin(torch.arange(kp.numel(), device=kp.device).view_as(kp) * 0.3)).sum())

    def outputs_match(tag, got, seed):
        hf_r, kp_r, leaves = TC.tail_reference(net, rows, xyz1, canon, seed)
        _hold("fast_tail", tag, "kp_hand", got[0], hf_r.detach(), 1e-5 + 1e-5 * hf_r.detach().abs())
        _hold("fast_tail", tag, "kp_cam", got[1], kp_r.detach(), 1e-5 + 1e-5 * kp_r.detach().abs())
        return hf_r, kp_r, leaves

    v = (1 << 40) + 12345
    tail = FastTail(net)
    tail.set_dropout_state(v)
    assert tail.dropout_state() == v
    net.zero_grad()
    r_ = rows.clone().requires_grad_(True)
    first = tail.forward(r_, xyz1, canon)
    loss(*first).backward()
    assert tail.dropout_state() == v + 1
    hf_r, kp_r, leaves = outputs_match("fast_tail forward 1", first, v + 1)
    loss(hf_r, kp_r).backward()
    _hold("fast_tail", "fast_tail backward", "d rows", r_.grad, leaves["rows"].grad, _grad_ceiling(leaves["rows"].grad))
    got = {k: p_.grad for k, p_ in net.named_parameters() if p_.grad is not None}
    assert set(got) == set(leaves) - {"rows"} and len(got) > 15
    for k in sorted(got):
        _hold("fast_tail", "fast_tail backward", k, got[k], leaves[k].grad, _grad_ceiling(leaves[k].grad))
    # the dropout matters at these bounds: the same forward without it is far outside them
    hf_0, _, _ = TC.tail_reference(net.eval(), rows, xyz1, canon, v + 1)
    net.train()
    assert float((hf_0.detach() - hf_r.detach()).abs().max()) > 1e-3
    first = [o.detach().clone() for o in first]
    second = [o.detach().clone() for o in tail.forward(rows, xyz1, canon)]
    assert tail.dropout_state() == v + 2
    outputs_match("fast_tail forward 2", second, v + 2)
    assert float((second[0] - first[0]).abs().max()) > 1e-3
    # rewind (no snapshot: back to the value the counter was created with), in place
    seed_tensor = tail.seed
    tail.rewind_dropout_counter()
    assert tail.seed is seed_tensor and tail.dropout_state() == v
    again = tail.forward(rows, xyz1, canon)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and tail.dropout_state() == v + 1
    # rewind to a snapshot taken earlier
    snap = tail.seed.clone()
    tail.forward(rows, xyz1, canon)
    tail.forward(rows, xyz1, canon)
    tail.rewind_dropout_counter(snap)
    assert tail.seed is seed_tensor and tail.dropout_state() == v + 1
    # resume: a fresh FastTail handed the saved state draws the next forward's masks
    resumed = FastTail(net)
    resumed.set_dropout_state(tail.dropout_state())
    assert resumed.dropout_state() == v + 1
    cont = resumed.forward(rows, xyz1, canon)
    assert torch.equal(cont[0], second[0]) and torch.equal(cont[1], second[1]) and resumed.dropout_state() == v + 2
    # set_dropout_state on a live counter writes it in place
    live = resumed.seed
    resumed.set_dropout_state(v)
    assert resumed.seed is live and resumed.dropout_state() == v
    back = resumed.forward(rows, xyz1, canon)
    assert torch.equal(back[0], first[0]) and torch.equal(back[1], first[1])
    print(f"fast_tail: largest error / bound {RATIOS.get('fast_tail', 0.0):.3g}")


# ---- the C entries refuse bad calls and launch nothing -------------------------------------------------------------------------------
def test_c_entries_refuse_and_write_nothing():
    from hotrack_amd import tail_train as T
    lib = T._lib
    EINVAL, ENULL = -1, -2
    rows, C = 6, 8
    fill = lambda *s: torch.full(s, 7.0, device=DEV)
    x, y, bias, ga, ba, dout = (torch.randn(*s, device=DEV) for s in ((rows, C), (rows, C), (C,), (C,), (C,), (rows, C)))
    seed = _seed(5)
    out, stats, dx, dy, dga, dba, dbias = fill(rows, C), fill(rows, 4), fill(rows, C), fill(rows, C), fill(C), fill(C), fill(C)
    written = (out, stats, dx, dy, dga, dba, dbias)
    P = lambda t_: None if t_ is None else t_.data_ptr()

    def ln_fwd(rows_=rows, c=C, p=0.1, y_=y, seed_in=seed):
        return lib.pn2x_tail_ln_fwd(rows_, c, P(x), P(y_), P(bias), p, 2, P(seed_in), None, None, P(ga), P(ba), 1e-5, None, None, 0.0, P(out),
                                    P(stats), None)

    def ln_bwd(rows_=rows, c=C, p=0.1, y_=y, seed_in=seed):
        return lib.pn2x_tail_ln_bwd(rows_, c, P(x), P(y_), P(bias), p, 2, P(seed_in), P(ga), P(ba), 1e-5, None, None, 0.0, P(stats), P(dout),
                                    P(dx), P(dy), P(dga), P(dba), None, None, P(dbias), None)

    def relu_fwd(rows_=rows, c=C, p=0.1, z=None, o=None, seed_in=seed):
        return lib.pn2x_tail_relu_drop_fwd(rows_, c, P(x) if z is None else z, P(bias), p, 1, P(seed_in), P(out) if o is None else o, None)

    def relu_bwd(rows_=rows, c=C, p=0.1, z=None, dz=None, seed_in=seed):
        return lib.pn2x_tail_relu_drop_bwd(rows_, c, P(x) if z is None else z, P(bias), p, 1, P(seed_in), P(dout), P(dx) if dz is None else dz,
                                           P(dbias), None)

    for p in (1.0, -0.1, float("nan")):
        for f in (ln_fwd, ln_bwd, relu_fwd, relu_bwd):
            assert f(p=p) == EINVAL, (f.__name__, p)
    for c in (0, 1025):
        assert ln_fwd(c=c) == EINVAL and ln_bwd(c=c) == EINVAL, c
    assert ln_bwd(c=1024) == EINVAL and ln_bwd(c=513) == EINVAL           # the forward's widest variant has no backward
    assert relu_fwd(c=6) == EINVAL and relu_bwd(c=6) == EINVAL
    assert relu_fwd(z=x.data_ptr() + 4) == EINVAL and relu_fwd(o=out.data_ptr() + 4) == EINVAL
    assert relu_bwd(z=x.data_ptr() + 4) == EINVAL and relu_bwd(dz=dx.data_ptr() + 4) == EINVAL
    assert ln_fwd(seed_in=None) == ENULL and ln_bwd(seed_in=None) == ENULL    # p > 0, y present, no seed
    assert relu_fwd(seed_in=None) == ENULL and relu_bwd(seed_in=None) == ENULL
    for f in (ln_fwd, ln_bwd, relu_fwd, relu_bwd):
        assert f(rows_=0) == 0, f.__name__
    # pose head: backward with neither gradient
    B, J = 2, 3
    h, w = torch.randn(B * J, C, device=DEV), torch.randn(3, C, device=DEV)
    R, sc = torch.eye(3, device=DEV).repeat(B, 1, 1), torch.ones(1, device=DEV)
    dh, dw, db = fill(B * J, C), fill(3, C), fill(3)
    assert lib.pn2x_tail_pose_head_bwd(B, J, C, P(h), P(w), None, None, P(R), P(sc), 0, P(dh), P(dw), P(db), None) == ENULL
    assert lib.pn2x_tail_pose_head_bwd(0, J, C, P(h), P(w), None, None, P(R), P(sc), 0, P(dh), P(dw), P(db), None) == 0
    torch.cuda.synchronize()
    for t_ in written + (dh, dw, db):
        assert bool((t_ == 7.0).all())
