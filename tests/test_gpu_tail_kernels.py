"""GPU: the fused element-wise kernels of the 21-token tail (hotrack_amd/csrc/tail.hip: pn2x_add_layernorm, pn2x_pose_head) against
float64, at their edges: add_layernorm across the boundaries of its four template instances (c <= 128, 256, 512, 1024), below
one wave's width, on constant rows and on rows with a large mean; pose_head at token counts that are no multiple of the four a
workgroup holds and channel counts below / at / off the wave width, and with the per-cloud non-finite flags of pn2x_hand_frame.

Bounds: add_layernorm 2e-5 absolute and relative, pose_head 1e-5, as in test_gpu_fused.py::test_tail_kernels_match_torch (which
compares with float32 torch).  The large-mean rows are limited by the float32 rounding of the input alone; their tolerance is
4 x the error torch's own float32 layer_norm makes on the CPU for the same input (64-lane tree against a serial sum), with a
floor of 2e-5."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)
ROWS = (1, 5, 21)
FORMS = ("plain", "ln2", "y+bias+ln2", "y")
_LN = {}


def _norms(C):
    """Two LayerNorms with different eps and random affine parameters (CPU float32), built once per C."""
    if C not in _LN:
        g = torch.Generator().manual_seed(7000 + C)
        ln1, ln2 = nn.LayerNorm(C), nn.LayerNorm(C, eps=1e-6)
        assert ln1.eps == 1e-5
        with torch.no_grad():
            for ln in (ln1, ln2):
                ln.weight.copy_(torch.randn(C, generator=g))
                ln.bias.copy_(torch.randn(C, generator=g))
        _LN[C] = (ln1, ln2, nn.LayerNorm(C).cuda().requires_grad_(False), nn.LayerNorm(C, eps=1e-6).cuda().requires_grad_(False))
        for src, dst in ((ln1, _LN[C][2]), (ln2, _LN[C][3])):
            dst.load_state_dict(src.state_dict())
    return _LN[C]


def _ln64(u, ln):
    return F.layer_norm(u.double(), (u.shape[-1],), ln.weight.double(), ln.bias.double(), ln.eps)


def _reference(form, x, y, bias, ln1, ln2, dtype=torch.float64):
    """float64 (or `dtype`) layer_norm of CPU tensors, chained twice for ln2."""
    u = x.to(dtype)
    if form in ("y+bias+ln2", "y"):
        u = u + y.to(dtype)
    if form == "y+bias+ln2":
        u = u + bias.to(dtype)
    out = F.layer_norm(u, (u.shape[-1],), ln1.weight.to(dtype), ln1.bias.to(dtype), ln1.eps)
    if form in ("ln2", "y+bias+ln2"):
        out = F.layer_norm(out, (u.shape[-1],), ln2.weight.to(dtype), ln2.bias.to(dtype), ln2.eps)
    return out


def _kernel(ext, form, x, y, bias, d1, d2):
    kw = {}
    if form in ("y+bias+ln2", "y"):
        kw["y"] = y.cuda()
    if form == "y+bias+ln2":
        kw["bias"] = bias.cuda()
    if form in ("ln2", "y+bias+ln2"):
        kw["ln2"] = d2
    return ext.add_layernorm(x.cuda(), d1, **kw)


def _worst(got, ref, atol, rtol):
    got = got.cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


@pytest.mark.parametrize("C", CS)
def test_add_layernorm_matches_fp64_layer_norm(C):
    from hotrack_amd import ext
    ln1, ln2, d1, d2 = _norms(C)
    g = torch.Generator().manual_seed(C)
    worst = 0.0
    for rows in ROWS:
        x = torch.randn(rows, C, generator=g) * 3 + 1
        y, bias = torch.randn(rows, C, generator=g), torch.randn(C, generator=g)
        for form in FORMS:
            ref = _reference(form, x, y, bias, ln1, ln2)
            got = _kernel(ext, form, x, y, bias, d1, d2)
            r = _worst(got, ref, 2e-5, 2e-5)
            worst = max(worst, r)
            assert r <= 1.0, f"C={C} rows={rows} {form}: {r:.3g} times the bound atol = rtol = 2e-5"
    print(f"C={C}: worst |got - ref64| / (2e-5 + 2e-5 |ref64|) = {worst:.4f}")


@pytest.mark.parametrize("C", [100, 384])
def test_add_layernorm_constant_rows_give_the_bias(C):
    """x[r, :] = const: zero variance, the normalised row is 0 / sqrt(eps) = 0 and the output is ln.bias (chained through ln2)."""
    from hotrack_amd import ext
    ln1, ln2, d1, d2 = _norms(C)
    consts = torch.tensor([0.0, 1.0, -3.5, 1e3, 1e-3, -2.0 ** 20])
    x = consts[:, None].expand(-1, C).contiguous()
    zero = torch.zeros_like(x)
    for form in ("plain", "ln2"):
        want = ln1.bias.double().expand(len(consts), -1)
        if form == "ln2":
            want = _ln64(want, ln2)
        got = _kernel(ext, form, x, zero, None, d1, d2)
        r = _worst(got, want, 2e-5, 2e-5)
        print(f"C={C} constant rows, {form}: {r:.4f} times the bound")
        assert r <= 1.0, (form, r)
        assert _worst(got, _reference(form, x, zero, None, ln1, ln2), 2e-5, 2e-5) <= 1.0
    # x + y constant although neither is
    g = torch.Generator().manual_seed(C)
    xr = torch.randn(4, C, generator=g).mul(4).round() / 4   # multiples of 1/4: x + (c - x) is exact in float32
    got = _kernel(ext, "y", xr, 2.5 - xr, None, d1, d2)
    assert _worst(got, ln1.bias.double().expand(4, -1), 2e-5, 2e-5) <= 1.0


@pytest.mark.parametrize("form", ["plain", "ln2"])
@pytest.mark.parametrize("C", [100, 384])
def test_add_layernorm_rows_with_a_large_mean(C, form):
    """Mean 1e3, unit spread: a one-pass variance E[x^2] - E[x]^2 loses the spread to cancellation (1e6 against 1 in float32),
    the kernel's two-pass form does not.  The float32 rounding of the input alone limits the answer, so the tolerance is
    measured: 4 x the error of torch's float32 layer_norm on the CPU against the float64 reference, at least 2e-5."""
    from hotrack_amd import ext
    ln1, ln2, d1, d2 = _norms(C)
    g = torch.Generator().manual_seed(900 + C)
    x = 1e3 + torch.randn(21, C, generator=g)
    ref = _reference(form, x, None, None, ln1, ln2)
    cpu32 = _reference(form, x, None, None, ln1, ln2, torch.float32)
    cpu_err = float((cpu32.double() - ref).abs().max())
    tol = max(4 * cpu_err, 2e-5)
    got = _kernel(ext, form, x, None, None, d1, d2).cpu().double()
    err = float((got - ref).abs().max())
    print(f"C={C} {form}: kernel error {err:.3e}, torch float32 on the CPU {cpu_err:.3e}, tolerance {tol:.3e}")
    assert bool(torch.isfinite(got).all())
    assert err <= tol, f"kernel error {err:.3e} > {tol:.3e} = max(4 x {cpu_err:.3e} (torch float32 layer_norm on the CPU), 2e-5)"


def test_add_layernorm_limits():
    from hotrack_amd import ext
    from hotrack_amd.pointnet2_hip import Pn2Error
    ln = nn.LayerNorm(1025).cuda()
    with pytest.raises(Pn2Error):
        ext.add_layernorm(torch.randn(3, 1025, device="cuda"), ln)
    _, _, d1, d2 = _norms(64)
    out = ext.add_layernorm(torch.empty(0, 64, device="cuda"), d1, ln2=d2)
    assert out.shape == (0, 64) and out.dtype == torch.float32
    x = torch.randn(5, 64, device="cuda")     # nothing pending: a valid call afterwards
    assert _worst(ext.add_layernorm(x, d1), _ln64(x.cpu(), _norms(64)[0]), 2e-5, 2e-5) <= 1.0


POSE_SHAPES = [(1, 21, 256), (3, 5, 70), (7, 21, 33), (2, 1, 64), (65, 21, 256)]


def _pose_inputs(B, J, C):
    g = torch.Generator().manual_seed(B * 100 + J + C)
    h = torch.randn(B * J, C, generator=g)
    w = torch.randn(3, C, generator=g) * 0.1
    bias = torch.randn(3, generator=g)
    xyz1 = torch.randn(B, J, 3, generator=g)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0].contiguous()
    t = torch.randn(B, 3, 1, generator=g)
    return h, w, bias, xyz1, R, t


@pytest.mark.parametrize("B,J,C", POSE_SHAPES)
def test_pose_head_matches_fp64(B, J, C):
    from hotrack_amd import ext
    h, w, bias, xyz1, R, t = _pose_inputs(B, J, C)
    scale = 0.2
    s = float(torch.tensor(scale, dtype=torch.float32))
    ref_h = (h.double() @ w.double().t() + bias.double()).view(B, J, 3) + xyz1.double()
    ref_c = ref_h @ R.double().transpose(1, 2) * s + t.double().transpose(1, 2)
    dev = [x.cuda() for x in (h, w, bias, xyz1, R, t)]
    kh, kc = ext.pose_head(*dev, scale)
    assert kh.shape == (B, J, 3) == kc.shape
    rh, rc = _worst(kh, ref_h, 1e-5, 1e-5), _worst(kc, ref_c, 1e-5, 1e-5)
    print(f"B={B} J={J} C={C}: kp_hand {rh:.4f}, kp_cam {rc:.4f} times the bound atol = rtol = 1e-5")
    assert rh <= 1.0 and rc <= 1.0
    # flagged clouds come out all-NaN in both frames, every other cloud bit-equal to the unflagged run
    flags = torch.zeros(B, dtype=torch.int32)
    flags[1::2] = 1
    if B == 1:
        flags[0] = 1
    fh, fc = ext.pose_head(*dev, scale, nonfinite=flags.cuda())
    bad, good = flags.bool().cuda(), ~flags.bool().cuda()
    assert int(bad.sum()) >= 1
    assert bool(torch.isnan(fh[bad]).all()) and bool(torch.isnan(fc[bad]).all())
    assert torch.equal(fh[good], kh[good]) and torch.equal(fc[good], kc[good])
    zh, zc = ext.pose_head(*dev, scale, nonfinite=torch.zeros(B, dtype=torch.int32, device="cuda"))
    assert torch.equal(zh, kh) and torch.equal(zc, kc)
