"""CPU: the references and builders of tests/_stack_layer_cases.py, before tests/test_gpu_stack_layers_fp64.py rests on them.  Both
references are anchored to torch autograd in float64 -- a two-layer Linear + BatchNorm1d(train) + ReLU composition, with and without
a max over K rows -- to 1e-12 of each quantity's scale, and the builders are shown to produce what they claim: masks MASK_MARGIN
clear of zero with at most 1 % of the entries moved, statistics consistent with the data, complete sums, groups that straddle
tiles, a dead channel that is dead and a masked group."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stack_layer_cases as L  # noqa: E402

f64 = torch.float64


def _close(name, got, want, rel=1e-12):
    got, want = got.detach().to(f64), want.detach().to(f64)
    scale = float(want.abs().max()) + 1e-300
    err = float((got - want).abs().max())
    assert err <= rel * scale, (name, err, scale)


@pytest.mark.parametrize("K", [0, 1, 8])
@pytest.mark.parametrize("R,k,n", [(48, 6, 10), (200, 32, 64)])
def test_references_are_torch_autograd_in_float64(R, k, n, K):
    """K = 0: the layer-i output itself is the stack's output (gmode 1, and gmode 0 from the masked gradient); K > 0: a max over K
    consecutive rows on top (gmode 2 with torch's own arg-max)."""
    gen = torch.Generator().manual_seed(R + k + n + K)
    lin_p = torch.nn.Linear(7, k).double()
    lin_i = torch.nn.Linear(k, n).double()
    bn_p = torch.nn.BatchNorm1d(k, momentum=0.07).double().train()
    bn_i = torch.nn.BatchNorm1d(n, momentum=0.07).double().train()
    with torch.no_grad():
        for bn in (bn_p, bn_i):
            bn.weight.copy_(1 + 0.3 * torch.randn(bn.num_features, generator=gen, dtype=f64))
            bn.bias.copy_(0.2 * torch.randn(bn.num_features, generator=gen, dtype=f64))
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=gen, dtype=f64))
            bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=gen, dtype=f64))
    rm0, rv0 = bn_p.running_mean.clone(), bn_p.running_var.clone()
    x0 = torch.randn(R, 7, generator=gen, dtype=f64)
    z_p = lin_p(x0)                  # layer p's pre-activation WITH its bias; the fused layers carry it without
    pre_p = bn_p(z_p)
    pre_p.retain_grad()
    y_i = lin_i(torch.relu(pre_p))   # lin_i's bias cancels in bn_i
    y_i.retain_grad()
    pre_i = bn_i(y_i)
    h_i = torch.relu(pre_i)
    if K:
        out, arg = h_i.view(R // K, K, n).max(dim=1)
    else:
        out, arg = h_i, None
    go = torch.randn(out.shape, generator=gen, dtype=f64)
    (out * go).sum().backward()

    x = (z_p - lin_p.bias).detach()
    sums_in = torch.cat([x.sum(0), (x * x).sum(0)])
    fwd = L.layer_forward_reference(x, lin_i.weight.detach(), sums_in, bn_p.weight.detach(), bn_p.bias.detach(), lin_p.bias.detach(), bn_p.eps,
                                    0.07, rm0, rv0)
    yi_nobias = (y_i - lin_i.bias).detach()
    _close("y", fwd["y"], yi_nobias)
    _close("running_mean", fwd["running_mean"], bn_p.running_mean)
    _close("running_var", fwd["running_var"], bn_p.running_var)
    assert fwd["num_batches_tracked"] == int(bn_p.num_batches_tracked) == 1
    _close("sums_out", fwd["sums_out"], torch.cat([yi_nobias.sum(0), (yi_nobias * yi_nobias).sum(0)]))
    _close("mean", fwd["mean"], x.mean(0))
    _close("invstd", fwd["invstd"], 1.0 / torch.sqrt(x.var(0, unbiased=False) + bn_p.eps))

    yi = y_i.detach()
    mean_i, invstd_i = yi.mean(0), 1.0 / torch.sqrt(yi.var(0, unbiased=False) + bn_i.eps)
    zp = z_p.detach()
    mean_p, invstd_p = zp.mean(0), 1.0 / torch.sqrt(zp.var(0, unbiased=False) + bn_p.eps)
    sources = [(2, go, arg.int(), K)] if K else [(1, go, None, 1), (0, go * (pre_i.detach() > 0), None, 1)]
    for gmode, gsrc, a, kmax in sources:
        ref = L.layer_backward_reference(gmode, gsrc, a, kmax, yi, mean_i, invstd_i, bn_i.weight.detach(), bn_i.bias.detach(),
                                         lin_i.weight.detach(), zp, mean_p, invstd_p, bn_p.weight.detach(), bn_p.bias.detach())
        _close(f"dY gmode {gmode}", ref["dy"], y_i.grad)
        _close(f"g_p gmode {gmode}", ref["gp"], pre_p.grad)
        _close(f"dW gmode {gmode}", ref["dw"], lin_i.weight.grad)
        _close(f"dgamma gmode {gmode}", ref["dgamma"], bn_i.weight.grad)
        _close(f"dbeta gmode {gmode}", ref["dbeta"], bn_i.bias.grad)
        # the sums of layer p are its BatchNorm's parameter gradients
        _close(f"sums_bwd_p gmode {gmode}", ref["sums_bwd_p"], torch.cat([bn_p.bias.grad, bn_p.weight.grad]))
        assert float(lin_i.bias.grad.abs().max()) <= 1e-12 * float(go.abs().sum())   # dbias: analytically zero


def test_reference_takes_given_sums():
    """sums_bwd_i is an input: other sums give another dY (the kernels are handed the sums, they do not form them)."""
    c = L.backward_case(70, 32, 32, 1, seed=3)
    a = c["ref"]
    args = (1, c["gsrc"], None, 1, c["yi"], c["mean_i"], c["invstd_i"], c["gamma_i"], c["beta_i"], c["w"], c["yp"], c["mean_p"], c["invstd_p"],
            c["gamma_p"], c["beta_p"])
    b = L.layer_backward_reference(*args, sums_bwd_i=a["own_sums"])
    assert torch.equal(a["dy"], b["dy"])
    b = L.layer_backward_reference(*args, sums_bwd_i=torch.zeros(64, dtype=f64))
    assert not torch.allclose(a["dy"], b["dy"])


SPECS = sorted(set(s[1:] for s in L.backward_specs()))


def test_margin_is_derived():
    assert L.MASK_MARGIN == 4 * 2.0 ** -24 * (L.GAMMA_MAX * L.XHAT_MAX + L.BETA_MAX)
    assert 1e-6 < L.MASK_MARGIN < 1e-5 and L.MOVE_TO > 2 * L.MASK_MARGIN


@pytest.mark.parametrize("rows,k,n,gmode,kmax", SPECS)
def test_backward_cases_keep_their_claims(rows, k, n, gmode, kmax):
    c = L.cached_backward_case(rows, k, n, gmode, kmax)
    ref = c["ref"]
    for y, m, s, ga, be, pre, xh, moved in ((c["yi"], c["mean_i"], c["invstd_i"], c["gamma_i"], c["beta_i"], ref["pre_i"], ref["xhat_i"], c["moved"][0]),
                                            (c["yp"], c["mean_p"], c["invstd_p"], c["gamma_p"], c["beta_p"], ref["pre_p"], ref["xhat_p"], c["moved"][1])):
        assert y.dtype == torch.float32 and m.dtype == torch.float32 and s.dtype == torch.float32
        assert float(pre.abs().min()) >= L.MASK_MARGIN                      # no mask entry closer to zero than the margin
        assert moved <= 0.01 * y.numel()                                    # ... and at most 1 % of the entries had to be moved
        assert float(xh.abs().max()) <= L.XHAT_MAX and float(ga.abs().max()) <= L.GAMMA_MAX and float(be.abs().max()) <= L.BETA_MAX
        # the float32 statistics are those of the (final) data, to a float32 rounding of mean and spread
        y64 = y.double()
        mean = y64.mean(0)
        std = (y64 - mean).pow(2).mean(0).sqrt()
        assert bool(((m.double() - mean).abs() <= 2 * L.U * (mean.abs() + std) + 1e-30).all())
        inv = 1.0 / torch.sqrt(std * std + L.EPS)
        assert bool(((s.double() - inv).abs() <= 4 * L.U * inv).all())
    # the sums handed to the kernel are the complete sums of the reference's own g
    total = c["sums_parts"].sum(0)
    assert bool(((total - ref["own_sums"]).abs() <= 1e-13 * (ref["g"].abs().sum() + 1)).all())
    assert torch.equal(ref["dgamma"], ref["own_sums"][n:]) and torch.equal(ref["dbeta"], ref["own_sums"][:n])
    # the dead channel of layer p is dead: no gradient passes, its column of dW is exactly zero
    assert not bool(ref["mask_p"][:, L.DEAD].any())
    assert float(ref["gp"][:, L.DEAD].abs().max()) == 0.0 and float(ref["dw"][:, L.DEAD].abs().max()) == 0.0
    assert bool(ref["mask_p"][:, [c_ for c_ in range(k) if c_ != L.DEAD]].any()) or rows == 1
    if gmode == 2:
        assert c["arg"].dtype == torch.int32 and int(c["arg"].min()) >= 0 and int(c["arg"].max()) < kmax
        assert c["gsrc"].shape == (rows // kmax, n) and rows % kmax == 0
        nz = (L.route(torch.ones_like(c["gsrc"]), c["arg"], kmax) != 0)
        assert bool((nz.view(rows // kmax, kmax, n).sum(1) == 1).all())      # one row per (group, channel)
        assert not bool(ref["g"][~nz].any())                               # rows no arg selects: exactly zero
    if c["negative"]:
        assert not bool((ref["pre_i"][:c["negative"], 0::2] > 0).any())     # the masked group
        assert not bool(ref["g"][:c["negative"], 0::2].any())
        assert bool((ref["pre_i"][:c["negative"], 1::2] > 0).any())
    if gmode != 0:
        assert 0.1 < float((ref["pre_i"] > 0).double().mean()) < 0.9


def test_case_lists_reach_what_they_say():
    assert L.straddling_groups(240, 24) == 2 and L.straddling_groups(195, 3) == 2 and L.straddling_groups(197, 197) == 1
    assert L.straddling_groups(208, 16) == 0 and L.straddling_groups(64, 16) == 0
    for name, (rows, gmode, kmax, opt) in L.BWD_REDUCED.items():
        if gmode == 2:
            assert rows % kmax == 0, name
    assert any(L.cached_backward_case(r, k, n, g, km)["negative"] for (r, k, n, g, km) in SPECS if g == 2)
    assert sorted({s[1] for s in L.backward_specs() if s[0].startswith("bwd_slice") and s[2:4] == L.BWD_LARGEST}) >= [1, 63, 64, 65]
    assert set(L.BWD2_SHAPES) <= set(L.BWD_SHAPES) and L.BWD_LARGEST == max(L.BWD_SHAPES, key=lambda s: s[0] * s[1])
    assert sorted({(r, k, n) for r, k, n, _ in L.FWD_CASES} & {(r, k, n) for r in L.FWD_ROWS for k in L.FWD_K for n in L.FWD_N}) == \
        sorted({(r, k, n) for r, k, n, _ in L.FWD_CASES})
    assert {r for r, _, _, _ in L.FWD_CASES} == set(L.FWD_ROWS) and {k for _, k, _, _ in L.FWD_CASES} == set(L.FWD_K)
    assert {n for _, _, n, _ in L.FWD_CASES} == set(L.FWD_N)


@pytest.mark.parametrize("rows,k,n", [(1, 32, 32), (129, 96, 64)])
def test_forward_case_sums_and_dead_channel(rows, k, n):
    c = L.forward_case(rows, k, n, seed=rows + k)
    x = c["x"].double()
    assert torch.equal(c["sums_in"], torch.cat([x.sum(0), (x * x).sum(0)]))
    assert float(c["ref"]["h"][:, L.DEAD].abs().max()) == 0.0
    assert c["ref"]["num_batches_tracked"] == 1
    if rows == 1:
        assert float(c["ref"]["var"].abs().max()) == 0.0
