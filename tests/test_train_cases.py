"""CPU: the references and builders of tests/_train_cases.py, before tests/test_gpu_train_fp64.py rests on them.  The builders are
shown to produce what they claim (realised |mean| / std per channel, ties on the lattice, padded neighbour lists), the float64
BatchNorm reference is anchored to torch.nn.BatchNorm1d in float64 (forward, running statistics, every gradient), the other
references to torch's own autograd or optimiser in float64, and the comparison is shown to fail for a variance that is off by
the amount the fp32 sum-of-squares form loses at |mean| / std = 100."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _train_cases as T  # noqa: E402

f64 = torch.float64


@pytest.mark.parametrize("R", [257, 1000])
def test_plans_realise_their_ratio(R):
    plan, groups = T.ladder_plan(64)
    y = T.plan_inputs(R, plan, seed=R)
    assert y.dtype == torch.float32 and y.shape == (R, 64)
    got = T.realised_ratio(y)
    for c, (m, s) in enumerate(plan):
        want = abs(m) / s
        if want == 0:
            assert float(got[c]) < 1e-6          # exactly centred up to the float32 rounding of the samples
        else:
            assert abs(float(got[c]) - want) <= 0.1 * want, (c, float(got[c]), want)
    assert sorted(c for cs in groups.values() for c in cs) == list(range(64))


@pytest.mark.parametrize("K", [3, 24, 64])
def test_lattice_inputs_tie(K):
    y = T.lattice_inputs(40 * K, 16, seed=K)
    assert T.tie_share(y, K) > 0
    smooth = torch.randn(40 * K, 16, generator=torch.Generator().manual_seed(1))
    assert T.tie_share(smooth, K) == 0


def test_ball_padding_repeats_the_first_index():
    idx = T.ball_padded_idx(3, 11, 32, 200, seed=2)
    assert idx.dtype == torch.int32 and idx.shape == (3, 11, 32)
    padded = (idx == idx[:, :, :1]).sum(-1)
    assert int(padded.max()) == 32 and int(padded.min()) < 32   # a ball with one hit, and balls with many
    assert int(idx.min()) >= 0 and int(idx.max()) < 200


MILD = ((0.0, 1.0), (0.25, 1.0), (-1.0, 2.0), (0.5, 0.1))  # |mean| / std <= 5: float64 torch is itself good to 1e-14 here


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("R,C,ladder", [(7, 4, False), (257, 12, False), (1000, 64, False), (1000, 64, True)])
def test_bn_reference_is_torch_batchnorm_in_float64(R, C, relu, ladder):
    """THE ANCHOR is the three ladder=False rows: equal to 1e-12 of each quantity's scale on channels with |mean| / std <= 5, where
    float64 torch is itself good to 1e-14.
    The ladder=True row is NOT an anchor and proves little about the reference: its bound is 1e-12 x (|mean| / std)^2 per channel
    (1e-6 at ratio 1000), because torch's float64 kernel loses (|mean| / std)^2 x 1e-16 of the variance to its own accumulation
    while the reference is two-pass and does not (measured distance at ratio 1000: 1.2e-10 on dgamma of 50).  It only shows that
    nothing in the reference goes wrong by more than torch's own float64 cancellation on the inputs the GPU ladder uses."""
    plan = T.ladder_plan(C)[0] if ladder else [MILD[c % len(MILD)] for c in range(C)]
    y = T.plan_inputs(R, plan, seed=R + C).double()
    g = torch.Generator().manual_seed(3)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g, dtype=f64), 0.2 * torch.randn(C, generator=g, dtype=f64)
    bias = torch.randn(C, generator=g, dtype=f64)
    go = torch.randn(R, C, generator=g, dtype=f64)
    bn = torch.nn.BatchNorm1d(C, momentum=0.05).double().train()
    rm0, rv0 = torch.randn(C, generator=g, dtype=f64), 0.5 + torch.rand(C, generator=g, dtype=f64)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    yt = y.clone().requires_grad_(True)
    h = bn(yt + bias)
    h = torch.relu(h) if relu else h
    h.backward(go)
    # torch sees y + bias rounded to float64: the reference takes the same sum for outputs and gradients, and y with conv_bias=
    # (the kernels' form: the bias only shifts the running mean) for the running statistics
    ref = T.bn_reference(y + bias, gamma, beta, bn.eps, go=go, relu=relu)
    run = T.bn_reference(y, gamma, beta, bn.eps, relu=relu, conv_bias=bias, running_mean=rm0, running_var=rv0, momentum=0.05)
    tol = 1e-12 * torch.clamp(T.realised_ratio(y + bias), min=1.0) ** 2 if ladder else torch.full((C,), 1e-12, dtype=f64)

    def close(a, b):
        return bool(((a - b).abs() <= tol * max(1.0, float(b.abs().max()))).all())

    assert close(ref["out"], h.detach())
    assert close(run["running_mean"], bn.running_mean) and close(run["running_var"], bn.running_var)
    assert close(ref["dy"], yt.grad) and close(ref["dgamma"], bn.weight.grad) and close(ref["dbeta"], bn.bias.grad)


@pytest.mark.parametrize("K", [1, 3, 24])
def test_bn_max_reference_takes_the_first_row(K):
    G, C = 30, 8
    y = T.lattice_inputs(G * K, C, seed=K + 10).double()
    g = torch.Generator().manual_seed(4)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g, dtype=f64), 0.2 * torch.randn(C, generator=g, dtype=f64)
    go = torch.randn(G, C, generator=g, dtype=f64)
    ref = T.bn_reference(y, gamma, beta, 1e-5, go=go, K=K)
    h = T.bn_reference(y, gamma, beta, 1e-5)["out"].view(G, K, C)   # relu(BatchNorm(y)), row by row
    for grp in range(G):
        for c in range(C):
            col = h[grp, :, c]
            pcol = ref["pre"].view(G, K, C)[grp, :, c]
            first = min(k for k in range(K) if pcol[k] == pcol.max())
            assert int(ref["arg"][grp, c]) == first and ref["out"][grp, c] == col.max()
    # the gradient through torch's own autograd (amax splits ties evenly, so route by the reference's arg-max instead)
    yt = y.clone().requires_grad_(True)
    d = yt - yt.mean(0)
    pre = d / torch.sqrt((d * d).mean(0) + 1e-5) * gamma + beta
    out = torch.gather(torch.relu(pre).view(G, K, C), 1, ref["arg"].unsqueeze(1)).squeeze(1)
    out.backward(go)
    assert float((ref["dy"] - yt.grad).abs().max()) <= 1e-12 * max(1.0, float(yt.grad.abs().max()))
    dead = ref["out"] <= 0               # groups whose maximum is <= 0: no gradient reaches any of their rows
    if bool(dead.any()):
        g0 = T.bn_reference(y, gamma, beta, 1e-5, go=go * dead, K=K)
        assert float(g0["dgamma"].abs().max()) == 0.0 and float(g0["dy"].abs().max()) == 0.0


def test_sa_layer1_reference_against_autograd():
    B, N, S, K, C1 = 2, 40, 7, 5, 8
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    xyz, cxyz, a1f, cadd, wx = r(B, N, 3), r(B, S, 3), r(B, N, C1).requires_grad_(True), r(B, S, C1).requires_grad_(True), r(C1, 3).requires_grad_(True)
    idx = T.ball_padded_idx(B, S, K, N, seed=6)
    go = r(B, S * K, C1)
    out = torch.empty(B, S * K, C1, dtype=f64)
    rows = []
    for b in range(B):           # the definition, one slot at a time
        for s in range(S):
            for k in range(K):
                j = int(idx[b, s, k])
                rows.append(a1f[b, j] + wx @ (xyz[b, j] - cxyz[b, s]) + cadd[b, s])
    out = torch.stack(rows).view(B, S * K, C1)
    out.backward(go)
    ref = T.sa_layer1_reference(a1f.detach(), cadd.detach(), xyz, cxyz, idx, wx.detach(), go=go)
    for a, b in ((ref["out"], out.detach()), (ref["d_a1f"], a1f.grad), (ref["d_cadd"], cadd.grad), (ref["d_wx"], wx.grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_row_transposes_against_autograd():
    B, M, n, C = 2, 9, 30, 4
    g = torch.Generator().manual_seed(7)
    pts = torch.randn(B, M, C, generator=g, dtype=f64).requires_grad_(True)
    idx = torch.randint(0, M - 1, (B, n, 3), generator=g, dtype=torch.int32)     # row M - 1 is never named
    idx[:, 0, 1] = idx[:, 0, 0]                                                  # a triple that names one source twice
    w = torch.rand(B, n, 3, generator=g, dtype=f64)
    w[:, 1, 2] = 0.0
    go = torch.randn(B, n, C, generator=g, dtype=f64)
    out = sum(torch.gather(pts, 1, idx[:, :, t].long().unsqueeze(-1).expand(-1, -1, C)) * w[:, :, t:t + 1] for t in range(3))
    out.backward(go)
    assert torch.allclose(T.interpolate_reference(pts.detach(), idx, w), out.detach(), rtol=0, atol=1e-13)
    back = T.interpolate_backward(go, idx, w, M)
    assert torch.allclose(back, pts.grad, rtol=0, atol=1e-13) and float(back[:, M - 1].abs().max()) == 0.0
    init = torch.randn(B, M, C, generator=g, dtype=f64)
    flat = idx.reshape(B, -1)[:, :n]
    assert torch.allclose(T.segment_sum_reference(go, flat, M, init=init), init + T.gather_backward(go, flat, M), rtol=0, atol=1e-13)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step0", [0, 9999])
def test_adam_reference_is_torch_adam_in_float64(wd, step0):
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(33, generator=g, dtype=f64)
    gr = torch.randn(33, generator=g, dtype=f64)
    gr[:5] = 0.0
    m0, v0 = 0.1 * torch.randn(33, generator=g, dtype=f64), 0.01 * torch.rand(33, generator=g, dtype=f64)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = gr.clone()
    opt.step()
    want, m, v = T.adam_reference(p0, gr, m0, v0, step0 + 1, 1e-3, 0.9, 0.999, 1e-8, wd)
    assert float((want - p.detach()).abs().max()) <= 1e-14
    assert torch.allclose(m, opt.state[p]["exp_avg"], rtol=1e-14, atol=0) and torch.allclose(v, opt.state[p]["exp_avg_sq"], rtol=1e-14, atol=1e-300)


def test_the_bound_sees_the_cancellation_it_is_there_for():
    """A variance that is off by 1e-4 (what fp32 sums of y and y^2 lose at |mean| / std = 100) moves a BatchNorm output of 3 by
    1.5e-4: 5 x outside rtol 1e-5 / atol 2e-5, and outside 4 x the distance of a float32 two-pass evaluation."""
    y = T.plan_inputs(1000, [(100.0, 1.0)] * 4, seed=9)
    one, zero = torch.ones(4, dtype=f64), torch.zeros(4, dtype=f64)
    ref = T.bn_reference(y, one, zero, 1e-5, relu=False)
    wrong = (y.double() - ref["mean"]) / torch.sqrt(ref["var"] * (1 + 1e-4) + 1e-5)
    y32 = y - y.mean(0)
    fp32 = y32 / torch.sqrt((y32 * y32).mean(0) + 1e-5)
    e_torch = T.dist(fp32, ref["out"], 1e-5, 2e-5)
    assert T.dist(wrong, ref["out"], 1e-5, 2e-5) > T.bound(e_torch)
    assert T.dist(ref["out"], ref["out"], 1e-5, 2e-5) == 0.0
    nan = ref["out"].clone()
    nan[0, 0] = float("nan")
    assert T.dist(nan, ref["out"], 1e-5, 2e-5) == float("inf")
