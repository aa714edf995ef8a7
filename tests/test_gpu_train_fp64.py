"""GPU: the training operators (csrc/train_ops.hip, adam.hip, tail_train.hip's LayerNorm, the fused stacks' statistics) against the
float64 references of tests/_train_cases.py at the shapes and inputs where they can go wrong.

The tolerance rule, everywhere: distance from float64 <= max(F, 4 x E_torch), where F is the tolerance the operator's existing
test in test_gpu_train.py uses and E_torch the distance of the fp32 torch composition of the same operation from the same float64
reference on the same inputs, measured in the test.  Distances are printed in units of F (<= 1: inside F) as
`case quantity [channel group]: kernel <d> torch <d>`; no bound is derived from a kernel's own output."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _train_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
DEV = "cuda"


def _measure(case, name, got, want, torch_got, rtol, atol, cols=None, what=""):
    """got / torch_got vs want (float64) in units of (atol + rtol |want|) (atol: a number, or a tensor shaped like want); prints both
    distances and returns (kernel distance, torch distance, bound)."""
    if cols is not None:
        got, want, torch_got = got[..., cols], want[..., cols], torch_got[..., cols]
    dk, dt = T.dist(got, want, rtol, atol), T.dist(torch_got, want, rtol, atol)
    print(f"{case} {name}{' [' + what + ']' if what else ''}: kernel {dk:.3g} torch {dt:.3g} bound {T.bound(dt):.3g}")
    return dk, dt, T.bound(dt)


def _check(case, name, got, want, torch_got, rtol, atol, cols=None, what=""):
    """_measure(), and asserts the rule."""
    dk, dt, bound = _measure(case, name, got, want, torch_got, rtol, atol, cols, what)
    assert dk <= bound, (case, name, what, dk, dt)
    return dk, dt


def _bn_modules(C, seed, momentum=0.05):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    bns = []
    for _ in range(2):
        bn = torch.nn.BatchNorm1d(C, momentum=momentum).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
        bns.append(bn)
    return bns[0], bns[1], gamma, beta, rm, rv


def _run_bn(case, y0, relu=True, K=0, groups=None, wide=0, gamma_beta=None, go_scale=None, dy_rows=None):
    """bn_relu / bn_relu_max on y0 (CPU float32 (R, C)) vs float64, beside torch.nn.BatchNorm1d (+ relu, + max) in float32: output,
    saved mean / invstd, running statistics, dY, dgamma, dbeta -- per channel group when `groups` is given.  wide: y is read as
    columns [4, 4 + C) of a (R, C + wide) buffer.  dy_rows (with K and groups): reference -> (R, C) bool, the elements of dY to
    compare.  Returns (kernel results, reference)."""
    from hotrack_amd.train_ops import Workspace, bn_relu, bn_relu_max
    R, C = y0.shape
    bn_a, bn_b, gamma, beta, rm, rv = _bn_modules(C, seed=C + R)
    if gamma_beta is not None:
        gamma, beta = gamma_beta
        with torch.no_grad():
            for bn in (bn_a, bn_b):
                bn.weight.copy_(gamma)
                bn.bias.copy_(beta)
    g = torch.Generator().manual_seed(R * 7 + C)
    go = torch.randn(R // K if K else R, C, generator=g)
    if go_scale is not None:
        go = go * go_scale
    bias = torch.randn(C, generator=g)
    ref = T.bn_reference(y0, gamma, beta, bn_a.eps, go=go, relu=relu, K=K, conv_bias=bias, running_mean=rm, running_var=rv, momentum=0.05)
    # the kernel
    if wide:
        buf = torch.full((R, C + wide), float("nan"), device=DEV)
        buf[:, 4:4 + C] = y0.to(DEV)
        leaf = buf.requires_grad_(True)
        ya = leaf[:, 4:4 + C]
    else:
        leaf = y0.to(DEV).requires_grad_(True)
        ya = leaf
    ws = Workspace(DEV)
    ba = bias.to(DEV).requires_grad_(True)
    ha = bn_relu_max(ya, K, bn_a, ws, ba) if K else bn_relu(ya, bn_a, ws, ba, relu=relu)
    saved = ha.grad_fn.saved_tensors[3].clone()     # (y, gamma, beta, saved mean | invstd[, arg-max])
    assert saved.shape == (2, C)
    arg = [ha.grad_fn.saved_tensors[4]] if K else []
    ha.backward(go.to(DEV))
    dya = leaf.grad[:, 4:4 + C] if wide else leaf.grad
    assert float(ba.grad.abs().max()) == 0.0  # a bias in front of BatchNorm: analytically zero
    # fp32 torch
    yb = y0.to(DEV).requires_grad_(True)
    hb = bn_b(yb + bias.to(DEV))
    hb = torch.relu(hb) if (relu or K) else hb
    if K:
        hb = hb.view(R // K, K, C).max(dim=1)[0]
    hb.backward(go.to(DEV))
    with torch.no_grad():
        y32 = y0.to(DEV)
        tmean = y32.mean(0)
        tinv = 1.0 / torch.sqrt(y32.var(0, unbiased=False) + bn_b.eps)
    gs = float(ref["dy"][torch.isfinite(ref["dy"])].abs().max())
    for what, cols in (groups or {"": None}).items():
        chk = lambda n, a, w, t, rt, at: _check(case, n, a, w, t, rt, at, cols, what)
        chk("out", ha.detach(), ref["out"], hb.detach(), 1e-5, 2e-5)
        chk("save_mean", saved[0], ref["mean"], tmean, 1e-5, 1e-6)
        chk("save_invstd", saved[1], ref["invstd"], tinv, 1e-5, 1e-6)
        chk("running_mean", bn_a.running_mean, ref["running_mean"], bn_b.running_mean, 1e-5, 1e-6)
        chk("running_var", bn_a.running_var, ref["running_var"], bn_b.running_var, 1e-5, 1e-6)
        if K == 0 or not groups:  # (with the max, dY per element only where the caller rules out near-ties: one other row = O(go))
            chk("dY", dya, ref["dy"], yb.grad, 1e-4, 2e-5 * max(gs, 1.0))
        elif dy_rows is not None:  # ... or on the rows of the (group, channel) pairs whose routing the caller calls decidable
            m = dy_rows(ref)[:, cols]
            assert float(m.double().mean()) > 0.5, (case, what)
            pick = lambda t: t.detach().cpu()[:, cols][m]
            _check(case, "dY (decidable rows)", pick(dya), pick(ref["dy"]), pick(yb.grad), 1e-4, 2e-5 * max(gs, 1.0), None, what)
        c = slice(None) if cols is None else cols
        chk("dgamma", bn_a.weight.grad, ref["dgamma"], bn_b.weight.grad, 1e-4, 1e-4 * float(ref["dgamma"][c].abs().max()) + 1e-30)
        chk("dbeta", bn_a.bias.grad, ref["dbeta"], bn_b.bias.grad, 1e-4, 1e-4 * float(ref["dbeta"][c].abs().max()) + 1e-30)
    assert int(bn_a.num_batches_tracked) == 1
    return {"out": ha.detach(), "dy": dya, "saved": saved, "arg": arg[0] if arg else None, "bn": bn_a, "go": go}, ref


# ---- bn_relu ------------------------------------------------------------------------------------------------------------------------
# rows_per_block_for(): rpp = 256 / (C / 4) rows per pass; at these sizes a workgroup owns 16 x rpp rows in the statistics pass and
# 4 x rpp in the apply / backward passes (R / 512 and R / 1024 are smaller):
#        C =    4     12     64    192    512
#   statistics  4096  1360   256    80     32   rows per workgroup
#   apply, bwd  1024   340    64    20      8
#   R = 2, 7      fewer rows than one pass of one workgroup (threads without a row; R = 2 < the 4-row unroll)
#   R = 255, 257  4-row unroll remainders; at C = 64 the two sides of the statistics pass's 256-row share (one workgroup / two,
#                 the second with one row), 4 - 5 apply workgroups; one workgroup in every pass at C = 4, 12; many at C = 192, 512
#   R = 1000      C = 4: still ONE workgroup in every pass (1000 < 1024); C = 12: one in the statistics pass, three in apply / bwd;
#                 C = 192, 512 (and the ladder's (1000, 64)): several in every pass, fewer than the 512 / 1024-workgroup grid
#   C = 12, 192   quads (3, 48) that do not divide 256: idle threads in every workgroup;  C = 512: rpp = 2
BN_SHAPES = [(2, 4), (2, 512), (7, 12), (7, 192), (255, 4), (255, 64), (257, 12), (257, 64), (257, 192), (257, 512), (1000, 4), (1000, 12),
             (1000, 192), (1000, 512)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("R,C", BN_SHAPES)
def test_bn_relu_shapes(R, C, relu):
    plan = [((-1.0) ** c * 0.5 * (c % 3), 0.5 + (c % 4)) for c in range(C)]
    _run_bn(f"bn_relu R={R} C={C} relu={relu}", T.plan_inputs(R, plan, seed=R + C), relu=relu)


def test_bn_relu_reads_a_column_block():
    _run_bn("bn_relu ld>C", T.plan_inputs(257, [(0.3, 1.5)] * 64, seed=1), wide=12)


@pytest.mark.parametrize("relu", [True, False])
def test_bn_relu_conditioning_ladder(relu):
    """std 1 with mean 0 / 10 / 100 / 1000 and one channel (0.5, 1e-3): with fp32 sums of y and y^2 the variance of the ratio-100
    channels was off by ~1e-4 and that of the ratio-1000 channels by percents."""
    plan, groups = T.ladder_plan(64)
    _run_bn(f"bn_relu ladder relu={relu}", T.plan_inputs(1000, plan, seed=64), relu=relu, groups=groups)


def test_bn_relu_constant_channel():
    R, C = 1000, 8
    y = T.plan_inputs(R, [(0.3, 1.0)] * C, seed=2)
    y[:, 1], y[:, 6] = 3.0, -0.7123
    res, ref = _run_bn("bn_relu constant", y, relu=False, groups={"const": [1, 6], "rest": [0, 2, 3, 4, 5, 7]})
    bn = res["bn"]
    assert torch.equal(res["out"][:, [1, 6]], bn.bias.detach()[[1, 6]].expand(R, 2))   # (y - mean) is exactly 0
    assert float(ref["var"][1]) == 0.0 and float(ref["var"][6]) == 0.0
    assert bool(torch.isfinite(res["dy"]).all())
    # running_var moves by momentum x 0: (1 - momentum) x the old value, to fp32 round-off
    _, _, _, _, _, rv = _bn_modules(C, seed=C + R)
    want = (0.95 * rv.double())[[1, 6]]
    assert T.dist(bn.running_var[[1, 6]], want, 1e-5, 1e-6) <= 1.0, (bn.running_var[[1, 6]], want)


def test_bn_relu_dead_channel_and_nan():
    R, C = 257, 12
    y = T.plan_inputs(R, [(0.3, 1.0)] * C, seed=3)
    g = torch.Generator().manual_seed(4)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    gamma[5], beta[5] = 0.01, -5.0     # BatchNorm output in [-5.1, -4.9]: negative everywhere
    res, ref = _run_bn("bn_relu dead", y, gamma_beta=(gamma, beta))
    assert float(res["out"][:, 5].abs().max()) == 0.0 and float(res["dy"][:, 5].abs().max()) == 0.0
    assert float(res["bn"].weight.grad[5]) == 0.0 and float(res["bn"].bias.grad[5]) == 0.0
    # one NaN in channel 7: that channel is NaN, every other channel keeps its bound
    y[100, 7] = float("nan")
    keep = [c for c in range(C) if c != 7]
    res, ref = _run_bn("bn_relu nan", y, gamma_beta=(gamma, beta), groups={"others": keep})
    assert bool(torch.isnan(res["out"][:, 7]).all()) and bool(torch.isfinite(res["out"][:, keep]).all())


# ---- bn_relu_max --------------------------------------------------------------------------------------------------------------------
# pn2x_bn_relu_max splits a group's rows over lanes when K >= 4 and groups x C / 4 < 65536 (split >= 4), else one thread per
# (group, quad): at C = 64 the switch is at 4096 groups.  K = 1, 3: always the serial kernel.
@pytest.mark.parametrize("G,K,C", [(300, 1, 64), (50, 3, 12),      # serial (K < 4)
                                   (300, 24, 64), (40, 64, 192),   # split kernel (few groups)
                                   (4100, 24, 64)])                # serial: past the switch at 4096 groups
def test_bn_relu_max_matches_fp64(G, K, C):
    plan = [((-1.0) ** c * 0.5 * (c % 3), 0.5 + (c % 4)) for c in range(C)]
    # inputs on a 2^-10 grid: two rows of a group are equal (a tie: the first row, in float64 as in fp32) or 1e-3 apart (no
    # float32 rounding can make them meet), so the arg-max is decidable and dY comparable element by element
    y = torch.round(T.plan_inputs(G * K, plan, seed=G + K) * 1024) / 1024
    res, ref = _run_bn(f"bn_relu_max G={G} K={K} C={C}", y, K=K)
    assert torch.equal(res["arg"].cpu().long(), ref["arg"])


@pytest.mark.parametrize("G,K,C", [(50, 3, 12), (300, 24, 64), (4100, 24, 64), (40, 64, 192)])
def test_bn_relu_max_lattice_ties_and_dead_groups(G, K, C):
    y = T.lattice_inputs(G * K, C, seed=G + K + C)
    y[: 3 * K] = -torch.abs(y[: 3 * K]) - 4.0   # three groups far below the mean: their maximum is <= 0 in every channel with beta small
    assert T.tie_share(y, K) > 0
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.3 * torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g)
    res, ref = _run_bn(f"bn_relu_max lattice G={G} K={K} C={C}", y, K=K, gamma_beta=(gamma, beta), groups={"all": list(range(C))})
    assert torch.equal(res["arg"].cpu().long(), ref["arg"])          # the first row among equal maxima, exactly
    dy, want = res["dy"].double().cpu(), ref["dy"]
    gs = float(want.abs().max())
    assert T.dist(dy, want, 1e-4, 2e-5 * max(gs, 1.0)) <= 1.0        # same routing: only round-off remains
    dead = (ref["out"] <= 0)
    assert bool(dead[:3].all())
    # a gradient that reaches dead groups only: exactly zero everywhere
    from hotrack_amd.train_ops import Workspace, bn_relu_max
    bn = torch.nn.BatchNorm1d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    yy = y.to(DEV).requires_grad_(True)
    out = bn_relu_max(yy, K, bn, Workspace(DEV))
    out.backward((res["go"] * dead).to(DEV))
    assert float(yy.grad.abs().max()) == 0.0 and float(bn.weight.grad.abs().max()) == 0.0 and float(bn.bias.grad.abs().max()) == 0.0


@pytest.mark.parametrize("G,K", [(300, 24), (4100, 24)])
def test_bn_relu_max_conditioning_ladder(G, K):
    plan, groups = T.ladder_plan(64)

    def decidable(ref):
        """(G, C): the float64 maximum leads the runner-up by 1e-3 and is 1e-3 away from the ReLU's kink -- at ratio 1000
        neighbouring float32 inputs are 6e-5 apart, so no fp32 rounding of the pre-activation (<~ 1e-4) reorders these or flips
        their mask."""
        top = ref["pre"].view(G, K, 64).topk(2, dim=1)[0]
        return ((top[:, 0] - top[:, 1]) > 1e-3) & (top[:, 0].abs() > 1e-3)

    # dY is compared on the rows of the decidable (group, channel) pairs: there kernel, torch and reference route the same go to the
    # same row.  The column sums inside dY still run over every group; an undecidable group that routes to its runner-up moves one
    # go between two rows whose xhat differ by < 1e-3 / |gamma|, i.e. the mean term by < 1e-3 |go| / R: far below the tolerance.
    res, ref = _run_bn(f"bn_relu_max ladder G={G}", T.plan_inputs(G * K, plan, seed=G), K=K, groups=groups,
                       dy_rows=lambda ref: decidable(ref).unsqueeze(1).expand(G, K, 64).reshape(G * K, 64))
    assert bool((res["arg"].cpu().long() == ref["arg"])[decidable(ref)].all())


def test_bn_relu_max_ld_sentinel_and_pair_launch():
    """The output as a column block of a wider buffer (columns outside untouched), and the pair launch bit for bit equal to two
    single launches (both problems on the split kernel: the pair kernel exists for that side of the switch only)."""
    from hotrack_amd import train_ops as TO
    from hotrack_amd import train_stack as TS
    lib, C = TS._lib, 64
    probs = []
    for (G, K, seed) in ((300, 24, 1), (150, 64, 2)):
        y = T.plan_inputs(G * K, [((-1.0) ** c * 0.4, 1.0 + (c % 3)) for c in range(C)], seed=seed).to(DEV)
        sums = torch.zeros(lib.pn2x_bn_sums_doubles(C), dtype=f64, device=DEV)
        TO._native._check(lib.pn2x_bn_stats(G * K, C, y.data_ptr(), C, sums.data_ptr(), TO._native._stream(y)), "bn_stats")
        probs.append((G, K, y, sums))
    gamma, beta = torch.linspace(0.7, 1.3, C, device=DEV), torch.linspace(-0.2, 0.2, C, device=DEV)

    def bufs(G):
        return (torch.full((G, C + 8), -7.0, device=DEV), torch.empty(G, C, dtype=torch.int32, device=DEV),
                torch.empty(2, C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                torch.zeros((), dtype=torch.int64, device=DEV))

    def record(p, b):
        G, K, y, sums = p
        wide, arg, saved, rm, rv, nbt = b
        return TO._BnReluMaxProblem(y=y.data_ptr(), sums=sums.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), conv_bias=None,
                                    running_mean=rm.data_ptr(), running_var=rv.data_ptr(), num_batches_tracked=nbt.data_ptr(),
                                    save_mean=saved[0].data_ptr(), save_invstd=saved[1].data_ptr(), out=wide[:, 4:].data_ptr(),
                                    arg=arg.data_ptr(), groups=G, k=K, c=C, ldy=C, ldo=C + 8, eps=1e-5, momentum=0.1)

    st = TO._native._stream(probs[0][2])
    single = [bufs(p[0]) for p in probs]
    for p, b in zip(probs, single):
        TO._native._check(lib.pn2x_bn_relu_max(*TO._records(record(p, b)), st), "bn_relu_max")
    pair = [bufs(p[0]) for p in probs]
    TO._native._check(lib.pn2x_bn_relu_max(*TO._records(record(probs[0], pair[0]), record(probs[1], pair[1])), st), "bn_relu_max")
    for p, s, q in zip(probs, single, pair):
        for a, b in zip(s, q):
            assert torch.equal(a, b)
        wide = s[0]
        assert bool((wide[:, :4] == -7.0).all()) and bool((wide[:, 4 + C:] == -7.0).all())
        ref = T.bn_reference(p[2].cpu(), gamma.cpu(), beta.cpu(), 1e-5, K=p[1])
        assert T.dist(wide[:, 4:4 + C], ref["out"], 1e-5, 2e-5) <= 1.0
        assert torch.equal(s[1].cpu().long(), ref["arg"])


# ---- sa_layer1 ----------------------------------------------------------------------------------------------------------------------
# the statistics kernel gives a workgroup max(8 x rpp, S K B / 2048) consecutive slots of a cloud (rpp = 256 / (C1 / 4) rows per
# pass): S K = 37 x 7 = 259 and 37 x 32 = 1184 are no multiples of it; K = 1: every slot a centroid of its own.
def _sa_layer1_case(name, Ks, C1s, with_feat, with_centre, variants):
    """sa_layer1 over the scales (Ks[i], C1s[i]) -- scale i reads and writes column block i of a1f / cadd and of their gradients --
    against the float64 reference scale by scale, beside the fp32 torch composition.  variants: (statistics in the launch, inverted
    neighbour lists handed in) per run; with two scales the first switch selects one two-record pn2x_sa_layer1_stats call over two
    plain launches and the second one two-record pn2x_rows_segment_sum call over two segment sums for d(a1f) (d(cadd) of two scales
    is always the pair)."""
    from hotrack_amd.train_ops import Workspace, inverse_index, sa_layer1
    B, N, S, W = 3, 300, 37, sum(C1s)
    cols = [slice(sum(C1s[:i]), sum(C1s[:i + 1])) for i in range(len(Ks))]
    g = torch.Generator().manual_seed(sum(Ks) + 2 * with_feat + 4 * with_centre)
    xyz, cxyz = torch.rand(B, N, 3, generator=g), torch.rand(B, S, 3, generator=g)
    a1f = torch.randn(B, N, W, generator=g) if with_feat else None
    cadd = torch.randn(B, S, W, generator=g) if with_centre else None
    wxs = [torch.randn(C1, 3, generator=g) for C1 in C1s]
    idxs = [T.ball_padded_idx(B, S, K, N, seed=K) for K in Ks]
    gos = [torch.randn(B, S * K, C1, generator=g) for K, C1 in zip(Ks, C1s)]
    refs = [T.sa_layer1_reference(None if a1f is None else a1f[:, :, c], None if cadd is None else cadd[:, :, c], xyz, cxyz, idx, wx, go=go)
            for c, idx, wx, go in zip(cols, idxs, wxs, gos)]
    dev = lambda t: None if t is None else t.to(DEV)
    leaves = lambda: (None if a1f is None else a1f.to(DEV).requires_grad_(True), None if cadd is None else cadd.to(DEV).requires_grad_(True),
                      [wx.to(DEV).requires_grad_(True) for wx in wxs])

    # fp32 torch composition
    ta, tc, tw = leaves()
    touts = []
    for c, K, idx, w in zip(cols, Ks, idxs, tw):
        ii = idx.view(B, S * K).long().to(DEV)
        rel = torch.gather(dev(xyz), 1, ii.unsqueeze(-1).expand(-1, -1, 3)) - dev(cxyz).repeat_interleave(K, dim=1)
        tout = rel @ w.t()
        if ta is not None:
            tout = tout + torch.gather(ta[:, :, c], 1, ii.unsqueeze(-1).expand(-1, -1, c.stop - c.start))
        if tc is not None:
            tout = tout + tc[:, :, c].repeat_interleave(K, dim=1)
        touts.append(tout)
    torch.autograd.backward(touts, [go.to(DEV) for go in gos])
    for stats, with_invs in variants:
        a, c_, ws_ = leaves()
        didx = [dev(idx) for idx in idxs]
        invs = [inverse_index(i.view(B, -1), N) for i in didx] if with_invs else None
        outs = sa_layer1(a, c_, dev(xyz), dev(cxyz), didx, ws_, invs=invs, aux={} if stats else None, ws=Workspace(DEV) if stats else None)
        torch.autograd.backward(outs, [go.to(DEV) for go in gos])
        for i, (c, K, ref) in enumerate(zip(cols, Ks, refs)):
            case = f"{name} scale {i} K={K} C1={C1s[i]} feat={with_feat} centre={with_centre} stats={stats} invs={with_invs}"
            _check(case, "out", outs[i].detach(), ref["out"], touts[i].detach(), 1e-5, 1e-4)
            if with_feat:
                _check(case, "d_a1f", a.grad[:, :, c], ref["d_a1f"], ta.grad[:, :, c], 1e-4, 1e-3)
            if with_centre:
                _check(case, "d_cadd", c_.grad[:, :, c], ref["d_cadd"], tc.grad[:, :, c], 1e-4, 1e-3)
            _check(case, "d_wx", ws_[i].grad, ref["d_wx"], tw[i].grad, 1e-4, 1e-4 * float(ref["d_wx"].abs().max()))


@pytest.mark.parametrize("with_feat,with_centre", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("K", [1, 7, 32])
def test_sa_layer1_matches_fp64(with_feat, with_centre, K):
    _sa_layer1_case("sa_layer1", [K], [32], with_feat, with_centre, [(False, False), (True, False)])


@pytest.mark.parametrize("with_feat,with_centre", [(False, False), (True, False), (False, True), (True, True)])
def test_sa_layer1_two_scales_match_fp64(with_feat, with_centre):
    """Two scales of unequal width (column blocks [0, 32) and [32, 96) of a1f / cadd): as two plain launches with the backward's
    own list inversion, and as the pair launches (pn2x_sa_layer1_stats forward; pn2x_rows_segment_sum for d(a1f) over the
    handed-in inverted lists and for d(cadd), two records each).  A wrong column offset or a row of the other scale's problem shows in out,
    d_a1f or d_cadd of one scale."""
    _sa_layer1_case("sa_layer1 pair", [7, 32], [32, 64], with_feat, with_centre, [(False, False), (True, True)])


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("C1", [32, 12])   # 12: quads that do not divide the workgroup -> sa_layer1 then pn2x_bn_stats inside
def test_sa_layer1_statistics_of_shifted_outputs(C1, pair):
    """The sums left in the workspace, for outputs with |mean| / std of about 100 (centre terms of 60 on a spread of ~0.6): the batch
    variance they imply against the float64 variance of the kernel's own (float32) output.  F: 1e-5 of the variance (the running
    variance's rtol); E_torch: torch.var of the same output in fp32."""
    from hotrack_amd import train_ops as TO
    B, N, S = 3, 300, 37
    Ks = [7, 32] if pair else [32]
    g = torch.Generator().manual_seed(C1)
    xyz, cxyz = torch.rand(B, N, 3, generator=g).to(DEV), torch.rand(B, S, 3, generator=g).to(DEV)
    a1f = (0.5 * torch.randn(B, N, C1 * len(Ks), generator=g)).to(DEV)
    cadd = (60.0 + 0.1 * torch.randn(B, S, C1 * len(Ks), generator=g)).to(DEV)
    wxs = [(0.5 * torch.randn(C1, 3, generator=g)).to(DEV) for _ in Ks]
    idxs = [T.ball_padded_idx(B, S, K, N, seed=K).to(DEV) for K in Ks]
    ws, aux = TO.Workspace(DEV), {}
    outs = TO.sa_layer1(a1f, cadd, xyz, cxyz, idxs, wxs, aux=aux, ws=ws)
    assert set(aux["sums"]) == set(range(len(Ks)))
    for i, out in enumerate(outs):
        y = out.view(-1, C1)
        R = y.shape[0]
        rep = aux["sums"][i].numel() // (2 * C1)
        s = aux["sums"][i].view(rep, 2, C1).sum(0)
        mean = s[0] / R
        var = s[1] / R - mean * mean
        y64 = y.double()
        m64 = y64.mean(0)
        v64 = (y64 - m64).pow(2).mean(0)
        ratio = float((m64.abs() / v64.sqrt()).min())
        assert 50 < ratio < 200, ratio
        case = f"sa_layer1 stats C1={C1} K={Ks[i]} pair={pair} ratio>={ratio:.0f}"
        _check(case, "mean", mean, m64, y.mean(0), 1e-5, 1e-6)
        _check(case, "var", var, v64, y.var(0, unbiased=False), 1e-5, 1e-6)


# ---- row transposes -----------------------------------------------------------------------------------------------------------------
def test_interpolate_rows_matches_fp64():
    from hotrack_amd.train_ops import interpolate_rows
    B, M, n, C = 3, 130, 500, 64
    g = torch.Generator().manual_seed(9)
    pts = torch.randn(B, M, C, generator=g)
    idx = torch.randint(0, M - 2, (B, n, 3), generator=g, dtype=torch.int32)   # rows M - 2, M - 1: named by no query
    idx[:, ::7, 1] = idx[:, ::7, 0]                                            # triples that name one source twice
    w = torch.rand(B, n, 3, generator=g)
    w = w / w.sum(-1, keepdim=True)
    w[:, ::5, 2] = 0.0                                                         # zero weights
    go = torch.randn(B, n, C, generator=g)
    a = pts.to(DEV).requires_grad_(True)
    out = interpolate_rows(a, idx.to(DEV), w.to(DEV))
    out.backward(go.to(DEV))
    b = pts.to(DEV).requires_grad_(True)
    rows = torch.gather(b, 1, idx.view(B, -1, 1).long().to(DEV).expand(-1, -1, C)).view(B, n, 3, C)
    tout = (rows * w.to(DEV).unsqueeze(-1)).sum(2)
    tout.backward(go.to(DEV))
    _check("interpolate_rows", "out", out.detach(), T.interpolate_reference(pts, idx, w), tout.detach(), 1e-5, 1e-5)
    _check("interpolate_rows", "d_points", a.grad, T.interpolate_backward(go, idx, w, M), b.grad, 1e-4, 1e-4)
    assert float(a.grad[:, M - 2:].abs().max()) == 0.0


@pytest.mark.parametrize("C", [4, 12, 128])
def test_scatter_add_rows_and_accumulating_segment_sum(C):
    """scatter_add_rows (LDS slab kernel at this size) and rows_segment_sum(accumulate=True) onto a non-zero destination; C = 12:
    quads that do not divide 256 (the one-thread-per-(row, quad) segment kernel), C = 4 / 128: the split-segment kernel."""
    from hotrack_amd.train_ops import inverse_index, rows_segment_sum, scatter_add_rows
    B, N, M = 3, 100, 1000
    g = torch.Generator().manual_seed(C)
    idx = T.ball_padded_idx(B, M // 8, 8, N - 1, seed=C).view(B, M)            # row N - 1 receives nothing
    dout, init = torch.randn(B, M, C, generator=g), torch.randn(B, N, C, generator=g)
    want = T.segment_sum_reference(dout, idx, N, init=init)
    tor = init.to(DEV).clone()
    for b in range(B):
        tor[b].index_add_(0, idx[b].long().to(DEV), dout[b].to(DEV))
    got = scatter_add_rows(dout.to(DEV), idx.to(DEV), init.to(DEV).clone())
    _check(f"scatter_add_rows C={C}", "din", got, want, tor, 1e-5, 1e-3)
    got = rows_segment_sum(dout.to(DEV), inverse_index(idx.to(DEV), N), N, init.to(DEV).clone(), accumulate=True)
    _check(f"rows_segment_sum accumulate C={C}", "din", got, want, tor, 1e-5, 1e-3)
    assert torch.equal(got[:, N - 1].cpu(), init[:, N - 1])


def test_rows_segment_sum_pair_with_an_interpolation_problem():
    """A plain row scatter (t = 1) and a weighted three-NN scatter (t = 3) over the same destination rows as ONE two-record call --
    the pair kernel covers t = 1 only, so this runs as two launches -- bit for bit equal to the two one-record calls, and both
    against float64 index_add at rows_segment_sum's tolerance (test_scatter_add_rows_and_accumulating_segment_sum)."""
    from hotrack_amd import train_ops as TO
    B, N, C = 2, 64, 8
    g = torch.Generator().manual_seed(5)
    cases = []
    for t, m in ((1, 96), (3, 40)):
        idx = torch.randint(0, N - 1, (B, m * t), generator=g, dtype=torch.int32)      # row N - 1 receives nothing
        dout = torch.randn(B, m, C, generator=g)
        w = torch.rand(B, m * t, generator=g) if t == 3 else None
        rows = lambda x, ww: x.repeat_interleave(t, dim=1) * (ww.unsqueeze(-1) if t == 3 else 1.0)  # one row per index entry
        want, tor = torch.zeros(B, N, C, dtype=f64), torch.zeros(B, N, C, device=DEV)
        for b in range(B):
            want[b].index_add_(0, idx[b].long(), rows(dout.double(), w.double() if t == 3 else None)[b])
            tor[b].index_add_(0, idx[b].long().to(DEV), rows(dout, w)[b].to(DEV))
        cases.append((dout.to(DEV), TO.inverse_index(idx.to(DEV), N), None if w is None else w.to(DEV), want, tor))
    st = TO._native._stream(cases[0][0])

    def run(which):
        dins = [torch.full((B, N, C), 3.0, device=DEV) for _ in cases]                   # accumulate = 0: overwritten
        recs = [TO._segment_sum_problem(c[0], c[1], din, c[2]) for c, din in zip(cases, dins)]
        TO._native._check(TO._lib.pn2x_rows_segment_sum(*TO._records(*(recs[i] for i in which)), B, N, 0, st), "rows_segment_sum")
        return dins

    both = run((0, 1))
    for i, (c, got) in enumerate(zip(cases, both)):
        assert torch.equal(got, run((i,))[i])
        _check(f"rows_segment_sum pair t={1 if c[2] is None else 3}", "din", got, c[3], c[4], 1e-5, 1e-3)
        assert float(got[:, N - 1].abs().max()) == 0.0


# ---- FusedAdam ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step0", [0, 9999])   # the update happens AT step 1 / step 10000: bias correction at both ends
def test_fused_adam_matches_fp64(wd, step0):
    """Tensors around the 8192-element chunk; gradient entries i % 4 == 1 exact zeros on a zero second moment (the denominator is eps
    alone), == 2 of magnitude 1e-20 (g^2 underflows in fp32), == 3 of magnitude 1e18 (g^2 = 1e36, near the top of fp32)."""
    from hotrack_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(11 + step0)
    sizes = [1, 3, 8191, 8192, 8193]
    p0 = [torch.randn(s, generator=g) for s in sizes]
    gr, m0, v0 = [], [], []
    for s in sizes:
        i = torch.arange(s) % 4
        sign = torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0)
        x = torch.randn(s, generator=g)
        x = torch.where(i == 1, torch.zeros(s), torch.where(i == 2, 1e-20 * sign, torch.where(i == 3, 1e18 * sign, x)))
        gr.append(x)
        m0.append(torch.where(i == 1, 1e-9 * torch.randn(s, generator=g), 0.1 * torch.randn(s, generator=g)))
        v0.append(torch.where(i == 1, torch.zeros(s), 0.01 * torch.rand(s, generator=g)))
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)

    def run(cls):
        ps = [p.to(DEV).clone().requires_grad_(True) for p in p0]
        src = torch.optim.Adam(ps, **hp)
        sd = src.state_dict()
        sd["state"] = {k: {"step": torch.tensor(float(step0)), "exp_avg": m0[k].to(DEV).clone(), "exp_avg_sq": v0[k].to(DEV).clone()}
                       for k in range(len(ps))}
        opt = cls(ps, **hp)
        opt.load_state_dict(sd)
        for p, x in zip(ps, gr):
            p.grad = x.to(DEV).clone()
        opt.step()
        return [p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps], \
               [float(opt.state[p]["step"]) for p in ps]

    ka, ta = run(FusedAdam), run(torch.optim.Adam)
    assert ka[3] == [float(step0 + 1)] * len(sizes)
    for k, s in enumerate(sizes):
        want = T.adam_reference(p0[k].double(), gr[k].double(), m0[k].double(), v0[k].double(), step0 + 1, 1e-3, 0.9, 0.999, 1e-8, wd)
        case = f"adam n={s} wd={wd} step={step0 + 1}"
        _check(case, "param", ka[0][k], want[0], ta[0][k], 2e-6, 2e-7)
        # exp_avg = 0.9 m0 + 0.1 (g + wd p) is a sum of terms of either sign (test_fused_adam_matches_torch_adam does not check it, so
        # there is no F to inherit): a few fp32 roundings of each term bound its error by ~2e-7 x the terms' magnitudes, not by
        # the result's, which cancels to nothing where 0.9 m0 ~ -0.1 wd p.  F: the parameters' rtol 2e-6 on the result, with that
        # rtol on the summed magnitudes as the element-wise floor -- an absolute floor of 1e-12 made this figure measure the
        # cancellation (208 F here, torch 94 F), not the kernel.
        floor = 2e-6 * (0.9 * m0[k].double().abs() + 0.1 * (gr[k].double().abs() + wd * p0[k].double().abs()))
        _check(case, "exp_avg", ka[1][k], want[1], ta[1][k], 2e-6, floor + 1e-30)
        _check(case, "exp_avg_sq", ka[2][k], want[2], ta[2][k], 2e-6, 1e-12)
        for a, b in zip((ka[0][k], ka[1][k], ka[2][k]), (ta[0][k], ta[1][k], ta[2][k])):
            assert bool(torch.isfinite(a)[torch.isfinite(b)].all())   # finite wherever fp32 torch is finite


# ---- training LayerNorm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["large_mean", "constant"])
@pytest.mark.parametrize("rows,C,two", [(21, 384, False), (100, 256, True)])
def test_tail_ln_edge_rows_match_fp64(rows, C, two, kind):
    from hotrack_amd import tail_train as TT
    g = torch.Generator().manual_seed(rows + C)
    r = lambda *s: torch.randn(*s, generator=g)
    if kind == "large_mean":
        x0 = r(rows, C) + 1000.0 * (1 + torch.arange(rows).view(rows, 1) % 3)   # rows with a large common mean
    else:
        x0 = r(rows, 1).expand(rows, C).contiguous() * 3.0                        # constant rows: variance exactly 0
    ga, ba, gb, bb = 1 + 0.3 * r(C), 0.2 * r(C), 1 + 0.3 * r(C), 0.2 * r(C)
    go = r(rows, C)

    def mods(dtype):
        na, nb = torch.nn.LayerNorm(C).to(DEV).to(dtype), torch.nn.LayerNorm(C).to(DEV).to(dtype)
        with torch.no_grad():
            for m, w, b in ((na, ga, ba), (nb, gb, bb)):
                m.weight.copy_(w)
                m.bias.copy_(b)
        return na, nb

    na, nb = mods(torch.float32)
    x = x0.to(DEV).requires_grad_(True)
    out = TT.ln(x, na, nb if two else None, TT.TailGrads(DEV, 8 * C))
    out.backward(go.to(DEV))
    res = {}
    for dtype in (torch.float32, f64):
        ma, mb = mods(dtype)
        xx = x0.to(DEV).to(dtype).requires_grad_(True)
        o = ma(xx)
        o = mb(o) if two else o
        o.backward(go.to(DEV).to(dtype))
        res[dtype] = (o.detach(), xx.grad, ma.weight.grad, ma.bias.grad, mb.weight.grad if two else None, mb.bias.grad if two else None)
    got = (out.detach(), x.grad, na.weight.grad, na.bias.grad, nb.weight.grad if two else None, nb.bias.grad if two else None)
    case = f"tail_ln {kind} rows={rows} C={C} two={two}"
    for name, a, w, t in zip(("out", "dx", "dga", "dba", "dgb", "dbb"), got, res[f64], res[torch.float32]):
        if w is None:
            continue
        if name == "out":
            _check(case, name, a, w, t, 1e-5, 1e-5)
        else:
            _check(case, name, a, w, t, 0.0, 1e-4 * (float(w.abs().max()) + 1e-12))


# ---- mlp_stack ----------------------------------------------------------------------------------------------------------------------
def _stack_case(shifted, seed):
    """(32 x 64 rows, [32, 32, 64], max over 32): the smallest shape of test_mlp_stack_matches_torch.  shifted: the input rows share
    an offset of 150 (layer 1's pre-activations: |mean| / std ~ 100, statistics from pn2x_bn_stats), and layer 1's BatchNorm has
    gamma 0.1 / beta 2 with near-uniform positive layer-2 weights, so that layer 2's pre-activations -- whose statistics come from
    the fused GEMM's epilogue -- have |mean| / std ~ 100 as well."""
    R, widths, K = 32 * 64, [32, 32, 64], 32
    g = torch.Generator().manual_seed(seed)
    y1 = torch.randn(R, widths[0], generator=g) * 1.5 + (150.0 if shifted else 0.3)
    Ws = [torch.randn(b, a, generator=g) / a ** 0.5 for a, b in zip(widths[:-1], widths[1:])]
    gammas = [1 + 0.3 * torch.randn(c, generator=g) for c in widths]
    betas = [0.2 * torch.randn(c, generator=g) for c in widths]
    if shifted:
        gammas[0], betas[0] = torch.full((widths[0],), 0.1), torch.full((widths[0],), 2.0)
        Ws[0] = (1.0 + 0.2 * torch.randn(widths[1], widths[0], generator=g)) / widths[0]
    go = torch.randn(R // K, widths[-1], generator=g)
    return R, widths, K, y1, Ws, gammas, betas, go


def _stack_torch(case, dtype):
    R, widths, K, y1, Ws, gammas, betas, go = case
    bns = [torch.nn.BatchNorm1d(c, momentum=0.07).to(DEV).to(dtype).train() for c in widths]
    Wp = [W.to(DEV).to(dtype).requires_grad_(True) for W in Ws]
    with torch.no_grad():
        for bn, ga, be in zip(bns, gammas, betas):
            bn.weight.copy_(ga)
            bn.bias.copy_(be)
    y = y1.to(DEV).to(dtype).requires_grad_(True)
    pres = [bns[0](y)]
    h = torch.relu(pres[0])
    for W, bn in zip(Wp, bns[1:]):
        pres.append(bn(h @ W.t()))
        h = torch.relu(pres[-1])
    out = h.view(R // K, K, -1).max(dim=1)[0]
    out.backward(go.to(DEV).to(dtype))
    margin = min(float(p.detach().abs().min()) for p in pres)
    return out.detach(), y.grad, Wp, bns, margin, pres


_STACK_RUNS = {}


def _stack_run(shifted):
    """Runs mlp_stack once per case (shared by the tests below) beside the float64 and fp32 torch modules, prints every quantity's
    distances and returns {"ratios": realised |mean| / std range of layer 1's and layer 2's pre-activations,
    "dist": {quantity: (kernel distance, torch distance, bound)}}.  Asserts nothing about the kernel."""
    if shifted in _STACK_RUNS:
        return _STACK_RUNS[shifted]
    from hotrack_amd import train_stack
    from hotrack_amd.train_ops import Workspace
    for attempt in range(200):   # a draw whose float64 ReLU inputs keep clear of zero (test_mlp_stack_matches_torch: KINK_MARGIN)
        case = _stack_case(shifted, 77 + 1000 * attempt)
        ref = _stack_torch(case, f64)
        if ref[4] >= 2e-6:
            break
    else:
        raise RuntimeError("no draw with a kink margin")
    R, widths, K, y1, Ws, gammas, betas, go = case
    ratios = []
    for i in (0, 1):
        pre_in = y1.double() if i == 0 else (torch.relu(ref[5][0].detach()) @ Ws[0].double().to(DEV).t()).cpu()
        ratio = T.realised_ratio(pre_in)
        ratios.append((float(ratio.min()), float(ratio.max())))
    tor = _stack_torch(case, torch.float32)
    bns = [torch.nn.BatchNorm1d(c, momentum=0.07).to(DEV).train() for c in widths]
    with torch.no_grad():
        for bn, ga, be in zip(bns, gammas, betas):
            bn.weight.copy_(ga)
            bn.bias.copy_(be)
    Wp = [W.to(DEV).requires_grad_(True) for W in Ws]
    cb = [torch.zeros(c, device=DEV, requires_grad=True) for c in widths]
    if not train_stack.stack_supported(widths[0], widths[1:]):
        raise RuntimeError("the smallest shape of test_mlp_stack_matches_torch is no longer supported")
    layers = [train_stack.Layer(None, bns[0], cb[0])] + [train_stack.Layer(W, bn, b) for W, bn, b in zip(Wp, bns[1:], cb[1:])]
    ya = y1.to(DEV).requires_grad_(True)
    out = train_stack.mlp_stack(ya, layers, Workspace(DEV), max_over=K)
    out.backward(go.to(DEV))
    name, d = f"mlp_stack shifted={shifted}", {}
    d["out"] = _measure(name, "out", out.detach(), ref[0], tor[0], 2e-4, 2e-4)
    sc = lambda t: 2e-3 * (float(t.abs().max()) + 1e-12)
    d["dy1"] = _measure(name, "dy1", ya.grad, ref[1], tor[1], 0.0, sc(ref[1]))
    for i in range(len(widths)):
        n = i + 1
        d[f"running_mean{n}"] = _measure(name, f"running_mean{n}", bns[i].running_mean, ref[3][i].running_mean, tor[3][i].running_mean, 1e-4, 1e-5)
        d[f"running_var{n}"] = _measure(name, f"running_var{n}", bns[i].running_var, ref[3][i].running_var, tor[3][i].running_var, 1e-4, 1e-5)
        d[f"dgamma{n}"] = _measure(name, f"dgamma{n}", bns[i].weight.grad, ref[3][i].weight.grad, tor[3][i].weight.grad, 0.0, sc(ref[3][i].weight.grad))
        d[f"dbeta{n}"] = _measure(name, f"dbeta{n}", bns[i].bias.grad, ref[3][i].bias.grad, tor[3][i].bias.grad, 0.0, sc(ref[3][i].bias.grad))
    for i in range(len(Ws)):
        d[f"dW{i + 2}"] = _measure(name, f"dW{i + 2}", Wp[i].grad, ref[2][i].grad, tor[2][i].grad, 0.0, sc(ref[2][i].grad))
    _STACK_RUNS[shifted] = {"ratios": ratios, "dist": d}
    return _STACK_RUNS[shifted]


def _outside(run, names):
    return {n: run["dist"][n] for n in names if not run["dist"][n][0] <= run["dist"][n][2]}


# What of the shifted case rests on which producer of the sums.  Layer 1's statistics come from pn2x_bn_stats, and the sum of y of
# layer 2 (its running mean) is taken over layer 1's output and does not cancel.  Everything else passes through layer 2's batch
# variance, which the fused GEMM's epilogue forms from fp32 sums of y and y^2: layer 2's running variance, the output, layer 3's
# statistics (its input is layer 2's output), and every gradient (all of them come back through layers 3 and 2).
_STACK_PIVOTED = ("running_mean1", "running_var1", "running_mean2")
_STACK_EPILOGUE = ("out", "running_var2", "running_mean3", "running_var3", "dy1", "dgamma1", "dbeta1", "dgamma2", "dbeta2", "dgamma3",
                   "dbeta3", "dW2", "dW3")


def test_mlp_stack_matches_fp64():
    """The smallest shape of test_mlp_stack_matches_torch, unshifted: every quantity."""
    run = _stack_run(False)
    assert sorted(run["dist"]) == sorted(_STACK_PIVOTED + _STACK_EPILOGUE)
    assert not _outside(run, _STACK_PIVOTED + _STACK_EPILOGUE)


def test_mlp_stack_shifted_rows_case_and_layer1_statistics():
    """The shifted case is what it claims -- |mean| / std of about 100 in the pre-activations of layer 1 AND of layer 2, the only case
    here that reaches the GEMM-epilogue statistics -- and what rests on pn2x_bn_stats alone meets the bound."""
    run = _stack_run(True)
    for lo, hi in run["ratios"]:
        assert 50 < lo and hi < 400, run["ratios"]
    assert not _outside(run, _STACK_PIVOTED)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=(
    "the statistics epilogues of the fused GEMMs (train_fwd.hip / train_gemm.hip) still sum y and y^2 in fp32: with layer 2's "
    "pre-activations at |mean| / std ~ 110 the stack's output is 5.9 F from float64 (F: rtol = atol = 2e-4) where fp32 torch is "
    "0.41 F and the bound 1.63 F, and dY_1 1.04 F (F: 2e-3 of its maximum; torch 0.0015 F, bound F); every other quantity is inside "
    "F.  Supported ratio for these producers: DESIGN.md, 'Conditioning of the BatchNorm statistics'"))
def test_mlp_stack_shifted_rows_epilogue_statistics():
    """Only the quantities fed by the GEMM-epilogue statistics of layers 2 and 3 (_STACK_EPILOGUE); the case's own conditions and
    layer 1 are asserted by the test above, and anything but a missed bound here (RuntimeError from the set-up) is a failure."""
    run = _stack_run(True)
    if not all(50 < lo and hi < 400 for lo, hi in run["ratios"]):
        raise RuntimeError(f"the shifted case is not at |mean| / std ~ 100: {run['ratios']}")
    missed = _outside(run, _STACK_EPILOGUE)
    assert not missed, f"(kernel, torch, bound) in F: {missed}"
