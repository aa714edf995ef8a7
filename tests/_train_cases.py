"""Float64 references and seeded input builders for the training operators (hotrack_amd/csrc/train_ops.hip, adam.hip, the
statistics epilogues of train_fwd.hip / train_gemm.hip, tail_train.hip's LayerNorm).  Everything here is CPU tensors and is
written from the formulas -- nothing calls project code; tests/test_train_cases.py checks that the builders produce what they
claim and anchors the BatchNorm reference to torch.nn.BatchNorm1d in float64, tests/test_gpu_train_fp64.py runs the kernels.

  bn_reference        train-mode BatchNorm (+ ReLU) (+ max over K consecutive rows, first row wins ties): output, arg-max, batch
                      mean / biased variance / invstd, running-statistics update, dY / dgamma / dbeta for an upstream gradient
  sa_layer1_reference a1f[idx] + (xyz[idx] - centre) Wx^T + cadd per centroid, and its gradients
  segment_sum_reference / interpolate_reference / interpolate_backward / gather_backward     the row gathers and their transposes
  adam_reference      Adam with (L2) weight decay and bias correction from a given state and step
  plan_inputs         (R, C) float32 pre-activations whose channels realise a per-channel (mean, std) plan
  lattice_inputs      pre-activations rounded to a coarse lattice: equal maxima inside a group are common
  bound               max(F, 4 x E_torch): the tolerance rule of test_gpu_train_fp64.py
"""
import torch

f64 = torch.float64

# The conditioning ladder: std 1 and |mean| / std of 0, 10, 100, 1000, and one narrow channel (mean 0.5, std 1e-3: ratio 500).
LADDER = ((0.0, 1.0), (10.0, 1.0), (100.0, 1.0), (1000.0, 1.0), (0.5, 1e-3))
LADDER_NAMES = ("ratio0", "ratio10", "ratio100", "ratio1000", "narrow500")
TORCH_MARGIN = 4.0  # the margin a fp32 route gets over torch's own fp32 distance from fp64 (GEOM_TOL, test_gpu_hand_pose_mano.py)


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------
def bn_reference(y, gamma, beta, eps, go=None, relu=True, K=0, conv_bias=None, running_mean=None, running_var=None, momentum=0.1):
    """y (R, C), go the upstream gradient ((R, C), or (R / K, C) with K); every tensor is taken to float64.  Returns a dict."""
    y, gamma, beta = y.to(f64), gamma.to(f64), beta.to(f64)
    R, C = y.shape
    mean = y.sum(0) / R
    d = y - mean
    var = (d * d).sum(0) / R                    # biased (two-pass: no cancellation)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * invstd
    pre = xhat * gamma + beta
    h = torch.where(pre > 0, pre, torch.where(pre != pre, pre, torch.zeros_like(pre))) if relu else pre
    res = {"mean": mean, "var": var, "invstd": invstd, "pre": pre}
    if running_mean is not None:
        bm = mean + (conv_bias.to(f64) if conv_bias is not None else 0.0)   # the bias only shifts the batch mean
        unbiased = var * (R / (R - 1.0)) if R > 1 else var
        res["running_mean"] = (1 - momentum) * running_mean.to(f64) + momentum * bm
        res["running_var"] = (1 - momentum) * running_var.to(f64) + momentum * unbiased
    if K:
        G = R // K
        pk = pre.view(G, K, C)                  # the arg-max is taken in front of the ReLU (max and ReLU commute; a group whose
        top = pk.max(dim=1)[0]                  # maximum is <= 0 still names its largest row, and receives no gradient)
        arg = torch.argmax((pk == top.unsqueeze(1)).to(torch.int64), dim=1)   # the first of equal values: the first row wins ties
        res["out"], res["arg"] = h.view(G, K, C).max(dim=1)[0], arg
    else:
        res["out"] = h
    if go is not None:
        go = go.to(f64)
        if K:
            g = torch.zeros(G, K, C, dtype=f64)
            g.scatter_(1, res["arg"].unsqueeze(1), go.unsqueeze(1))
            g = g.view(R, C)
        else:
            g = go
        if relu:
            g = torch.where(pre > 0, g, torch.zeros_like(g))
        sg, sgx = g.sum(0), (g * xhat).sum(0)
        res["dy"] = gamma * invstd * (g - sg / R - xhat * (sgx / R))
        res["dgamma"], res["dbeta"] = sgx, sg
    return res


def plan_inputs(R, plan, seed):
    """(R, len(plan)) float32: channel c is standard-normal draws standardised to zero mean / unit variance exactly (in float64),
    scaled by plan[c][1], shifted by plan[c][0], then rounded to float32 (the rounding moves mean and std by ~6e-8 |mean|)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(R, len(plan), generator=g, dtype=f64)
    if R > 1:
        z = z - z.mean(0)
        z = z / z.pow(2).mean(0).sqrt()
    mean = torch.tensor([p[0] for p in plan], dtype=f64)
    std = torch.tensor([p[1] for p in plan], dtype=f64)
    return (z * std + mean).float()


def ladder_plan(C):
    """C channels cycling through LADDER; returns (plan, {rung name: channel indices})."""
    plan = [LADDER[c % len(LADDER)] for c in range(C)]
    groups = {n: [c for c in range(C) if c % len(LADDER) == i] for i, n in enumerate(LADDER_NAMES)}
    return plan, groups


def realised_ratio(y):
    y = y.to(f64)
    m = y.mean(0)
    return m.abs() / (y - m).pow(2).mean(0).sqrt()


def lattice_inputs(R, C, seed, step=0.5, scale=1.5, shift=-0.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.round((torch.randn(R, C, generator=g) * scale + shift) / step) * step).contiguous()


def tie_share(y, K):
    """Share of (group, channel) pairs whose maximum over the K rows is attained more than once."""
    G = y.shape[0] // K
    yk = y[:G * K].view(G, K, -1)
    return float(((yk == yk.max(dim=1, keepdim=True)[0]).sum(1) > 1).double().mean())


# ---- the first layer of a set-abstraction scale -------------------------------------------------------------------------------------
def _rows(t, idx):
    B, C = t.shape[0], t.shape[2]
    return torch.gather(t, 1, idx.reshape(B, -1, 1).long().expand(-1, -1, C))


def sa_layer1_reference(a1f, cadd, xyz, cxyz, idx, wx, go=None):
    """a1f (B, N, C1) | None, cadd (B, S, C1) | None, xyz (B, N, 3), cxyz (B, S, 3), idx (B, S, K), wx (C1, 3) -> dict with
    out (B, S K, C1), rel (B, S K, 3) and, for go (B, S K, C1), d_a1f, d_cadd, d_wx."""
    B, S, K = idx.shape
    xyz, cxyz, wx = xyz.to(f64), cxyz.to(f64), wx.to(f64)
    rel = _rows(xyz, idx) - cxyz.repeat_interleave(K, dim=1)
    out = rel @ wx.t()
    if a1f is not None:
        out = out + _rows(a1f.to(f64), idx)
    if cadd is not None:
        out = out + cadd.to(f64).repeat_interleave(K, dim=1)
    res = {"out": out, "rel": rel}
    if go is not None:
        go = go.to(f64)
        if a1f is not None:
            res["d_a1f"] = segment_sum_reference(go, idx.reshape(B, -1), a1f.shape[1])
        if cadd is not None:
            res["d_cadd"] = go.view(B, S, K, -1).sum(2)
        res["d_wx"] = torch.einsum("brc,brt->ct", go, rel)
    return res


def ball_padded_idx(B, S, K, N, seed):
    """Neighbour lists padded the way a ball query pads them: a ball holds 1 .. K distinct hits, the rest repeat its first index."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, N, (B, S, K), generator=g, dtype=torch.int32)
    hits = torch.randint(1, K + 1, (B, S, 1), generator=g)
    pad = torch.arange(K).view(1, 1, K) >= hits
    return torch.where(pad, idx[:, :, :1].expand(-1, -1, K), idx).contiguous()


# ---- row scatters / gathers ---------------------------------------------------------------------------------------------------------
def segment_sum_reference(src, idx, n_dst, weight=None, init=None):
    """dst[b, idx[b, e], :] += (weight[b, e] *) src[b, e // t, :] with t = idx.shape[1] // src.shape[1], from `init` or zeros."""
    B, M, C = src.shape
    t = idx.shape[1] // M
    s = src.to(f64).repeat_interleave(t, dim=1)
    if weight is not None:
        s = s * weight.to(f64).reshape(B, -1, 1)
    dst = torch.zeros(B, n_dst, C, dtype=f64) if init is None else init.to(f64).clone()
    for b in range(B):
        dst[b].index_add_(0, idx[b].long(), s[b])
    return dst


def interpolate_reference(points, idx, weight):
    """points (B, M, C), idx / weight (B, n, 3) -> (B, n, C)."""
    B, n, _ = idx.shape
    rows = _rows(points.to(f64), idx).view(B, n, 3, -1)
    return (rows * weight.to(f64).unsqueeze(-1)).sum(2)


def interpolate_backward(go, idx, weight, M):
    B, n, _ = idx.shape
    return segment_sum_reference(go, idx.reshape(B, n * 3), M, weight=weight.reshape(B, n * 3))


def gather_backward(go, idx, N):
    return segment_sum_reference(go, idx, N)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
def adam_reference(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """One Adam step (L2 weight decay added to the gradient, bias correction) arriving at step number `step` (>= 1) in `dtype` of p."""
    dt = p.dtype
    p, g, m, v = p.clone(), g.to(dt), m.clone(), v.clone()
    if weight_decay:
        g = g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    return p - (lr / bc1) * (m / denom), m, v


# ---- the tolerance rule -------------------------------------------------------------------------------------------------------------
def dist(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|) in float64 (NaN anywhere -> inf; positions where both are NaN are skipped).  atol: a
    number, or a tensor shaped like ref (an element-wise floor)."""
    got, ref = got.detach().to(f64).cpu(), ref.detach().to(f64).cpu()
    if torch.is_tensor(atol):
        atol = atol.detach().to(f64).cpu()
    both_nan = (got != got) & (ref != ref)
    r = (got - ref).abs() / (atol + rtol * ref.abs())
    r = torch.where(both_nan, torch.zeros_like(r), r)
    if r.numel() == 0:
        return 0.0
    r = torch.where(r != r, torch.full_like(r, float("inf")), r)
    return float(r.max())


def bound(e_torch):
    """In units of the operator's existing tolerance F (dist() <= 1 means inside F): max(F, 4 x E_torch)."""
    return max(1.0, TORCH_MARGIN * e_torch)
