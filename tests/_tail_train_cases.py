"""Host-side restatement of the training tail (hotrack_amd/csrc/tail_train.hip) for tests: the dropout keep-mask as an exact
integer function, float64 references of the three fused element-wise runs and of the whole of FastTail.forward under those masks,
and running error bounds for the outputs that are sums of products.  Not a test file; imports without a GPU.

The mask (tail_train.hip's header: "a hash of (seed, site, element index)"): element i of dropout site `site` in the forward whose
counter value is `seed` is kept iff the high 32 bits of SplitMix64's output function, applied to the 64-bit state
seed * golden + (site << 40) + i, are >= p * 2^32 (p as the float32 the kernel receives, the product in float64, truncated).
i is the flat index row * c + ch.  Kept elements are scaled by 1 / (1 - p): in float32 in the kernel (SCALE32), in float64 in the
references.

The running bounds (bound = K * u * A, u = 2^-24): A is the output's own expression in float64 with every term replaced by its
absolute value (so it carries the inputs' magnitudes and any cancellation), K twice the number of float32 roundings on the longest
path to the output -- twice for the float32 dropout scale and fused-multiply slack; a sum of n terms by atomics or butterflies
counts n - 1 roundings whatever its order.  The counts stand next to each function."""
import numpy as np
import torch

f64 = torch.float64
U = 2.0 ** -24
_M64 = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


# ---- the mask --------------------------------------------------------------------------------------------------------------------
def mix64(seed, site, idx):
    """The 64-bit hash of (seed, site, idx) -- idx an integer array -- as a numpy uint64 array (wrapping arithmetic)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.full(idx.shape, int(seed) & _M64, dtype=np.uint64) * np.uint64(GOLDEN) + (np.uint64(site) << np.uint64(40)) + idx
        z ^= z >> np.uint64(30)
        z *= np.uint64(MIX1)
        z ^= z >> np.uint64(27)
        z *= np.uint64(MIX2)
        z ^= z >> np.uint64(31)
    return z


def mix64_int(seed, site, i):
    """The same hash on plain Python integers masked to 64 bits (the numpy restatement is checked against this)."""
    z = ((int(seed) & _M64) * GOLDEN + (int(site) << 40) + int(i)) & _M64
    z ^= z >> 30
    z = z * MIX1 & _M64
    z ^= z >> 27
    z = z * MIX2 & _M64
    z ^= z >> 31
    return z


def drop_threshold(p):
    p32 = np.float32(p)
    if p32 <= 0:
        return 0
    if p32 >= 1:
        return 0xFFFFFFFF
    return int(np.float64(p32) * 2.0 ** 32)


def keep_mask(seed, site, n, p):
    """bool (n,): element i of site `site` is kept in the forward whose counter value is `seed`."""
    hi = mix64(seed, site, np.arange(n, dtype=np.uint64)) >> np.uint64(32)
    return hi >= np.uint64(drop_threshold(p))


def mask_tensor(seed, site, shape, p):
    """keep_mask as a bool tensor of `shape` (row-major: the flat index is row * c + ch)."""
    n = int(np.prod(shape))
    return torch.from_numpy(keep_mask(seed, site, n, p)).view(*shape)


def scale32(p):
    """1 / (1 - p) as the kernels form it: float32 throughout."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def scale64(p):
    """1 / (1 - p) for the references: p as the float32 the kernel receives, the rest in float64."""
    return 1.0 / (1.0 - float(np.float32(p)))


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def _leaf(t):
    return None if t is None else t.detach().cpu().to(f64).requires_grad_(True)


def _grad(t):
    return None if t is None else t.grad


def ln_reference(x, ga, ba, eps_a, gb=None, bb=None, eps_b=0.0, y=None, bias=None, p=0.0, site=0, seed=0, go=None):
    """LN_b(LN_a(x + mask * (y + bias) * scale)) on rows (R, C), float64 on the float32 inputs; LN_b when gb is given.  With `go`
    also the gradients.  Returns a dict: out, mask, and dx, dy, dbias, dga, dba, dgb, dbb (None where there is no such input)."""
    xd, yd, bd, gad, bad, gbd, bbd = (_leaf(t) for t in (x, y, bias, ga, ba, gb, bb))
    rows, c = xd.shape
    mask = mask_tensor(seed, site, (rows, c), p)
    u = xd
    if yd is not None:
        d = yd + bd if bd is not None else yd
        u = xd + mask.to(f64) * d * scale64(p)
    out = torch.nn.functional.layer_norm(u, (c,), gad, bad, eps_a)
    if gbd is not None:
        out = torch.nn.functional.layer_norm(out, (c,), gbd, bbd, eps_b)
    res = {"out": out.detach(), "mask": mask}
    if go is not None:
        out.backward(go.detach().cpu().to(f64))
        res.update(dx=xd.grad, dy=_grad(yd), dbias=_grad(bd), dga=gad.grad, dba=bad.grad, dgb=_grad(gbd), dbb=_grad(bbd))
    return res


def relu_drop_reference(z, bias=None, p=0.0, site=0, seed=0, dh=None):
    """mask * relu(z + bias) * scale in float64; with `dh` also dz, dbias, and dbias_abs -- dbias with every term replaced by its
    absolute value (the A of its running bound)."""
    zd, bd = _leaf(z), _leaf(bias)
    mask = mask_tensor(seed, site, tuple(zd.shape), p)
    out = mask.to(f64) * torch.relu(zd + bd if bd is not None else zd) * scale64(p)
    res = {"out": out.detach(), "mask": mask}
    if dh is not None:
        dhd = dh.detach().cpu().to(f64)
        out.backward(dhd)
        pos = (zd + bd if bd is not None else zd).detach() > 0
        res.update(dz=zd.grad, dbias=_grad(bd), dbias_abs=((mask & pos).to(f64) * dhd.abs() * scale64(p)).sum(0))
    return res


def relu_drop_dbias_bound(rows, dbias_abs):
    """dbias[ch] = sum over rows of dh * scale where kept and positive.  Roundings on the longest path: 1 (dh * scale) + rows - 1
    (a wave's four rows, four waves in LDS, one atomic per 16-row workgroup: a sum of `rows` terms in some order) = rows; K = 2 rows."""
    return 2 * rows * U * dbias_abs


def pose_head_reference(h, w, bias, xyz1, R, t, scale, g_hand=None, g_cam=None):
    """kp_hand (B,3,J) = (h w^T + bias)[b, j, :] transposed + xyz1;  kp_cam (B,J,3) = scale_b R_b kp_hand[b, :, j] + t_b -- the
    layout tail_train.pose_head documents -- in float64, with dh, dw, dbias for the given output gradients, and under "abs" the
    same five quantities with every term replaced by its absolute value (pose_head_bounds)."""
    hd, wd, bd = _leaf(h), _leaf(w), _leaf(bias)
    B, _, J = xyz1.shape
    xd, Rd, td = xyz1.detach().cpu().to(f64), R.detach().cpu().to(f64).reshape(B, 3, 3), t.detach().cpu().to(f64).reshape(B, 3, 1)
    sd = scale.detach().cpu().to(f64).reshape(-1).expand(B) if scale.numel() == 1 else scale.detach().cpu().to(f64).reshape(B)
    kp_hand = (hd @ wd.t() + bd).view(B, J, 3).transpose(1, 2) + xd
    kp_cam = (sd.view(B, 1, 1) * (Rd @ kp_hand) + td).transpose(1, 2)
    a_hand = (hd.detach().abs() @ wd.detach().abs().t() + bd.detach().abs()).view(B, J, 3).transpose(1, 2) + xd.abs()
    a_cam = (sd.abs().view(B, 1, 1) * (Rd.abs() @ a_hand) + td.abs()).transpose(1, 2)
    res = {"kp_hand": kp_hand.detach(), "kp_cam": kp_cam.detach(), "abs": {"kp_hand": a_hand, "kp_cam": a_cam}}
    if g_hand is not None or g_cam is not None:
        gh = None if g_hand is None else g_hand.detach().cpu().to(f64)
        gc = None if g_cam is None else g_cam.detach().cpu().to(f64)
        loss = (0 if gh is None else (kp_hand * gh).sum()) + (0 if gc is None else (kp_cam * gc).sum())
        loss.backward()
        # |g| of a token: |d kp_hand| + |scale| |R|^T |d kp_cam|, as rows (B*J, 3)
        ag = torch.zeros(B, 3, J, dtype=f64)
        if gh is not None:
            ag = ag + gh.abs()
        if gc is not None:
            ag = ag + sd.abs().view(B, 1, 1) * (Rd.abs().transpose(1, 2) @ gc.abs().transpose(1, 2))
        ag = ag.transpose(1, 2).reshape(B * J, 3)
        res.update(dh=hd.grad, dw=wd.grad, dbias=bd.grad)
        res["abs"].update(dh=ag @ wd.detach().abs(), dw=ag.t() @ hd.detach().abs(), dbias=ag.sum(0))
    return res


def pose_head_bounds(B, J, C, ref, cam_grad):
    """Running bounds of the pose head's five outputs from pose_head_reference(...)["abs"].  Float32 roundings on the longest path:

      kp_hand   C + 2 terms (C products, bias, xyz1) summed per lane and by a wave butterfly: C + 1 additions, and one rounding
                for the products (fused into the lane's running sum)                                              -> C + 2
      kp_cam    kp_hand's, then 3 products + 2 additions, the product with scale, the addition of t            -> C + 2 + 7
      g         (a token's gradient of kp_hand, read by all three below) with d kp_cam: 3 products + 2 additions, the product
                with scale, the addition to d kp_hand -> 7; with d kp_hand alone it is read as it is           -> 0
      dh        g's, then 3 products + 2 additions                                                             -> g + 5
      dw        g's, one product, tokens - 1 additions (32 tokens per thread, one atomic per 32 tokens)        -> g + tokens
      dbias     g's, tokens - 1 additions (as dw)                                                              -> g + tokens - 1

    K is twice the count."""
    tokens, g = B * J, (7 if cam_grad else 0)
    a = ref["abs"]
    counts = {"kp_hand": C + 2, "kp_cam": C + 9, "dh": g + 5, "dw": g + tokens, "dbias": g + tokens - 1}
    return {k: 2 * max(n, 1) * U * a[k] for k, n in counts.items() if k in a}, {k: 2 * max(n, 1) for k, n in counts.items()}


def tail_reference(net, rows, xyz1, canon, seed):
    """The whole of FastTail.forward in float64 on the net's own parameters: token-major rows (B*J, C) through LN(s11.norm1),
    LN(c11.norm1), c11's FFN block, c3's LayerNorm and FFN block, final_mlp and the pose head, with the dropout sites 1-4 drawn by
    keep_mask from `seed` (the p of each site read from its module; 0 when the module is in eval mode).

    Returns (kp_hand (B,3,J), kp_cam (B,J,3), leaves): leaves maps "rows" and every parameter name of `net` that takes part to its
    float64 leaf, so the caller can run a backward and read the gradients."""
    F = torch.nn.functional
    s11, c11, c3, fm = net.transt.s11, net.transt.c11, net.c3, net.final_mlp
    names = {id(p): k for k, p in net.named_parameters()}
    leaves = {"rows": _leaf(rows)}

    def P(param):
        k = names[id(param)]
        if k not in leaves:
            leaves[k] = _leaf(param)
        return leaves[k]

    def norm(m, x):
        return F.layer_norm(x, tuple(m.normalized_shape), P(m.weight), P(m.bias), m.eps)

    def drop(m, site, x):
        p = float(m.p) if m.training else 0.0
        return mask_tensor(seed, site, tuple(x.shape), p).to(f64) * x * scale64(p)

    def block(m, x, site):  # x + dropout3(linear2(dropout2(relu(linear1(x))))), then norm2
        d = drop(m.dropout2, site, torch.relu(F.linear(x, P(m.linear1.weight), P(m.linear1.bias))))
        return norm(m.norm2, x + drop(m.dropout3, site + 1, F.linear(d, P(m.linear2.weight), P(m.linear2.bias))))

    B, _, J = xyz1.shape
    h = norm(c11.norm1, norm(s11.norm1, leaves["rows"]))
    h2 = norm(c3.norm1, block(c11, h, 1))
    h3 = block(c3, h2, 3)
    hf = torch.relu(F.linear(h3, P(fm[0].weight).squeeze(-1), P(fm[0].bias)))
    tok = F.linear(hf, P(fm[2].weight).squeeze(-1), P(fm[2].bias))                      # (B*J, 3)
    kp_hand = tok.view(B, J, 3).transpose(1, 2) + xyz1.detach().cpu().to(f64)
    sc = canon["scale"].detach().cpu().to(f64).reshape(-1)
    Rd = canon["rotation"].detach().cpu().to(f64).reshape(B, 3, 3)
    td = canon["translation"].detach().cpu().to(f64).reshape(B, 3, 1)
    kp_cam = (sc.view(-1, 1, 1) * (Rd @ kp_hand) + td).transpose(1, 2)
    return kp_hand, kp_cam, leaves


# ---- comparison helpers ----------------------------------------------------------------------------------------------------------
def worst(got, want, bound):
    """max over elements of |got - want| / bound (bound: a number or a tensor shaped like want); (ratio, max error, bound there)."""
    err = (got.detach().cpu().to(f64) - want).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    ratio = err / b.clamp_min(1e-300)
    ratio = torch.where((err == 0) & (b == 0), torch.zeros_like(ratio), ratio)
    k = int(ratio.argmax())
    return float(ratio.flatten()[k]), float(err.flatten()[k]), float(b.flatten()[k])
