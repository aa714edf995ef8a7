"""Float64 references, seeded input builders and case lists for ONE fused [Conv 1x1 + BatchNorm + ReLU] layer of the training
stacks (hotrack_amd/csrc/train_gemm.hip, train_fwd.hip, train_bwd.hip; formulas: include/pn2_ext.h, "Train-mode [Conv 1x1 +
BatchNorm + ReLU] layers" and "The whole backward of fused layer i").  CPU tensors only, written from the formulas -- nothing
here calls project code.  tests/test_stack_layer_cases.py anchors the references to torch autograd in float64 and checks the
builders' claims, tests/test_gpu_stack_layers_fp64.py runs the kernels through the C ABI.

  layer_forward_reference    mean / invstd of layer p from sums_in, its running statistics, y = relu(BN_p(x)) w^T, [sum y | sum y^2]
  layer_backward_reference   g of layer i (three sources), dY_i, g_p, sums_bwd_p, dW, dgamma_i / dbeta_i
  forward_case / backward_case   seeded inputs whose ReLU masks stay MASK_MARGIN clear of zero
  *_CASES                    the shapes (data; one line per case saying which branch it reaches)

`p` is layer i-1 (k channels), `i` layer i (n channels), w (n, k), as in the header.  A whole stack is ill-conditioned because
its masks depend on computed statistics; here mean_* / invstd_* / sums_* are INPUTS (float32 / float64 numbers the kernel and
the reference both read), so a mask depends on given numbers only and the result is a short dot product.

The tolerance rule is _train_cases.bound: distance <= max(F, 4 x E_torch), F = the floor of a length-L fp32 dot product,
L 2^-24 sum |a_i| |b_i|, maximised over the outputs and computed from the reference (the "F" entry of each reference's result); E_torch is measured by
the GPU test."""
import torch

import _train_cases as T

f64 = torch.float64
U = 2.0 ** -24      # unit round-off of float32
REP = 8             # copies of every fp64 accumulator (pn2x_bn_sums_doubles(c) = 2 c REP; copy r: [r 2 ld, r 2 ld + ld) | [.. + ld, ..))
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the entries take eps / momentum as float32: these exact values
MOMENTUM = float(torch.tensor(0.07, dtype=torch.float32))

# ---- the mask margin ---------------------------------------------------------------------------------------------------------------
# A kernel evaluates pre = ((y - mean) invstd) gamma + beta in float32 from float32 y, mean, invstd, gamma, beta: a subtraction, two
# products and a sum, each rounding its result by at most u = 2^-24 relative.  The three roundings in front of the final sum move
# gamma xhat by <= 3 u |gamma xhat| (first order), the sum rounds by u |gamma xhat + beta|: |pre_fp32 - pre_fp64| <= 4 u (|gamma xhat|
# + |beta|) (a fused multiply-add only removes roundings).  The builders keep |gamma| <= GAMMA_MAX, |beta| <= BETA_MAX and the tests
# check |xhat| <= XHAT_MAX on every case, so no float32 evaluation of a pre-activation at least MASK_MARGIN from zero in float64 can
# land on the other side of zero.
GAMMA_MAX, BETA_MAX, XHAT_MAX = 2.0, 1.0, 8.0
MASK_MARGIN = 4 * U * (GAMMA_MAX * XHAT_MAX + BETA_MAX)     # 4.1e-6
MOVE_TO = 4 * MASK_MARGIN   # where a moved element lands: rounding the shifted y to float32 moves pre by u |y| gamma invstd << 3 margins
DEAD = 5                    # the dead channel of layer p: gamma 0.01, beta -0.5 -> pre in [-0.56, -0.44], ReLU output 0 everywhere


def _f(t):
    return t.to(f64)


# ---- references --------------------------------------------------------------------------------------------------------------------
def layer_forward_reference(x, w, sums_in, gamma_p, beta_p, conv_bias, eps, momentum, running_mean, running_var, num_batches_tracked=0):
    """x (rows, k), w (n, k), sums_in (2 k) = [sum x | sum x^2] float64.  Everything in float64; returns a dict."""
    x, w, sums_in, gamma_p, beta_p = _f(x), _f(w), _f(sums_in), _f(gamma_p), _f(beta_p)
    R, k = x.shape
    mean = sums_in[:k] / R
    var = (sums_in[k:] / R - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    res = {"mean": mean, "var": var, "invstd": invstd}
    bm = mean + (_f(conv_bias) if conv_bias is not None else 0.0)       # the GEMM output excludes the bias: it only shifts the mean
    unbiased = var * (R / (R - 1.0)) if R > 1 else var
    res["running_mean"] = (1 - momentum) * _f(running_mean) + momentum * bm
    res["running_var"] = (1 - momentum) * _f(running_var) + momentum * unbiased
    res["num_batches_tracked"] = num_batches_tracked + 1
    pre = (x - mean) * invstd * gamma_p + beta_p
    h = pre.clamp_min(0.0)
    y = h @ w.t()
    res.update(pre=pre, h=h, y=y, sums_out=torch.cat([y.sum(0), (y * y).sum(0)]))
    # floors: a length-k dot product per element of y; the column sums inherit the elements' floors (first order)
    ey = k * U * (h @ w.abs().t())
    res["F"] = {"y": float(ey.max()) + 1e-30, "sum_y": ey.sum(0) + 1e-30, "sum_y2": (2 * y.abs() * ey).sum(0) + 1e-30}
    return res


def route(dh, arg, kmax):
    """dh, arg (G, n) -> (G kmax, n) float64: dh[grp, c] in row arg[grp, c] of group grp, zeros elsewhere."""
    G, n = dh.shape
    g = torch.zeros(G, kmax, n, dtype=f64)
    g.scatter_(1, arg.long().unsqueeze(1), _f(dh).unsqueeze(1))
    return g.view(G * kmax, n)


def layer_backward_reference(gmode, gsrc, arg, kmax, yi, mean_i, invstd_i, gamma_i, beta_i, w, yp, mean_p, invstd_p, gamma_p, beta_p,
                             sums_bwd_i=None):
    """gsrc: gmode 0 the stored masked g_i (rows, n); 1 dh_i (rows, n); 2 d(max over kmax rows) (rows / kmax, n) with arg likewise.
    sums_bwd_i (2 n) float64 or None (then the complete sums of this g).  Everything in float64; returns a dict."""
    yi, yp, w = _f(yi), _f(yp), _f(w)
    R, n = yi.shape
    k = yp.shape[1]
    xi = (yi - _f(mean_i)) * _f(invstd_i)
    pre_i = xi * _f(gamma_i) + _f(beta_i)
    if gmode == 0:
        g = _f(gsrc)
    elif gmode == 1:
        g = _f(gsrc) * (pre_i > 0)
    else:
        g = route(gsrc, arg, kmax) * (pre_i > 0)
    own = torch.cat([g.sum(0), (g * xi).sum(0)])
    s = own if sums_bwd_i is None else _f(sums_bwd_i)
    dy = _f(gamma_i) * _f(invstd_i) * (g - s[:n] / R - xi * (s[n:] / R))
    xp = (yp - _f(mean_p)) * _f(invstd_p)
    pre_p = xp * _f(gamma_p) + _f(beta_p)
    mask_p = pre_p > 0
    raw = dy @ w
    gp = raw * mask_p
    h = pre_p.clamp_min(0.0)
    dw = dy.t() @ h
    res = {"xhat_i": xi, "pre_i": pre_i, "g": g, "own_sums": own, "dy": dy, "xhat_p": xp, "pre_p": pre_p, "mask_p": mask_p, "raw": raw,
           "gp": gp, "sums_bwd_p": torch.cat([gp.sum(0), (gp * xp).sum(0)]), "dw": dw, "dgamma": s[n:].clone(), "dbeta": s[:n].clone()}
    # floors: gp a length-n product, dW a length-rows one; the sums of layer p inherit the floors of the elements they add (the
    # kernels' own fp32 partial sums, at most a few adds per thread and tile, stay below them: |g_p| <= (|dY| |w|) and adds < n)
    eg = n * U * (dy.abs() @ w.abs())
    res["F"] = {"gp": float(eg.max()) + 1e-30, "dw": float(R * U * (dy.abs().t() @ h).max()) + 1e-30,
                "sum_g": (eg * mask_p).sum(0) + 1e-30, "sum_gx": (eg * mask_p * xp.abs()).sum(0) + 1e-30,
                # (float) of a float64 sum: one rounding; summing REP float64 copies: 1e-15 of the terms
                "dgamma": 2 * U * s[n:].abs() + 1e-15 * (g * xi).abs().sum(0) + 1e-30,
                "dbeta": 2 * U * s[:n].abs() + 1e-15 * g.abs().sum(0) + 1e-30}
    return res


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def plan(C):
    """|mean| / std <= 2 per channel (the mild plan of test_gpu_train_fp64.test_bn_relu_shapes)."""
    return [((-1.0) ** c * 0.5 * (c % 3), 0.5 + (c % 4)) for c in range(C)]


def affine(C, gen, dead=()):
    """gamma in [0.5, GAMMA_MAX] (either sign would do; positive like a trained BatchNorm), 0.05 <= |beta| <= 0.6."""
    gamma = (1 + 0.3 * torch.randn(C, generator=gen)).clamp(0.5, GAMMA_MAX)
    b = 0.2 * torch.randn(C, generator=gen)
    beta = torch.where(b >= 0, 1.0, -1.0) * (0.05 + b.abs()).clamp(max=0.6)
    for c in dead:
        gamma[c], beta[c] = 0.01, -0.5
    return gamma, beta


def stats32(y, eps=EPS):
    """Batch mean / invstd of the float32 data, formed in float64 (two-pass) and rounded ONCE to float32, and the float64 sums."""
    y = _f(y)
    R = y.shape[0]
    mean = y.sum(0) / R
    var = ((y - mean) ** 2).sum(0) / R
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float(), torch.cat([y.sum(0), (y * y).sum(0)])


def pre_activation(y, mean32, invstd32, gamma, beta):
    """float64 pre-activation from the float32-rounded statistics: what decides a mask."""
    return (_f(y) - _f(mean32)) * _f(invstd32) * _f(gamma) + _f(beta)


def clear_kinks(y, mean32, invstd32, gamma, beta):
    """Moves every element whose pre-activation lies within MASK_MARGIN of zero to +-MOVE_TO (its own side) by shifting that y
    entry; the statistics stay as given (a handful of shifts of ~1e-5 do not move them by a float32 rounding).  Decided from the
    float64 pre-activation alone, in one pass.  Returns (y, number moved)."""
    pre = pre_activation(y, mean32, invstd32, gamma, beta)
    near = pre.abs() < MASK_MARGIN
    target = torch.where(pre >= 0, MOVE_TO, -MOVE_TO)
    ynew = _f(mean32) + (target - _f(beta)) / (_f(gamma) * _f(invstd32))
    return torch.where(near, ynew.float(), y), int(near.sum())


def split_sums(total, ld, parts):
    """The REP-copy layout of a fp64 accumulator: (REP, 2, ld) flattened, copy r holding parts[r] ((REP, 2 c) summing to total up to
    float64 rounding) in its first c columns of each half."""
    c = total.numel() // 2
    out = torch.zeros(REP, 2, ld, dtype=f64)
    out[:, 0, :c], out[:, 1, :c] = parts[:, :c], parts[:, c:]
    return out.reshape(-1)


def forward_case(rows, k, n, seed):
    gen = torch.Generator().manual_seed(seed)
    x = T.plan_inputs(rows, plan(k), seed)
    gamma, beta = affine(k, gen, dead=(DEAD,))
    _, _, sums = stats32(x)
    c = {"rows": rows, "k": k, "n": n, "x": x, "w": torch.randn(n, k, generator=gen) / k ** 0.5, "sums_in": sums, "gamma": gamma, "beta": beta,
         "conv_bias": 0.5 * torch.randn(k, generator=gen), "running_mean": torch.randn(k, generator=gen),
         "running_var": 0.5 + torch.rand(k, generator=gen)}
    c["ref"] = layer_forward_reference(x, c["w"], sums, gamma, beta, c["conv_bias"], EPS, MOMENTUM, c["running_mean"], c["running_var"])
    return c


def backward_case(rows, k, n, gmode, kmax=1, seed=0, negative=True):
    """One layer's backward inputs.  Layer p has the dead channel DEAD.  negative: the first group (gmode 2; the first 8 rows
    otherwise) is pushed far below the mean in the even channels of layer i, so that its ReLU mask is 0 there -- only where the
    case has at least four groups (a forced share of the rows above a quarter would just become the new mean)."""
    gen = torch.Generator().manual_seed(seed)
    grp = kmax if gmode == 2 else 8
    negative = negative and rows >= 4 * grp
    yi, yp = T.plan_inputs(rows, plan(n), seed + 1), T.plan_inputs(rows, plan(k), seed + 2)
    if negative:
        pl = plan(n)
        for c in range(0, n, 2):
            yi[:grp, c] = pl[c][0] - 5.0 * pl[c][1] - 0.5 * (yi[:grp, c] - pl[c][0]).abs()
    gi, bi = affine(n, gen)
    gpm, bp = affine(k, gen, dead=(DEAD,))
    # two fixed passes: the statistics are taken again from the moved data (one shift of ~1e-4 among 100 rows moves a mean by more
    # than a float32 rounding), and the second pass moves what those new statistics bring inside the margin (as a rule nothing:
    # the first pass left its elements at four margins, the statistics moved by ~1e-7) -- so the given statistics are the data's
    mi, isi, _ = stats32(yi)
    mp, isp, _ = stats32(yp)
    yi, moved_i = clear_kinks(yi, mi, isi, gi, bi)
    yp, moved_p = clear_kinks(yp, mp, isp, gpm, bp)
    mi, isi, _ = stats32(yi)
    mp, isp, _ = stats32(yp)
    yi, again_i = clear_kinks(yi, mi, isi, gi, bi)
    yp, again_p = clear_kinks(yp, mp, isp, gpm, bp)
    moved_i, moved_p = moved_i + again_i, moved_p + again_p
    G = rows // kmax if gmode == 2 else rows
    dh = torch.randn(G, n, generator=gen)
    arg = torch.randint(0, kmax, (G, n), generator=gen, dtype=torch.int32) if gmode == 2 else None
    pre_i = pre_activation(yi, mi, isi, gi, bi)
    gsrc = (dh * (pre_i > 0)).float() if gmode == 0 else dh        # gmode 0: the stored, pre-masked gradient (exact in float32)
    w = torch.randn(n, k, generator=gen) / n ** 0.5
    ref = layer_backward_reference(gmode, gsrc, arg, kmax, yi, mi, isi, gi, bi, w, yp, mp, isp, gpm, bp)
    g, xi = ref["g"], ref["xhat_i"]
    parts = torch.stack([torch.cat([g[r::REP].sum(0), (g[r::REP] * xi[r::REP]).sum(0)]) for r in range(REP)])   # copy r: rows r, r + REP, ..
    return {"rows": rows, "k": k, "n": n, "gmode": gmode, "kmax": kmax, "yi": yi, "yp": yp, "mean_i": mi, "invstd_i": isi, "gamma_i": gi,
            "beta_i": bi, "mean_p": mp, "invstd_p": isp, "gamma_p": gpm, "beta_p": bp, "gsrc": gsrc, "arg": arg, "w": w, "sums_parts": parts,
            "moved": (moved_i, moved_p), "negative": grp if negative else 0, "ref": ref}


def straddling_groups(rows, kmax, tile=64):
    """Number of groups of kmax consecutive rows that lie in two tiles."""
    return sum(1 for g0 in range(0, rows, kmax) if g0 // tile != (g0 + kmax - 1) // tile)


# ---- case lists --------------------------------------------------------------------------------------------------------------------
FWD_K, FWD_N, FWD_ROWS = (32, 96, 512), (32, 64, 192, 384), (1, 127, 128, 129, 4000)
# pn2x_tg_fwd (BM = 128 rows per tile, reduction chunk 32): (rows, k, n, padded)
FWD_CASES = [(129, k, n, True) for k in FWD_K for n in FWD_N]   # every (k, n): 1 / 3 / 16 chunks x column tiles 32 / 64 / 64 x 3 / 128 x 3; one row past a tile
FWD_CASES += [
    (1, 32, 32, False),      # a single row (variance 0, R - 1 = 0), one chunk: the weight tile stays resident
    (1, 512, 384, True),     # a single row, 16 chunks, three column groups
    (127, 96, 64, True),     # BM - 1: one ragged tile
    (127, 32, 384, False),
    (128, 96, 192, False),   # exactly one full tile (the unguarded store)
    (128, 512, 32, True),
    (4000, 32, 64, True),    # 32 tiles, the last one ragged (4000 = 31 x 128 + 32), single chunk
    (4000, 96, 384, False),  # 32 tiles x three column groups
    (4000, 512, 192, True),  # 32 tiles x 16 chunks
    (127, 512, 192, False), (128, 32, 64, True), (1, 96, 192, True),
]
FWD2_K, FWD2_N, FWD2_ROWS = (64, 128, 256), (32, 64, 128, 192, 256, 384, 512), (1, 63, 65, 64 * 5 + 17)
# what pn2x_tg_fwd2_supported is expected to accept among FWD2_K x FWD2_N (asserted against the entry by the GPU test)
FWD2_SUPPORTED = [(k, n) for k in FWD2_K for n in FWD2_N if n != 32]
FWD2_PAIRS = [(128, 128, 1, 64 * 5 + 17), (128, 192, 65, 1), (128, 192, 63, 64 * 5 + 17)]   # (k, n, rows a, rows b): 1 row against many, both orders

# pn2x_tg_bwd_slice: the instantiated (k, n) of tg_bwd; tg_bwd2 (variant 1) serves BWD2_SHAPES of them
BWD_SHAPES = [(32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (128, 192)]
BWD2_SHAPES = [(64, 64), (64, 128), (128, 128), (128, 192)]
BWD_ROWS = (64 * 3 + 5, 1)   # gmode 2 at 197 rows: ONE group of kmax = 197 (a prime: the division branch, a group over four tiles)
BWD_LARGEST = (128, 192)     # the largest shape of either variant
# the reduced set on BWD_LARGEST: name -> (rows, gmode, kmax, options)
BWD_REDUCED = {
    "rows63_routed3": (63, 2, 3, {}),            # one ragged tile; kmax 3: division branch
    "rows63_masked": (63, 0, 1, {}),             # one ragged tile, stored gradient
    "rows64_routed16": (64, 2, 16, {}),          # exactly one tile; kmax 16: shift branch
    "rows65_dense": (65, 1, 1, {}),              # one row into the second tile
    "rows240_routed24": (240, 2, 24, {}),        # kmax 24: division branch, groups 2 (rows 48..71) and 7 (168..191) straddle tiles
    "rows195_routed3": (195, 2, 3, {}),          # kmax 3: groups 21, 42 straddle; ragged last tile
    "rows208_routed16": (208, 2, 16, {}),        # shift branch, ragged last tile of 16 rows
    "ldarg": (240, 2, 24, {"wide_g": 16}),       # g a column block of a gradient 16 columns wider, arg contiguous: ldarg != ldg
    "padded": (197, 1, 1, {"pad": (4, 8, 12, 4)}),   # ldyi, ldyp, ldgp, ldw beyond the widths
    "padded_routed": (208, 2, 16, {"pad": (8, 4, 4, 12), "wide_g": 8}),
    "persistent": (0, 1, 1, {"persistent": True}),  # more tiles than workgroups + a ragged tail (rows from pn2x_tg_bwd_partials)
}
# slice chaining: (k, n whole, slice width, rows, gmode, kmax)
CHAIN_CASES = [(128, 384, 192, 197, 1, 1), (128, 384, 192, 208, 2, 16), (128, 512, 128, 197, 0, 1), (128, 512, 128, 240, 2, 24)]
# pair launches: (k, n); rows (a, b) per gmode (gmode 2: kmax 1 for the single row, 16 for 208 rows)
PAIR_SHAPES = [(128, 128), (128, 192)]
PAIR_ROWS = (1, 208)
PAIR_NO_KERNEL = (64, 128)
# the two-kernel route: (kd = channels of layer i, n = channels of layer p) as pn2x_tg_dgrad names them
TWO_KERNEL_SHAPES = [(32, 32), (192, 128), (256, 256), (384, 128), (512, 96)]
TWO_KERNEL_ROWS = (1, 127, 129, 128 * 4 + 33)
# (bit-equality of two reductions, and of a run with its repeat, holds while pn2x_tg_reduce_multi cuts a layer's P partial tiles
# into at most two slices, P < 384: the slices are added to dW by fp32 atomics, and three or more land in any order.  Every row
# count here writes at most 72 tiles; a larger case would have to compare dW under the bound instead)
# gmode 2 needs rows % kmax == 0 (the entries refuse anything else) and 127, 129, 545 have no factor 16 or 24: the routed cases
# take the multiples of kmax next to those edges -- below BM, above BM, a ragged fifth tile -- and kmax 1 at one row
TWO_KERNEL_ROUTED = [(1, 1), (112, 16), (120, 24), (144, 16), (144, 24), (544, 16), (552, 24)]   # (rows, kmax)
PERSISTENT_NOMINAL_ROWS = (256 + 1) * 64 + 17   # 256 persistent workgroups (one per compute unit at BWD_LARGEST) + one tile + a ragged tail


def case_seed(rows, k, n, gmode, kmax):
    return 7 * rows + 3 * k + n + 1000 * gmode + 31 * kmax


def backward_specs():
    """(entry, rows, k, n, gmode, kmax) of every backward case the GPU test builds (the persistent case at its nominal row count)."""
    out = []
    for (k, n) in BWD_SHAPES:
        for gmode in (0, 1, 2):
            for rows in BWD_ROWS:
                out.append(("bwd_slice", rows, k, n, gmode, rows if gmode == 2 else 1))
    for name, (rows, gmode, kmax, opt) in BWD_REDUCED.items():
        out.append(("bwd_slice " + name, rows or PERSISTENT_NOMINAL_ROWS, BWD_LARGEST[0], BWD_LARGEST[1], gmode, kmax))
    for (k, n, wd, rows, gmode, kmax) in CHAIN_CASES:
        out.append(("bwd_slice chain", rows, k, n, gmode, kmax))
    for (k, n) in PAIR_SHAPES + [PAIR_NO_KERNEL]:
        for gmode in (0, 1, 2):
            for rows in PAIR_ROWS:
                out.append(("bwd_slice pair", rows, k, n, gmode, (1 if rows == 1 else 16) if gmode == 2 else 1))
    for (kd, n) in TWO_KERNEL_SHAPES:
        for gmode in (0, 1):
            for rows in TWO_KERNEL_ROWS:
                out.append(("dgrad/wgrad", rows, n, kd, gmode, 1))
        for rows, kmax in TWO_KERNEL_ROUTED:
            out.append(("dgrad/wgrad", rows, n, kd, 2, kmax))
    return out


_CASES = {}


def cached_backward_case(rows, k, n, gmode, kmax):
    """backward_case at case_seed, built once per process and shared (never modified) by the tests that need it."""
    key = (rows, k, n, gmode, kmax)
    if key not in _CASES:
        _CASES[key] = backward_case(rows, k, n, gmode, kmax, seed=case_seed(*key))
    return _CASES[key]
