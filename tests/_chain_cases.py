"""Inputs, weights and plain float64 references for the tests of the fp32-MFMA chains over their whole accepted range
(pn2x_row_chain / pn2x_row_lists in hotrack_amd/csrc/row_chain.hip, pn2x_sa3_chain / pn2x_fp3_chain in mid_chain.hip, the shared
k-loop in mfma_rows.h).  Nothing here needs a GPU: every generator returns CPU tensors and every reference is a few lines of
torch that run on whatever device their arguments live on.  tests/test_chain_cases.py checks the generators' own conditions on
the CPU; tests/test_gpu_chain_range.py runs the kernels against them.

Layer shapes (fixed by the kernels):
  row chain   x[:131] -> 128 -> 128 -> 384 -> 512   wa ba wb bb wc bc wq   (ReLU after the first three, no bias on wq)
  sa3         x[:131] -> 128 -> 128 -> 512          three (W, b) pairs, ReLU after each, then the max over each 32-row tile
  fp3         relu(Wf relu(Wa x[:128] + Wg l3 + bg) + bf), 128 / 512 -> 256 -> 256
"""
import functools

import torch

F64 = torch.float64
TILE = 32                      # rows per tile of the mid chains
ROW_K = (144, 128, 128, 384)   # dot-product lengths of the row chain's layers as the kernel runs them (layer 1 zero-padded)
SA3_K = (144, 128, 128)
U = 2.0 ** -24                 # unit roundoff of float32


# ---- plain float64 references ---------------------------------------------------------------------------------------------
def row_chain_layers(x, W):
    """[pre1, pre2, pre3, out] of the row chain in float64: the three pre-activations and the final product (..., 512)."""
    wa, ba, wb, bb, wc, bc, wq = (t.to(F64) for t in W)
    p1 = x[..., :131].to(F64) @ wa.t() + ba
    p2 = torch.relu(p1) @ wb.t() + bb
    p3 = torch.relu(p2) @ wc.t() + bc
    return [p1, p2, p3, torch.relu(p3) @ wq.t()]


def row_chain_ref(x, W):
    return row_chain_layers(x, W)[3]


def sa3_layers(x, sa3):
    """The three pre-activations of sa3 in float64, per row."""
    h, pre = x[..., :131].to(F64), []
    for Wl, bl in sa3:
        pre.append(h @ Wl.to(F64).t() + bl.to(F64))
        h = torch.relu(pre[-1])
    return pre


def sa3_part_ref(x, sa3):
    """(B, S/32, 512) float64: the per-tile maxima of sa3's output."""
    y = torch.relu(sa3_layers(x, sa3)[2])
    B, S, C = y.shape
    return y.view(B, S // TILE, TILE, C).amax(dim=2)


def fp3_layers(x, l3, fp3):
    """[g, pre1, pre2] of fp3 in float64 for l3 (B, 512): the per-cloud term and both pre-activations."""
    wg, bg, wa, wf, bf = (t.to(F64) for t in fp3)
    g = l3.to(F64) @ wg.t() + bg
    p1 = x[..., :128].to(F64) @ wa.t() + g[:, None, :]
    return [g, p1, torch.relu(p1) @ wf.t() + bf]


def fp3_ref(x, l3, fp3):
    return torch.relu(fp3_layers(x, l3, fp3)[2])


# ---- dense random weights and inputs (the recipes of tests/test_gpu_row_chain_bits.py, on the CPU) ---------------------------
@functools.lru_cache(maxsize=None)
def row_weights(seed=11):
    g = torch.Generator().manual_seed(seed)

    def lin(o, i, s):
        return torch.randn(o, i, generator=g) * s, torch.randn(o, generator=g) * 0.1
    wa, ba = lin(128, 131, 0.1)
    wb, bb = lin(128, 128, 0.1)
    wc, bc = lin(384, 128, 0.1)
    return wa, ba, wb, bb, wc, bc, torch.randn(512, 384, generator=g) * 0.05


@functools.lru_cache(maxsize=None)
def mid_weights(seed=23):
    """-> (sa3, fp3): three (W, b) pairs and (wg, bg, wa, wf, bf), BatchNorm-folded-like scales."""
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        scale = 0.5 + torch.rand(o, 1, generator=g)
        return torch.randn(o, i, generator=g) / i ** 0.5 * scale, torch.randn(o, generator=g) * 0.1
    sa3 = (lin(128, 131), lin(128, 128), lin(512, 128))
    wg, bg = lin(256, 512)
    wa, _ = lin(256, 128)
    wf, bf = lin(256, 256)
    return sa3, (wg, bg, wa, wf, bf)


def random_rows(B, N, seed):
    """(B, N, 132) standard-normal rows; the pad float, column 131, is NaN: the kernels never read it."""
    x = torch.randn(B, N, 132, generator=torch.Generator().manual_seed(seed))
    x[:, :, 131] = float("nan")
    return x


# ---- A: exact-integer probes ----------------------------------------------------------------------------------------------
def int_linear(n_out, k, bias=True, positive=False):
    """Sparse integer layer.  Output channel c reads the 2 + c % 3 inputs (7 c + j (37 + 4 (c // k))) % k, j = 0, 1, ..., with
    weights +1, then -1 / +1 by a pattern of c and j: no two channels of a layer read the same set, so a swapped channel, n-tile
    or k-group changes the result.  Biases are (3 c) % 5 - 2.  positive: 1 + c % 2 inputs, all with weight +1."""
    W = torch.zeros(n_out, k)
    for c in range(n_out):
        off = 37 + 4 * (c // k)
        for j in range(1 + c % 2 if positive else 2 + c % 3):
            W[c, (7 * c + j * off) % k] = 1.0 if positive or j == 0 or (c // 3 + j) % 2 else -1.0
    b = ((3 * torch.arange(n_out)) % 5 - 2).float() if bias else None
    return W, b


@functools.lru_cache(maxsize=None)
def int_row_weights():
    wa, ba = int_linear(128, 131)
    wb, bb = int_linear(128, 128)
    wc, bc = int_linear(384, 128)
    return wa, ba, wb, bb, wc, bc, int_linear(512, 384, bias=False)[0]


@functools.lru_cache(maxsize=None)
def int_mid_weights():
    sa3 = (int_linear(128, 131), int_linear(128, 128), int_linear(512, 128))
    # l3 is a maximum over rows, some tens, and Wg l3 is the same on every row of a cloud: with signed Wg and Wf it pushes a few
    # channels of fp3 below zero on every row, and dead channels are identical channels.  Positive weights keep each channel
    # alive; channels that read small entries still reach 0 and -1 before the ReLU (the signed case is Wa's and sa3's).
    wg, bg = int_linear(256, 512, positive=True)
    wf, bf = int_linear(256, 256, positive=True)
    return sa3, (wg, bg, int_linear(256, 128, bias=False)[0], wf, bf)


ROW_ID_COL = 3  # the column of int_rows that carries the row's index inside its cloud
INT_ROW_CASE = (3, 64, 5)  # (B, N, seed) of the row chain's probe; its lists: INT_ROW_PAIRS
INT_ROW_PAIRS = ((17, 47), (0, 0), (64, 0))
INT_MID_CASE = (2, 64, 7)  # (B, S, seed) of the mid chains' probe: a seed at which the four partial maxima tell all 512 channels apart


def int_rows(B, N, seed):
    """(B, N, 132) integers in [-8, 8]; column ROW_ID_COL holds the row's index in its cloud (a row permutation inside a tile
    shows), row 0 of cloud 0 is all zero (its layer-1 pre-activation is the bias: 0 and -1 among others), column 131 is NaN."""
    x = torch.randint(-8, 9, (B, N, 132), generator=torch.Generator().manual_seed(seed)).float()
    x[:, :, ROW_ID_COL] = torch.arange(N).float()
    x[0, 0] = 0.0
    x[:, :, 131] = float("nan")
    return x


# ---- row lists ------------------------------------------------------------------------------------------------------------
def lists(B, N, pairs, seed):
    """Hand-built lists: cloud b names pairs[b] = (small, large-only) distinct points drawn at random, each part ascending.
    -> list (B, N) int32 (-7 past the count), counts (B, 2) int32, mask (B, N, 512) bool of the elements the chain writes."""
    g = torch.Generator().manual_seed(seed)
    lst = torch.full((B, N), -7, dtype=torch.int32)
    counts = torch.zeros((B, 2), dtype=torch.int32)
    rows_s = torch.zeros(B, N, dtype=torch.bool)
    rows_o = torch.zeros(B, N, dtype=torch.bool)
    for b, (ns, nl) in enumerate(pairs):
        if ns + nl == 0:
            continue
        perm = torch.randperm(N, generator=g)
        s, o = perm[:ns].sort().values, perm[ns:ns + nl].sort().values
        lst[b, :ns + nl] = torch.cat([s, o]).int()
        counts[b, 0], counts[b, 1] = ns, ns + nl
        rows_s[b, s] = True
        rows_o[b, o] = True
    mask = torch.zeros(B, N, 512, dtype=torch.bool)
    mask[:, :, :256] = rows_s[:, :, None]
    mask[:, :, 256:] = (rows_s | rows_o)[:, :, None]
    return lst, counts, mask


BATCH_N = 32
BATCH_CYCLE = ((0, 0), (1, 0), (0, 1), (15, 17), (32, 0))
BATCHES = (256, 257, 513, 1024)  # one block of the prefix scan, one cloud into the second, into the third, the limit


def batch_pairs(B, kind):
    """Per-cloud (small, large-only) counts at N = 32.  "cycle": BATCH_CYCLE repeated, clouds 255 and 256 -- the two sides of the
    prefix scan's first block boundary -- empty.  "last": only the last cloud has rows, one of each kind."""
    if kind == "last":
        return [(0, 0)] * (B - 1) + [(1, 1)]
    ps = [BATCH_CYCLE[b % len(BATCH_CYCLE)] for b in range(B)]
    for b in (255, 256):
        if b < B:
            ps[b] = (0, 0)
    return ps


def lists_from_sets(lst_rows, N):
    """One cloud's row_lists output from the index tensors: (small (J, KS), any (J, KL)) -> expected list prefix, counts."""
    gs, ga = lst_rows
    s = torch.unique(gs[(gs >= 0) & (gs < N)])
    a = torch.unique(torch.cat([ga[(ga >= 0) & (ga < N)].flatten(), s]))
    o = a[~torch.isin(a, s)]
    return torch.cat([s, o]).int(), (int(s.numel()), int(s.numel() + o.numel()))


ROW_LIST_SHAPES = ((2, 21, 1000, 64, 16), (2, 3, 33, 8, 8), (3, 1, 1, 1, 1), (2, 21, 8193, 64, 16), (1, 40, 16384, 200, 7),
                   (2, 5, 100, 7, 3))
OUT_OF_RANGE = lambda N: (-1, N, 2 ** 31 - 1)  # noqa: E731


def hand_indices(B, J, N, KL, KS, kind, seed=0):
    """Hand-made (gi (B,J,KL), gi_small (B,J,KS)) int32 index tensors:
      random   uniform in [0, N)
      all      every point named (needs J * KL >= N); the small lists name the first min(N, J * KS)
      last     only point N - 1 named; first: only point 0
      words    points of bitmap words 255 and 256 only (N = 16384): the boundary between two threads' word ranges
    """
    g = torch.Generator().manual_seed(1000 * N + 7 * KL + seed)
    if kind == "random":
        gi = torch.randint(0, N, (B, J, KL), generator=g)
        gs = torch.randint(0, N, (B, J, KS), generator=g)
    elif kind == "all":
        assert J * KL >= N
        gi = (torch.arange(J * KL) % N).view(1, J, KL).expand(B, J, KL).clone()
        gs = (torch.arange(J * KS) % N).view(1, J, KS).expand(B, J, KS).clone()
    elif kind in ("last", "first"):
        v = N - 1 if kind == "last" else 0
        gi, gs = torch.full((B, J, KL), v), torch.full((B, J, KS), v)
    elif kind == "words":
        assert N >= 257 * 32
        gi = 255 * 32 + torch.randint(0, 64, (B, J, KL), generator=g)
        gs = 255 * 32 + 16 + torch.randint(0, 32, (B, J, KS), generator=g)
    else:
        raise KeyError(kind)
    return gi.int(), gs.int()


def with_out_of_range(t, N, seed):
    """-> (dirty, clean): every fifth entry of a cloud (from entry 2 + seed % 3 on, so never the first) replaced by the
    out-of-range values -1, N and 2**31 - 1 in turn in `dirty`, and by the cloud's first entry -- a point the cloud names anyway
    -- in `clean`.  A kernel that ignores out-of-range entries gives the same lists for both."""
    B = t.shape[0]
    flat = t.reshape(B, -1).clone()
    i = torch.arange(flat.shape[1])
    hit = ((i % 5) == 2 + seed % 3)[None].expand_as(flat)
    junk = torch.tensor(OUT_OF_RANGE(N), dtype=torch.int64)[(i // 5) % 3].int()[None].expand_as(flat)
    dirty = torch.where(hit, junk, flat)
    clean = torch.where(hit, flat[:, :1].expand_as(flat), flat)
    return dirty.view(t.shape), clean.view(t.shape)


# ---- D: mid chains at other S -----------------------------------------------------------------------------------------------
MID_SHAPES = ((32, 1), (32, 5), (64, 1), (64, 5), (96, 1), (96, 5), (256, 1), (256, 5), (1024, 1))  # (S, B)
MID_S = (32, 64, 96, 256, 1024)


def tile_scaled_rows(S, seed=77):
    """(S / 32, S, 132): cloud t is one random cloud with the rows of its tile t scaled by 3, so cloud t's maximum comes from the
    partial maximum of tile t for most channels (checked in float64 by tests/test_chain_cases.py)."""
    base = random_rows(1, S, seed + S)[0]
    x = base[None].repeat(S // TILE, 1, 1)
    for t in range(S // TILE):
        x[t, t * TILE:(t + 1) * TILE, :131] *= 3.0
    return x


# ---- F: ill-scaled rows and the first-order forward error bound -------------------------------------------------------------
def ill_scaled_rows(B, N, seed):
    """Feature columns ~1e3 in the rows with index % 4 == 0, ~1e-3 where it is 1, ~1 elsewhere; signs random, so sums cancel."""
    x = random_rows(B, N, seed)
    r = torch.arange(N)
    x[:, r % 4 == 0, :128] *= 1e3
    x[:, r % 4 == 1, :128] *= 1e-3
    return x


def forward_bound(x, layers, K):
    """First-order forward error bound of a float32 layer chain, propagated in float64 beside the reference:
        e_0 = 0 (the inputs are float32 already),
        e_{l+1} = |W_l| e_l + (K_l + 1) u (|W_l| |h_l| + |b_l|),      u = 2^-24,
    with h_l the float64 activations: a length-K dot product plus the bias add commits at most (K + 1) u relative to the sum
    of magnitudes in any summation order, and ReLU is 1-Lipschitz, so an activation's error is at most its pre-activation's.
    layers: (W, b or None, relu) triples.  -> (reference output, e_final), float64."""
    h = x[..., :131].to(F64)
    e = torch.zeros_like(h)
    for (Wl, bl, relu), k in zip(layers, K):
        Wd = Wl.to(F64)
        mag = h.abs() @ Wd.abs().t()
        pre = h @ Wd.t()
        if bl is not None:
            mag = mag + bl.to(F64).abs()
            pre = pre + bl.to(F64)
        e = e @ Wd.abs().t() + (k + 1) * U * mag
        h = torch.relu(pre) if relu else pre
    return h, e


def row_chain_bound(x, W):
    wa, ba, wb, bb, wc, bc, wq = W
    return forward_bound(x, ((wa, ba, True), (wb, bb, True), (wc, bc, True), (wq, None, False)), ROW_K)


def sa3_part_bound(x, sa3):
    """Per-tile maxima and their bound: the maximum over a tile's rows moves by at most the largest error among them."""
    y, e = forward_bound(x, tuple((Wl, bl, True) for Wl, bl in sa3), SA3_K)
    B, S, C = y.shape
    return y.view(B, S // TILE, TILE, C).amax(dim=2), e.view(B, S // TILE, TILE, C).amax(dim=2)
