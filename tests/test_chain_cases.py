"""CPU: the conditions that the chain tests' generators promise (tests/_chain_cases.py), checked in float64 from the generators
alone.  tests/test_gpu_chain_range.py leans on every one of them: an exact-integer probe is only exact if every intermediate
is an integer below 2^24, a tile-scaled cloud only picks its partial maximum if the scaled tile wins, and so on."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chain_cases as C  # noqa: E402
from _chain_cases import F64  # noqa: E402


def _is_exact_integer(t, what):
    assert bool((t == t.round()).all()), f"{what}: not an integer"
    assert float(t.abs().max()) < 2 ** 24, f"{what}: |v| reaches 2^24"


def _distinct_channels(t, what):
    """No two channels (last axis) of t agree on every row."""
    cols = t.reshape(-1, t.shape[-1]).t()
    assert torch.unique(cols, dim=0).shape[0] == cols.shape[0], f"{what}: two identical channels"


def _relu_boundary(pre, what):
    assert bool((pre == 0).any()) and bool((pre == -1).any()), f"{what}: no pre-activation of exactly 0 and exactly -1"


@pytest.mark.parametrize("n_out,k", [(128, 131), (128, 128), (384, 128), (512, 384), (512, 128), (256, 512), (256, 256), (256, 128)])
def test_integer_layers_are_sparse_signed_and_distinct(n_out, k):
    positive = k in (512, 256)  # fp3's Wg and Wf
    W, b = C.int_linear(n_out, k, positive=positive)
    assert set(W.unique().tolist()) == ({0.0, 1.0} if positive else {-1.0, 0.0, 1.0})
    nnz = (W != 0).sum(1)
    assert int(nnz.min()) >= 1 and int(nnz.max()) <= 4
    assert torch.unique(W != 0, dim=0).shape[0] == n_out  # every channel reads another input set
    assert bool((b == b.round()).all()) and float(b.abs().max()) <= 2 and {0.0, -1.0} <= set(b.tolist())
    if k == 131:  # layer 1: the three coordinate columns, and every one of the nine k-groups of 16 (the last one is 128..130)
        used = (W != 0).any(0)
        assert bool(used[128]) and bool(used[129]) and bool(used[130])
        assert all(bool(used[16 * kg:16 * kg + 16].any()) for kg in range(9))


def test_integer_row_chain_probe_is_exact_in_float32():
    x = C.int_rows(*C.INT_ROW_CASE)
    assert bool(x[:, :, 131].isnan().all()) and not bool(x[:, :, :131].isnan().any())
    body = torch.cat([x[:, :, :C.ROW_ID_COL], x[:, :, C.ROW_ID_COL + 1:131]], 2)
    assert float(body.abs().max()) <= 8 and bool((x[:, :, C.ROW_ID_COL] == torch.arange(64.0)).all())
    pre = C.row_chain_layers(x, C.int_row_weights())
    for l, p in enumerate(pre):
        _is_exact_integer(p, f"row chain layer {l + 1}")
        _distinct_channels(torch.relu(p) if l < 3 else p, f"row chain layer {l + 1}")
        if l < 3:
            _relu_boundary(p, f"row chain layer {l + 1}")
    # every partial sum is bounded by the sum of magnitudes, itself an integer below 2^24: exact in any summation order
    W = C.int_row_weights()
    h = x[..., :131].abs().to(F64)
    for Wl, bl in ((W[0], W[1]), (W[2], W[3]), (W[4], W[5]), (W[6], None)):
        h = h @ Wl.abs().to(F64).t() + (bl.abs().to(F64) if bl is not None else 0)
        assert float(h.max()) < 2 ** 24


def test_integer_mid_chain_probe_is_exact_in_float32():
    x = C.int_rows(*C.INT_MID_CASE)
    sa3, fp3 = C.int_mid_weights()
    pre = C.sa3_layers(x, sa3)
    for l, p in enumerate(pre):
        _is_exact_integer(p, f"sa3 layer {l + 1}")
        _distinct_channels(torch.relu(p), f"sa3 layer {l + 1}")
        _relu_boundary(p, f"sa3 layer {l + 1}")
    part = C.sa3_part_ref(x, sa3)
    _is_exact_integer(part, "sa3 part")
    _distinct_channels(part, "sa3 part")
    g, p1, p2 = C.fp3_layers(x, part.amax(1), fp3)
    for what, p in (("fp3 per-cloud term", g), ("fp3 layer 1", p1), ("fp3 layer 2", p2)):
        _is_exact_integer(p, what)
    _distinct_channels(torch.relu(p1), "fp3 layer 1")
    _distinct_channels(torch.relu(p2), "fp3 layer 2")
    _relu_boundary(p1, "fp3 layer 1")
    _relu_boundary(p2, "fp3 layer 2")
    # sums of magnitudes: every partial sum of every layer, in any order, is an integer below 2^24
    h = x[..., :131].abs().to(F64)
    for Wl, bl in sa3:
        h = h @ Wl.abs().to(F64).t() + bl.abs().to(F64)
    assert float(h.max()) < 2 ** 24
    wg, bg, wa, wf, bf = (t.abs().to(F64) for t in fp3)
    gm = part.amax(1).abs() @ wg.t() + bg
    hm = (x[..., :128].abs().to(F64) @ wa.t() + gm[:, None, :]) @ wf.t() + bf
    assert float(hm.max()) < 2 ** 24


@pytest.mark.parametrize("B", C.BATCHES)
def test_batch_lists_cover_the_cycle_and_the_scan_boundary(B):
    ps = C.batch_pairs(B, "cycle")
    assert len(ps) == B and set(C.BATCH_CYCLE) <= set(ps) and all(s + o <= C.BATCH_N for s, o in ps)
    assert all(ps[b] == (0, 0) for b in (255, 256) if b < B)
    assert sum(s for s, _ in ps[:256]) > 0 and sum(o for _, o in ps[:256]) > 0  # what both scans carry into block 2 is not zero
    assert B <= 257 or (any(s for s, _ in ps[257:]) and any(o for _, o in ps[257:]))  # and rows of both kinds lie beyond it
    lst, counts, mask = C.lists(B, C.BATCH_N, ps, B)
    assert counts.tolist() == [[s, s + o] for s, o in ps]
    for b in (0, 1, 2, 3, 4, B - 1):
        s, a = int(counts[b, 0]), int(counts[b, 1])
        rows = lst[b, :a].long()
        assert rows.unique().numel() == a and bool((lst[b, a:] == -7).all())
        assert bool(mask[b, rows[:s]].all()) and bool(mask[b, rows[s:], 256:].all()) and not bool(mask[b, rows[s:], :256].any())
        assert int(mask[b].sum()) == 512 * s + 256 * (a - s)
    last = C.batch_pairs(B, "last")
    assert last[-1] == (1, 1) and set(last[:-1]) == {(0, 0)}


@pytest.mark.parametrize("shape", C.ROW_LIST_SHAPES, ids=str)
def test_hand_made_index_tensors_name_what_they_say(shape):
    B, J, N, KL, KS = shape
    kinds = ["random", "last", "first"] + (["all"] if J * KL >= N else []) + (["words"] if N == 16384 else [])
    for kind in kinds:
        gi, gs = C.hand_indices(B, J, N, KL, KS, kind)
        assert gi.shape == (B, J, KL) and gs.shape == (B, J, KS) and gi.dtype == gs.dtype == torch.int32
        assert int(gi.min()) >= 0 and int(gi.max()) < N and int(gs.min()) >= 0 and int(gs.max()) < N
        want, (ns, na) = C.lists_from_sets((gs[0], gi[0]), N)
        if kind == "all":
            assert na == N and torch.equal(want.sort().values, torch.arange(N, dtype=torch.int32))
        elif kind in ("last", "first"):
            assert want.tolist() == [N - 1 if kind == "last" else 0] and (ns, na) == (1, 1)
        elif kind == "words":
            words = set((want // 32).tolist())
            assert words == {255, 256}
    gi, gs = C.hand_indices(B, J, N, KL, KS, "random")
    for t, seed in ((gi, 1), (gs, 2)):
        dirty, clean = C.with_out_of_range(t, N, seed)
        bad = (dirty < 0) | (dirty >= N)
        assert not bool(((clean < 0) | (clean >= N)).any())
        if t[0].numel() >= 15:
            assert {int(v) for v in dirty[bad].unique()} == set(C.OUT_OF_RANGE(N))
        for b in range(B):
            assert torch.equal(torch.unique(dirty[b][~bad[b]]), torch.unique(clean[b]))


@pytest.mark.parametrize("S", C.MID_S)
def test_scaled_tile_wins_its_cloud_in_float64(S):
    sa3, _ = C.mid_weights()
    x = C.tile_scaled_rows(S)
    assert x.shape == (S // C.TILE, S, 132)
    part = C.sa3_part_ref(x, sa3)  # (S/32 clouds, S/32 tiles, 512)
    winner = part.argmax(dim=1)
    for t in range(S // C.TILE):
        unique_max = (part[t] == part[t].amax(0)).sum(0) == 1
        won = (winner[t] == t) & unique_max
        assert int(won.sum()) >= 256, (S, t, int(won.sum()))


def test_ill_scaled_rows_and_bound():
    x = C.ill_scaled_rows(2, 64, 9)
    f = x[:, :, :128].abs()
    assert float(f[:, 0::4].median()) > 1e2 and float(f[:, 1::4].median()) < 1e-2 and 0.1 < float(f[:, 2::4].median()) < 10
    ref, e = C.row_chain_bound(x, C.row_weights())
    assert torch.equal(ref, C.row_chain_ref(x, C.row_weights()))  # the bound's reference is the plain reference
    assert bool((e > 0).all()) and bool(e.isfinite().all())
    # the bound follows the rows' scale: it is a per-element bound, not one tolerance for the whole output
    assert float(e[:, 0::4].median()) > 100 * float(e[:, 1::4].median())
    part, ep = C.sa3_part_bound(x, C.mid_weights()[0])
    assert torch.equal(part, C.sa3_part_ref(x, C.mid_weights()[0])) and bool((ep > 0).all())
