"""GPU: the fp32-MFMA chains over the whole range their entry points accept (pn2x_row_chain / pn2x_row_lists in
hotrack_amd/csrc/row_chain.hip, pn2x_sa3_chain / pn2x_fp3_chain in mid_chain.hip, the shared k-loop in mfma_rows.h), against the
plain float64 references of tests/_chain_cases.py (whose own conditions tests/test_chain_cases.py checks on the CPU):

  A  exact-integer probes: every product and partial sum is an integer below 2^24, so the kernels equal float64 bit for bit
  B  row_chain at 256 .. 1024 clouds (the carried prefix sums), the dynamic-LDS opt-in in a fresh process, the rejections
  C  row strides of x and out other than the contiguous ones
  D  sa3 / fp3 at S other than 128
  E  row_lists at every word count per thread, with out-of-range indices, in prefix mode, and feeding row_chain
  F  ill-scaled rows against a first-order forward error bound instead of a tolerance
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chain_cases as C  # noqa: E402
from test_gpu_row_chain_bits import SENTINEL, _check  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
FILL = -77  # pre-filled into row_lists' output: entries past the count keep it


def _cuda(ts):
    return tuple(t.cuda() for t in ts)


def _pack_row(W):
    from hotrack_amd import ext
    wa, ba, wb, bb, wc, bc, wq = _cuda(W)
    p = ext.row_chain_pack
    return p(wa), ba, p(wb), bb, p(wc), bc, p(wq)


def _pack_mid(sa3, fp3):
    from hotrack_amd import ext
    p = ext.row_chain_pack
    wg, bg, wa, wf, bf = _cuda(fp3)
    return [t for Wl, bl in sa3 for t in (p(Wl.cuda()), bl.cuda())], (wg.t().contiguous(), bg, p(wa), p(wf), bf)


@functools.lru_cache(maxsize=None)
def _row_packed():
    return _pack_row(C.row_weights())


@functools.lru_cache(maxsize=None)
def _mid_packed():
    return _pack_mid(*C.mid_weights())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row_chain(x, lst, counts, packed, grid=0, out=None):
    from hotrack_amd import ext
    if out is None:
        out = torch.full((x.shape[0], x.shape[1], 512), SENTINEL, device="cuda")
    return ext.row_chain(x, lst.cuda(), counts.cuda(), *packed, out=out, grid=grid)


def _mid_close(got, ref, what):
    """The mid chains' existing bound: atol = 2e-5, rtol = 1e-5 against float64 rounded to float32."""
    ref = ref.float()
    err = float((got - ref).abs().max())
    print(f"{what}: max |err| vs fp64 = {err:.3e} (bound 2e-5 + 1e-5 |ref|, |ref|max = {float(ref.abs().max()):.3e})")
    assert torch.allclose(got, ref, atol=2e-5, rtol=1e-5), (what, err)


# ---- A: exact-integer probes of the shared k-loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 7])
def test_row_chain_equals_fp64_bit_for_bit_on_integers(grid):
    B, N, seed = C.INT_ROW_CASE
    x = C.int_rows(B, N, seed)
    W = C.int_row_weights()
    lst, counts, mask = C.lists(B, N, C.INT_ROW_PAIRS, 3)
    out = _row_chain(x.cuda(), lst, counts, _pack_row(W), grid=grid).cpu()
    ref = C.row_chain_ref(x, W).float()
    assert bool((out[~mask] == SENTINEL).all()), "wrote outside the listed rows / columns"
    assert torch.equal(out[mask], ref[mask]), f"{int((out[mask] != ref[mask]).sum())} of {int(mask.sum())} elements differ from fp64"


def test_mid_chains_equal_fp64_bit_for_bit_on_integers():
    from hotrack_amd import ext
    B, S, seed = C.INT_MID_CASE
    x = C.int_rows(B, S, seed)
    sa3, fp3 = C.int_mid_weights()
    sa3_p, fp3_p = _pack_mid(sa3, fp3)
    ref_part = C.sa3_part_ref(x, sa3).float()
    part = ext.sa3_chain(x.cuda(), *sa3_p).cpu()
    assert torch.equal(part, ref_part), f"sa3: {int((part != ref_part).sum())} of {part.numel()} partial maxima differ from fp64"
    ref = C.fp3_ref(x, ref_part.amax(1), fp3).float()
    out = ext.fp3_chain(x.cuda(), ref_part.cuda(), *fp3_p).cpu()
    assert torch.equal(out, ref), f"fp3: {int((out != ref).sum())} of {out.numel()} elements differ from fp64"


# ---- B: row_chain across its batch range ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _batch_problem(B):
    """Rows and their float64 evaluation (on the device: 32 K rows at B = 1024), shared by the cases of one B and never
    modified; only the latest B is kept (134 MB at B = 1024)."""
    x = C.random_rows(B, C.BATCH_N, 4000 + B).cuda()
    return x, C.row_chain_ref(x, _cuda(C.row_weights())).cpu()


@pytest.mark.parametrize("kind", ["cycle", "last"])
@pytest.mark.parametrize("B", C.BATCHES)
def test_row_chain_across_the_batch_range(B, kind):
    N = C.BATCH_N
    x, ref = _batch_problem(B)
    lst, counts, mask = C.lists(B, N, C.batch_pairs(B, kind), 17 * B)
    outs = [_row_chain(x, lst, counts, _row_packed(), grid=grid) for grid in (1, 7, _cus())]
    torch.cuda.synchronize()
    _check(outs[0], ref, mask, f"B = {B} ({kind}), grid 1")
    for grid, out in zip((7, _cus()), outs[1:]):
        assert torch.equal(out, outs[0]), f"grid {grid} differs from grid 1 at B = {B} ({kind})"


def _lds_child():
    """Body of the child process of test_row_chain_lds_opt_in_covers_a_later_larger_batch: this process's first row_chain call
    has one cloud, its second 1024 clouds on the same weights."""
    packed = _row_packed()
    runs = []
    for B in (1, 1024):
        x = C.random_rows(B, C.BATCH_N, 4000 + B).cuda()
        lst, counts, mask = C.lists(B, C.BATCH_N, C.batch_pairs(B, "cycle") if B > 1 else [(15, 17)], 17 * B)
        runs.append((B, x, lst, counts, mask, _row_chain(x, lst, counts, packed)))  # the default grid
        torch.cuda.synchronize()
    for B, x, lst, counts, mask, out in runs:
        one = _row_chain(x, lst, counts, packed, grid=1)
        torch.cuda.synchronize()
        assert torch.equal(out, one), f"B = {B}: the default grid differs from grid 1"
        _check(out, C.row_chain_ref(x, _cuda(C.row_weights())).cpu(), mask, f"child, B = {B}")
    print("lds child ok")


def test_row_chain_lds_opt_in_covers_a_later_larger_batch():
    """The dynamic-LDS size grows with the batch and the opt-in above 64 KB is made once per device: it has to cover the
    largest batch, not the first call's.  A fresh process, because the opt-in of this one is long made."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_chain_range as t; t._lds_child()" % (os.path.dirname(tests), tests)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "lds child ok" in out.stdout, out.stderr[-3000:]


def test_row_chain_rejections():
    from hotrack_amd import ext
    from hotrack_amd.pointnet2_hip import Pn2Error
    packed = _row_packed()

    def run(x, out=None):
        B, N = x.shape[:2]
        lst = torch.zeros((B, N), dtype=torch.int32, device="cuda")
        counts = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        out = torch.full((B, N, 512), SENTINEL, device="cuda") if out is None else out
        ext.row_chain(x, lst, counts, *packed, out=out)
        return out

    assert ext.ROW_CHAIN_MAX_B == 1024
    with pytest.raises(Pn2Error, match=r"code -3"):  # PN2_ERANGE: one cloud beyond the LDS prefix arrays
        run(torch.zeros(1025, 1, 132, device="cuda"))
    with pytest.raises(Pn2Error, match=r"code -1"):  # PN2_EINVAL: ldx = 134 is not a multiple of 4
        run(torch.zeros(2, 4, 134, device="cuda")[:, :, :132])
    with pytest.raises(Pn2Error, match=r"code -1"):  # ldo = 514
        run(torch.zeros(2, 4, 132, device="cuda"), out=torch.full((2, 4, 514), SENTINEL, device="cuda")[:, :, :512])
    flat = torch.zeros(2 * 4 * 132 + 4, device="cuda")
    with pytest.raises(Pn2Error, match=r"code -1"):  # x starts one float into a row: not 16-byte aligned
        run(flat[1:1 + 2 * 4 * 132].view(2, 4, 132))
    out = run(flat[4:4 + 2 * 4 * 132].view(2, 4, 132))  # four floats in: aligned, accepted; empty lists write nothing
    assert bool((out == SENTINEL).all())


# ---- C: strides ----------------------------------------------------------------------------------------------------------------
STRIDE_PAIRS = ((15, 17), (0, 1), (40, 9))


@functools.lru_cache(maxsize=None)
def _stride_problem():
    B, N = 3, 64
    x = C.random_rows(B, N, 31)
    lst, counts, mask = C.lists(B, N, STRIDE_PAIRS, 5)
    base = _row_chain(x.cuda(), lst, counts, _row_packed(), grid=7)
    torch.cuda.synchronize()
    ref = C.row_chain_ref(x, C.row_weights())
    _check(base, ref, mask, "contiguous rows")
    return x, lst, counts, mask, base


@pytest.mark.parametrize("ld,col0", [(136, 0), (260, 0), (140, 4)])
def test_row_chain_reads_rows_of_any_stride(ld, col0):
    x, lst, counts, mask, base = _stride_problem()
    buf = torch.full((3, 64, ld), NAN)
    buf[:, :, col0:col0 + 132] = x
    view = buf.cuda()[:, :, col0:col0 + 132]
    assert view.stride(1) == ld
    assert torch.equal(_row_chain(view, lst, counts, _row_packed(), grid=7), base)


@pytest.mark.parametrize("ldo", [516, 1024])
def test_row_chain_writes_rows_of_any_stride(ldo):
    x, lst, counts, mask, base = _stride_problem()
    obuf = torch.full((3, 64, ldo), SENTINEL, device="cuda")
    _row_chain(x.cuda(), lst, counts, _row_packed(), grid=7, out=obuf[:, :, :512])
    assert torch.equal(obuf[:, :, :512], base)  # the listed elements bit-equal, the sentinel in the same places
    assert bool((obuf[:, :, 512:] == SENTINEL).all()), "wrote beyond column 511"


@pytest.mark.parametrize("ld,ldo", [(136, 260), (264, 512)])
def test_mid_chains_take_rows_of_any_stride(ld, ldo):
    from hotrack_amd import ext
    B, S = 2, 64
    x = C.random_rows(B, S, 32)
    sa3, fp3 = C.mid_weights()
    sa3_p, fp3_p = _mid_packed()
    part = ext.sa3_chain(x.cuda(), *sa3_p)
    out = ext.fp3_chain(x.cuda(), part, *fp3_p)
    _mid_close(part.cpu(), C.sa3_part_ref(x, sa3), "sa3, contiguous")
    _mid_close(out.cpu(), C.fp3_ref(x, part.cpu().double().amax(1), fp3), "fp3, contiguous")
    buf = torch.full((B, S, ld), NAN)
    buf[:, :, :132] = x
    view = buf.cuda()[:, :, :132]
    assert torch.equal(ext.sa3_chain(view, *sa3_p), part)
    obuf = torch.full((B, S, ldo), SENTINEL, device="cuda")
    ext.fp3_chain(view, part, *fp3_p, out=obuf[:, :, :256])
    assert torch.equal(obuf[:, :, :256], out)
    assert bool((obuf[:, :, 256:] == SENTINEL).all()), "wrote beyond column 255"


# ---- D: mid chains at other S ----------------------------------------------------------------------------------------------------
def _mid_against_fp64(x, what):
    """sa3's per-tile maxima against float64, then fp3 on them against float64 with l3 = part.amax(1).  The references run on
    the device too (32 K rows at S = 1024)."""
    from hotrack_amd import ext
    sa3, fp3 = C.mid_weights()
    sa3_p, fp3_p = _mid_packed()
    B, S = x.shape[:2]
    x = x.cuda()
    part = torch.full((B, S // C.TILE, 512), SENTINEL, device="cuda")
    ext.sa3_chain(x, *sa3_p, part=part)
    out = ext.fp3_chain(x, part, *fp3_p)
    _mid_close(part, C.sa3_part_ref(x, tuple(_cuda(l) for l in sa3)), f"sa3 {what}")
    _mid_close(out, C.fp3_ref(x, part.double().amax(1), _cuda(fp3)), f"fp3 {what}")
    return part.cpu()


@pytest.mark.parametrize("S,B", C.MID_SHAPES)
def test_mid_chains_at_other_row_counts(S, B):
    _mid_against_fp64(C.random_rows(B, S, 100 * S + B), f"S = {S}, B = {B}")


@pytest.mark.parametrize("S", C.MID_S)
def test_mid_chains_take_the_maximum_from_the_right_partial(S):
    """Cloud t's rows of tile t are scaled by 3: most of its maxima come from partial t (tests/test_chain_cases.py)."""
    x = C.tile_scaled_rows(S)
    part = _mid_against_fp64(x, f"S = {S}, scaled tiles")
    winner = part.argmax(dim=1)
    for t in range(S // C.TILE):
        assert int((winner[t] == t).sum()) >= 256, (S, t)


def test_sa3_chain_all_negative_gives_positive_zero():
    from hotrack_amd import ext
    (l1, l2, (w3, b3)), _ = C.mid_weights()
    sa3 = (l1, l2, (w3, torch.full_like(b3, -1e3)))
    x = C.random_rows(3, 96, 8)
    assert float(C.sa3_layers(x, sa3)[2].max()) < 0  # every layer-3 pre-activation is negative
    part = ext.sa3_chain(x.cuda(), *_pack_mid(sa3, C.mid_weights()[1])[0])
    assert bool((part.view(torch.int32) == 0).all()), "part is not +0.0 everywhere (bits)"


def test_mid_chains_refuse_a_row_count_off_the_tile():
    from hotrack_amd import ext
    assert not ext.sa3_chain_supported(48, 128, 128, 128, 512) and not ext.fp3_chain_supported(48, 128, 512, 256, 256)
    assert all(ext.sa3_chain_supported(S, 128, 128, 128, 512) and ext.fp3_chain_supported(S, 128, 512, 256, 256) for S in C.MID_S)
    sa3_p, fp3_p = _mid_packed()
    x = torch.zeros(2, 48, 132, device="cuda")
    with pytest.raises(ValueError):
        ext.sa3_chain(x, *sa3_p)
    with pytest.raises(ValueError):
        ext.fp3_chain(x, torch.zeros(2, 1, 512, device="cuda"), *fp3_p)
    lib, n = ext._lib, None  # the C ABI itself: PN2_EINVAL before the pointers are looked at
    assert lib.pn2x_sa3_chain(2, 48, n, 132, n, n, n, n, n, n, n, None) == -1
    assert lib.pn2x_fp3_chain(2, 48, n, 132, n, n, n, n, n, n, n, 256, None) == -1


# ---- E: row_lists across its range -------------------------------------------------------------------------------------------------
def _row_lists_raw(gi, gs, N, k_small=None):
    """pn2x_row_lists through the C ABI into a pre-filled list (ext.row_lists allocates with empty).  gs None: prefix mode with
    k_small.  -> rc, list (B, N), counts (B, 2) on the CPU."""
    from hotrack_amd import ext
    B, J, KL = gi.shape
    gi = gi.cuda().contiguous()
    gs = None if gs is None else gs.cuda().contiguous()
    KS = gs.shape[2] if gs is not None else k_small
    lst = torch.full((B, N), FILL, dtype=torch.int32, device="cuda")
    counts = torch.full((B, 2), FILL, dtype=torch.int32, device="cuda")
    rc = ext._lib.pn2x_row_lists(B, N, J, KL, KS, gi.data_ptr(), None if gs is None else gs.data_ptr(), lst.data_ptr(),
                                 counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, lst.cpu(), counts.cpu()


def _check_lists(gi, gs, N, what):
    rc, lst, counts = _row_lists_raw(gi, gs, N)
    assert rc == 0, (what, rc)
    for b in range(gi.shape[0]):
        want, (ns, na) = C.lists_from_sets((gs[b], gi[b]), N)
        assert counts[b].tolist() == [ns, na], (what, b, counts[b].tolist(), ns, na)
        assert torch.equal(lst[b, :na], want), (what, b)
        assert bool((lst[b, na:] == FILL).all()), f"{what}: cloud {b} wrote past its count"
    return lst, counts


@pytest.mark.parametrize("shape", C.ROW_LIST_SHAPES, ids=str)
def test_row_lists_match_torch_unique_across_the_range(shape):
    from hotrack_amd import ext
    B, J, N, KL, KS = shape
    kinds = ["random", "last", "first"] + (["all"] if J * KL >= N else []) + (["words"] if N == 16384 else [])
    for kind in kinds:
        gi, gs = C.hand_indices(B, J, N, KL, KS, kind)
        lst, counts = _check_lists(gi, gs, N, f"{shape} {kind}")
        if kind == "all":
            assert counts[:, 1].tolist() == [N] * B
    if N >= KL and N > 1:  # the kNN kernel's own lists (sorted by distance, duplicates across keypoints)
        g = torch.Generator().manual_seed(N)
        gi, gs = ext.knn_indices(KL, torch.rand(B, J, 3, generator=g).cuda(), torch.rand(B, N, 3, generator=g).cuda(), k2=KS)
        _check_lists(gi.cpu(), gs.cpu(), N, f"{shape} knn")
        a, b = ext.row_lists(gi, gs, N)  # the Python entry gives the same counts and listed rows
        rc, lst, counts = _row_lists_raw(gi, gs, N)
        assert torch.equal(b.cpu(), counts) and all(torch.equal(a[i, :counts[i, 1]].cpu(), lst[i, :counts[i, 1]]) for i in range(B))


@pytest.mark.parametrize("shape", C.ROW_LIST_SHAPES, ids=str)
def test_row_lists_ignore_out_of_range_indices(shape):
    B, J, N, KL, KS = shape
    gi, gs = C.hand_indices(B, J, N, KL, KS, "random")
    gi_d, gi_c = C.with_out_of_range(gi, N, 1)
    gs_d, gs_c = C.with_out_of_range(gs, N, 2)
    lst_d, cnt_d = _check_lists(gi_d, gs_d, N, f"{shape} with out-of-range entries")
    lst_c, cnt_c = _check_lists(gi_c, gs_c, N, f"{shape} without them")
    assert torch.equal(lst_d, lst_c) and torch.equal(cnt_d, cnt_c)
    rc, lst_p, cnt_p = _row_lists_raw(gi_d, None, N, k_small=KS)  # prefix mode skips them as well
    rc2, lst_q, cnt_q = _row_lists_raw(gi_c, None, N, k_small=KS)
    assert rc == 0 and rc2 == 0 and torch.equal(lst_p, lst_q) and torch.equal(cnt_p, cnt_q)


def test_row_lists_prefix_mode_equals_the_two_tensor_call():
    for B, J, N, KL, KS in ((2, 21, 1000, 64, 16), (2, 5, 100, 7, 3)):
        gi, _ = C.hand_indices(B, J, N, KL, KS, "random")
        rc, lst, counts = _row_lists_raw(gi, None, N, k_small=KS)
        rc2, lst2, counts2 = _row_lists_raw(gi, gi[:, :, :KS].contiguous(), N)
        assert rc == 0 and rc2 == 0
        assert torch.equal(lst, lst2) and torch.equal(counts, counts2)
        assert bool((counts[:, 0] < counts[:, 1]).all())  # the prefix is a strict subset here: both parts are populated
        _check_lists(gi, gi[:, :, :KS].contiguous(), N, "prefix mode's twin")


def test_row_lists_rejections():
    gi, gs = C.hand_indices(1, 2, 64, 8, 4, "random")
    assert _row_lists_raw(gi, gs, 16385)[0] == -3                 # PN2_ERANGE: beyond the LDS bitmap
    rc, lst, counts = _row_lists_raw(gs, gi, 64)                   # k_small = 8 > k_large = 4: PN2_EINVAL, nothing written
    assert rc == -1 and bool((lst == FILL).all()) and bool((counts == FILL).all())


def test_row_lists_feed_row_chain_off_the_benchmark_shape():
    B, J, N, KL, KS = 2, 21, 1000, 64, 16
    gi, gs = C.hand_indices(B, J, N, KL, KS, "random")
    rc, lst, counts = _row_lists_raw(gi, gs, N)
    assert rc == 0
    mask = torch.zeros(B, N, 512, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.unique(gs[b]).long()] = True
        mask[b, torch.unique(gi[b]).long(), 256:] = True
    x = C.random_rows(B, N, 33)
    out = _row_chain(x.cuda(), lst, counts, _row_packed())
    torch.cuda.synchronize()
    _check(out, C.row_chain_ref(x, C.row_weights()), mask, "row_lists -> row_chain, N = 1000")


# ---- F: ill-scaled rows against a derived bound ------------------------------------------------------------------------------------
def _bound_ratio(got, ref, e, what):
    # |got - ref| <= 2 e + u |ref|: e is the first-order forward bound of _chain_cases.forward_bound; the factor 2 covers the
    # second-order terms it drops and u |ref| the rounding of the float64 reference to the float32 result.
    bound = 2 * e + C.U * ref.abs()
    ratio = float(((got.double() - ref).abs() / bound).max())
    print(f"{what}: worst |err| / bound = {ratio:.3e} (|ref| from {float(ref.abs().min()):.2e} to {float(ref.abs().max()):.2e})")
    assert ratio <= 1.0, (what, ratio)


def test_row_chain_ill_scaled_rows_within_the_forward_bound():
    B, N = 2, 64
    x = C.ill_scaled_rows(B, N, 9)
    lst, counts, mask = C.lists(B, N, ((40, 24), (64, 0)), 6)
    out = _row_chain(x.cuda(), lst, counts, _row_packed()).cpu()
    ref, e = C.row_chain_bound(x, C.row_weights())
    assert bool((out[~mask] == SENTINEL).all())
    _bound_ratio(out[mask], ref[mask], e[mask], "row_chain, ill-scaled rows")


def test_sa3_chain_ill_scaled_rows_within_the_forward_bound():
    from hotrack_amd import ext
    x = C.ill_scaled_rows(2, 64, 10)
    part = ext.sa3_chain(x.cuda(), *_mid_packed()[0]).cpu()
    ref, e = C.sa3_part_bound(x, C.mid_weights()[0])
    _bound_ratio(part, ref, e, "sa3, ill-scaled rows")
