"""GPU: the row chains' results do not depend on how rows fall into tiles.

pn2x_row_chain (hotrack_amd/csrc/row_chain.hip) splits its rows over the grid in 16-row groups and runs each workgroup's
share as tiles of one to four groups; the k-loop (mfma_rows.h) accumulates every output element over the same k order whatever
the tile.  So grids of 1, 7 and one workgroup per compute unit -- three different partitions of the same rows -- must give
bit-equal outputs (torch.equal, no tolerance), write nothing outside the listed rows and columns, and stay within the fp64
bound of tests/test_gpu_row_chain.py.  pn2x_sa3_chain / pn2x_fp3_chain (mid_chain.hip) share the k-loop; their grid is fixed
at one workgroup per 32-row tile, so the partition is varied through the position of a cloud in the batch.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
S = 128  # level-2 rows per cloud (sa3 / fp3)


@functools.lru_cache(maxsize=None)
def _weights():
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(11)

    def lin(o, i, s):
        return (torch.randn(o, i, generator=g) * s).cuda(), (torch.randn(o, generator=g) * 0.1).cuda()
    wa, ba = lin(128, 131, 0.1)
    wb, bb = lin(128, 128, 0.1)
    wc, bc = lin(384, 128, 0.1)
    wq = (torch.randn(512, 384, generator=g) * 0.05).cuda()
    p = ext.row_chain_pack
    return (wa, ba, wb, bb, wc, bc, wq), (p(wa), ba, p(wb), bb, p(wc), bc, p(wq))


@functools.lru_cache(maxsize=None)
def _problem(B, N):
    """Input rows and their fp64 evaluation (B, N, 512), computed once per shape and never modified."""
    g = torch.Generator().manual_seed(1000 * B + N)
    x = torch.randn(B, N, 132, generator=g).cuda()
    x[:, :, 131] = float("nan")  # the pad float is never read
    wa, ba, wb, bb, wc, bc, wq = (t.double() for t in _weights()[0])
    h = torch.relu(x[..., :131].double() @ wa.t() + ba)
    h = torch.relu(h @ wb.t() + bb)
    c = torch.relu(h @ wc.t() + bc)
    return x, (c @ wq.t()).cpu()


def _lists(B, N, pairs, seed):
    """Hand-built lists: cloud b names pairs[b] = (small, large-only) distinct points drawn at random, each part ascending."""
    g = torch.Generator().manual_seed(seed)
    lst = torch.full((B, N), -7, dtype=torch.int32)
    counts = torch.zeros((B, 2), dtype=torch.int32)
    mask = torch.zeros(B, N, 512, dtype=torch.bool)
    for b, (ns, nl) in enumerate(pairs):
        perm = torch.randperm(N, generator=g)
        s, o = perm[:ns].sort().values, perm[ns:ns + nl].sort().values
        lst[b, :ns + nl] = torch.cat([s, o]).int()
        counts[b, 0], counts[b, 1] = ns, ns + nl
        mask[b, s, :] = True
        mask[b, o, 256:] = True
    return lst.cuda(), counts.cuda(), mask


def _pairs(N):
    ps = [(0, 0), (1, 0), (0, 1), (15, 17), (16, 16), (17, 47), (64, 0), (65, 63), (N, 0)]
    return [p for i, p in enumerate(ps) if p[0] + p[1] <= N and p not in ps[:i]]


def _cases():
    out = []
    for N in (64, 1000):
        ps = _pairs(N)
        out += [(1, N, (p,)) for p in ps]
        ps3 = ps + ps[: (-len(ps)) % 3]  # B = 3: consecutive triples, the last one padded from the front
        out += [(3, N, tuple(ps3[i:i + 3])) for i in range(0, len(ps3), 3)]
        out.append((3, N, ((N, 0), (0, 0), (65 if N > 128 else 17, 63 if N > 128 else 47))))  # a run that crosses an empty cloud
    return out


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(out, ref, mask, what):
    out = out.cpu()
    assert bool((out[~mask] == SENTINEL).all()), f"{what}: wrote outside the listed rows / columns"
    if mask.any():
        scale = max(1.0, float(ref.abs().max()))
        err = float((out.double()[mask] - ref[mask]).abs().max())
        print(f"{what}: max |err| vs fp64 = {err:.3e} (bound {2e-5 * scale:.3e})")
        assert err <= 2e-5 * scale, (what, err)


@pytest.mark.parametrize("B,N,pairs", _cases(), ids=lambda v: str(v).replace(" ", ""))
def test_row_chain_bits_do_not_depend_on_the_grid(B, N, pairs):
    from hotrack_amd import ext
    x, ref = _problem(B, N)
    lst, counts, mask = _lists(B, N, pairs, 7 * N + B)
    outs = []
    for grid in (1, 7, _cus()):
        out = torch.full((B, N, 512), SENTINEL, device="cuda")
        ext.row_chain(x, lst, counts, *_weights()[1], out=out, grid=grid)
        outs.append(out)
    torch.cuda.synchronize()
    _check(outs[0], ref, mask, f"grid 1 {pairs}")
    for grid, out in zip((7, _cus()), outs[1:]):
        assert torch.equal(out, outs[0]), f"grid {grid} differs from grid 1 for {pairs}"


def test_row_chain_capture_on_one_list_and_replay_on_others():
    from hotrack_amd import ext
    B, N = 3, 1000
    x, ref = _problem(B, N)
    lst_s, cnt_s, _ = _lists(B, N, ((16, 16), (0, 0), (1, 0)), 1)
    buf = torch.full((B, N, 512), SENTINEL, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the kernel has run once before the capture
        ext.row_chain(x, lst_s, cnt_s, *_weights()[1], out=buf, grid=7)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ext.row_chain(x, lst_s, cnt_s, *_weights()[1], out=buf, grid=7)
    for r, pairs in enumerate((((65, 63), (N, 0), (17, 47)), ((0, 1), (64, 0), (15, 17)), ((0, 0), (0, 0), (0, 0)))):
        lst, counts, mask = _lists(B, N, pairs, 50 + r)
        lst_s.copy_(lst)
        cnt_s.copy_(counts)
        buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        _check(buf, ref, mask, f"replay on {pairs}")
        eager = torch.full((B, N, 512), SENTINEL, device="cuda")
        ext.row_chain(x, lst, counts, *_weights()[1], out=eager, grid=1)
        assert torch.equal(buf, eager), f"replay on {pairs} differs from an eager launch on one workgroup"


# ---- sa3 / fp3 -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid_weights():
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(23)

    def lin(o, i):  # BatchNorm-folded-like weights, as in tests/test_gpu_mid_chain.py
        scale = 0.5 + torch.rand(o, 1, generator=g)
        return (torch.randn(o, i, generator=g) / i ** 0.5 * scale).cuda(), (torch.randn(o, generator=g) * 0.1).cuda()
    sa3 = [lin(128, 131), lin(128, 128), lin(512, 128)]
    wg, bg = lin(256, 512)
    wa, _ = lin(256, 128)
    wf, bf = lin(256, 256)
    p = ext.row_chain_pack
    packed = ([t for W, b in sa3 for t in (p(W), b)], (wg.t().contiguous(), bg, p(wa), p(wf), bf))
    return sa3, (wg, bg, wa, wf, bf), packed


def _mid_run(x):
    from hotrack_amd import ext
    _, _, (sa3_p, fp3_p) = _mid_weights()
    part = ext.sa3_chain(x, *sa3_p)
    return part, ext.fp3_chain(x, part, *fp3_p)


@pytest.mark.parametrize("B", [1, 3])
def test_mid_chains_bits_do_not_depend_on_the_tile_position(B):
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(40 + B)
    x = torch.randn(B, S, 132, generator=g)
    x[:, :, 131] = float("nan")
    x = x.cuda()
    sa3, fp3, _ = _mid_weights()
    part, out = _mid_run(x)
    torch.cuda.synchronize()
    # fp64, at the bound of tests/test_gpu_mid_chain.py
    h = x[..., :131].double()
    for W, b in sa3:
        h = torch.relu(h @ W.double().t() + b.double())
    T = ext.MID_CHAIN_TILE
    y = h.view(B, S // T, T, 512).amax(dim=2).float()
    assert torch.allclose(part, y, atol=2e-5, rtol=1e-5), float((part - y).abs().max())
    wg, bg, wa, wf, bf = (t.double() for t in fp3)
    gl = part.double().amax(dim=1) @ wg.t() + bg
    ref = torch.relu(torch.relu(x[..., :128].double() @ wa.t() + gl[:, None, :]) @ wf.t() + bf).float()
    assert torch.allclose(out, ref, atol=2e-5, rtol=1e-5), float((out - ref).abs().max())
    # the same clouds at other positions of a batch (other workgroups), and each cloud alone
    pad = torch.randn(2, S, 132, generator=g).cuda()
    part2, out2 = _mid_run(torch.cat([pad, x.flip(0)], 0).contiguous())
    assert torch.equal(part2[2:].flip(0), part) and torch.equal(out2[2:].flip(0), out)
    for b in range(B):
        pb, ob = _mid_run(x[b:b + 1].clone())
        assert torch.equal(pb[0], part[b]) and torch.equal(ob[0], out[b])
