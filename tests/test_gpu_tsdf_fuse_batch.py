"""GPU: the batched TSDF fusion launch (hotrack_amd/csrc/tsdf_fuse.hip: pn2s_tsdf_integrate_batch, hotrack_amd.sdf.tsdf_integrate_batch)
over the groups of tests/_tsdf_batch_cases.py: every sequence bit-equal to the single entry on it alone and inside the float64
check of tests/_tsdf_cases.py; sitting-out sequences and unobserved voxels keep their bytes; the second z tile at res 257;
repeatability; refused calls; VolumeFusionGroup without host synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

import _tsdf_batch_cases as B
import _tsdf_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu
IDS = [g["name"] for g in B.GROUPS]


def _dev():
    return torch.device("cuda", 0)


def _bits(x):
    x = x.detach().cpu().contiguous().numpy()
    return x.view(np.uint16 if x.dtype == np.float16 else np.uint32)


def _pattern(like, seed):
    """A tensor of like's shape and dtype whose BYTES are arbitrary: NaNs with payloads, infinities, denormals among them."""
    gen = torch.Generator().manual_seed(seed)
    wide = like.dtype == torch.float32
    top = 31 if wide else 15
    bits = torch.randint(-2 ** top, 2 ** top, (like.numel(),), dtype=torch.int64, generator=gen).to(torch.int32 if wide else torch.int16)
    bits[::3] = bits[::3] | (0x7F800001 if wide else 0x7C01)   # exponent all ones, mantissa not zero: NaNs, each with its payload
    out = bits.view(like.dtype).reshape(like.shape).to(like.device)
    assert bool(torch.isnan(out).any()) and not bool(torch.isnan(out).all())
    return out


def _run(group):
    from hotrack_amd import sdf
    args, kw, singles = B.pack(group, _dev())
    vols, wts = sdf.tsdf_integrate_batch(*args, **kw)
    assert vols is args[0] and wts is args[1]
    return args, kw, singles


@pytest.mark.parametrize("group", B.GROUPS, ids=IDS)
def test_every_sequence_has_the_single_entrys_bits_and_passes_the_fp64_check(group):
    from hotrack_amd import sdf
    args, kw, singles = _run(group)
    for k, single in enumerate(singles):
        if single is None:
            assert args[0][k] is None and args[1][k] is None
            continue
        V, W = sdf.tsdf_integrate(*single[0], **single[1])
        assert torch.equal(args[0][k], V) and torch.equal(args[1][k], W), (group["name"], k)
        assert np.array_equal(_bits(args[0][k]), _bits(V)) and np.array_equal(_bits(args[1][k]), _bits(W))
        case = B.sequence_case(group, k)
        B.reference(case)
        T.check(case, args[0][k].cpu().numpy(), args[1][k].cpu().numpy(), "batched kernel")   # (asserts MAX_EXCLUDED too)


@pytest.mark.parametrize("group", [B.GROUPS[0], B.GROUPS[3]], ids=[IDS[0], IDS[3]])
def test_a_sequence_that_sits_out_and_unobserved_voxels_keep_their_bytes(group):
    from hotrack_amd import sdf
    args, kw, singles = B.pack(group, _dev())
    vols, wts = args[0], args[1]
    live = next(k for k, s in enumerate(singles) if s is not None)
    idle = [k for k, s in enumerate(singles) if s is None]
    assert idle
    for k in idle:   # real tensors, count 0
        vols[k], wts[k] = _pattern(vols[live], 11 + k), _pattern(wts[live], 23 + k)
    before = [(_bits(vols[k]).copy(), _bits(wts[k]).copy()) for k in range(len(vols))]
    sdf.tsdf_integrate_batch(*args, **kw)
    torch.cuda.synchronize()
    for k in idle:
        assert np.array_equal(_bits(vols[k]), before[k][0]) and np.array_equal(_bits(wts[k]), before[k][1])
    for k, single in enumerate(singles):
        if single is None:
            continue
        a, _, _, cmp = B.reference(B.sequence_case(group, k))
        _, _, touched = T.fuse_fp32(a)
        keep = ~touched & cmp
        assert keep.any() and touched.any()
        assert np.array_equal(_bits(vols[k])[keep], before[k][0][keep]) and np.array_equal(_bits(wts[k])[keep], before[k][1][keep])
        assert not np.array_equal(_bits(wts[k]), before[k][1])


def test_the_second_z_tile_at_res_257():
    """res 257 = 256 + 1: the second z tile holds one voxel per row; bit-equality with the single entry only."""
    from hotrack_amd import sdf
    dev = _dev()
    res, scale, S = 257, 0.001, 2
    g17 = B.GROUPS[0]
    frames = [T.to_torch(B.reference(B.sequence_case(g17, k))[0], dev) for k in (2, 3)]   # 24 x 32 fp32 frames
    kw = dict(frames[0][1], trunc=5 * scale)
    ax = (torch.arange(res, device=dev) - res // 2).float() * scale
    prior = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt() - 0.04
    vols = [(prior + 0.002 * k).clamp(-5 * scale, 5 * scale).half().contiguous() for k in range(S)]
    wts = [torch.full((res,) * 3, 1.0 + k, device=dev) for k in range(S)]
    packed = [torch.cat([fr[0][i][:1] for fr in frames]).contiguous() for i in range(3, 8)]
    want = [sdf.tsdf_integrate(vols[k].clone(), wts[k].clone(), scale, *(x[k:k + 1].contiguous() for x in packed), **kw) for k in range(S)]
    last_tile = [wts[k][:, :, 256].clone() for k in range(S)]
    sdf.tsdf_integrate_batch(vols, wts, scale, *packed, [1, 1], **kw)
    for k in range(S):
        assert torch.equal(vols[k], want[k][0]) and torch.equal(wts[k], want[k][1]), k
    assert any(not torch.equal(wts[k][:, :, 256], last_tile[k]) for k in range(S))   # the one-voxel tile was reached (carved: its weights grew)


@pytest.mark.parametrize("group", [B.GROUPS[1], B.GROUPS[2]], ids=[IDS[1], IDS[2]])
def test_two_runs_are_bitwise_equal(group):
    a, _, _ = _run(group)
    b, _, _ = _run(group)
    for k in range(len(a[0])):
        if a[0][k] is not None:
            assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])) and np.array_equal(_bits(a[1][k]), _bits(b[1][k]))


def test_one_sequence_equals_the_single_entry():
    from hotrack_amd import sdf
    single = T.to_torch(B.reference(B.sequence_case(B.GROUPS[2], 0))[0], _dev())
    V, W = single[0][0].clone(), single[0][1].clone()
    sdf.tsdf_integrate_batch([V], [W], *single[0][2:], [3], **single[1])
    want = sdf.tsdf_integrate(*single[0], **single[1])
    assert torch.equal(V, want[0]) and torch.equal(W, want[1])


def _mixed_res(a, kw):
    a[0][0], a[1][0] = a[0][0][:9, :9, :9].contiguous(), a[1][0][:9, :9, :9].contiguous()


def _too_many(a, kw):
    from hotrack_amd import sdf
    extra = sdf.TSDF_BATCH_MAX + 1 - len(a[8])
    for i in (0, 1):
        a[i] = a[i] + [None] * extra
    a[8] = a[8] + [0] * extra


BAD = [
    ("mixed res", _mixed_res, ValueError),
    ("mixed dtype", lambda a, kw: a[0].__setitem__(2, a[0][2].float() if a[0][2].dtype == torch.float16 else a[0][2].half()), ValueError),
    ("aliased volumes", lambda a, kw: a[0].__setitem__(3, a[0][0]), ValueError),
    ("aliased weights", lambda a, kw: a[1].__setitem__(2, a[1][3]), ValueError),
    ("counts do not sum to F", lambda a, kw: a[8].__setitem__(0, 2), ValueError),
    ("None with a count", lambda a, kw: (a[8].__setitem__(1, 1), a[8].__setitem__(0, 2)), ValueError),
    ("negative count", lambda a, kw: (a[8].__setitem__(0, 4), a[8].__setitem__(2, -1), a[8].__setitem__(3, 3)), ValueError),
    ("S above the limit", _too_many, ValueError),
    ("trunc", lambda a, kw: kw.__setitem__("trunc", 0.0), ValueError),
    ("cpu depth", lambda a, kw: a.__setitem__(3, a[3].cpu()), RuntimeError),
]


@pytest.mark.parametrize("what,spoil,error", BAD, ids=[b[0] for b in BAD])
def test_refused_calls_raise_and_change_nothing(what, spoil, error):
    from hotrack_amd import sdf
    args, kw, _ = B.pack(B.GROUPS[0], _dev())
    args = list(args)
    held = [(v, w) for v, w in zip(args[0], args[1]) if v is not None]
    before = [(_bits(v).copy(), _bits(w).copy()) for v, w in held]
    spoil(args, kw)
    with pytest.raises(error):
        sdf.tsdf_integrate_batch(*args, **kw)
    torch.cuda.synchronize()
    for (v, w), (bv, bw) in zip(held, before):
        assert np.array_equal(_bits(v), bv) and np.array_equal(_bits(w), bw)


def test_the_c_entry_refuses_and_an_empty_group_launches_nothing():
    """pn2s_tsdf_integrate_batch's own checks, behind the binding's: negative codes with the volumes' bytes unchanged; S = 0,
    F = 0 and a table of empty slices are accepted and change nothing; a slice past F is clamped."""
    import ctypes
    from hotrack_amd import sdf
    args, kw, _ = B.pack(B.GROUPS[4], _dev())
    vols, wts, scale, depth, seg, intr, rot, trans, counts = args
    F = sum(counts)
    before = [(_bits(v).copy(), _bits(w).copy()) for v, w in zip(vols, wts)]
    ptrs = torch.tensor([v.data_ptr() for v in vols] + [w.data_ptr() for w in wts], dtype=torch.int64, device=_dev())

    def record(off, **over):
        r = sdf._TsdfGroup(res=5, vol_f16=0, sequences=2, frames=F, h=24, w=32, hs=24, ws=32, c=3, depth_u16=0, flip_yz=0, channel=1,
                           value=255, depth_scale=0.0, voxel_scale=scale, trunc=kw["trunc"], carve_weight=1.0, max_weight=64.0)
        r.volumes, r.weights, r.frame_off = ptrs.data_ptr(), ptrs.data_ptr() + 16, off.data_ptr()
        r.depth, r.seg, r.intrinsics, r.rotation, r.translation = (x.data_ptr() for x in (depth, seg, intr, rot, trans))
        for k, v in over.items():
            setattr(r, k, v)
        return r

    call = lambda r: sdf._lib.pn2s_tsdf_integrate_batch(ctypes.byref(r), None)
    off = torch.tensor([0, 2, 3], dtype=torch.int32, device=_dev())
    for over, code in ((dict(res=1), -1), (dict(sequences=-1), -1), (dict(frames=-1), -1), (dict(vol_f16=2), -1), (dict(trunc=0.0), -1),
                       (dict(hs=5), -1), (dict(c=2), -1), (dict(depth_u16=1), -1), (dict(res=513), -3), (dict(sequences=65536), -3),
                       (dict(frames=65536), -3), (dict(depth=None), -2), (dict(volumes=None), -2), (dict(frame_off=None), -2)):
        assert call(record(off, **over)) == code, over
    assert sdf._lib.pn2s_tsdf_integrate_batch(None, None) == -2
    empty = torch.zeros(3, dtype=torch.int32, device=_dev())
    backwards = torch.tensor([3, 2, 0], dtype=torch.int32, device=_dev())
    for r in (record(off, sequences=0), record(off, frames=0, depth=None), record(empty), record(backwards)):
        assert call(r) == 0
    torch.cuda.synchronize()
    for (v, w), (bv, bw) in zip(zip(vols, wts), before):
        assert np.array_equal(_bits(v), bv) and np.array_equal(_bits(w), bw)
    # offsets that reach past F are clamped to it: sequence 0 gets its two frames, sequence 1 frames [2, F) = its one
    wild = torch.tensor([-5, 2, 1 << 30], dtype=torch.int32, device=_dev())
    assert call(record(wild)) == 0
    want_v, want_w = [v.clone() for v in vols], [w.clone() for w in wts]
    fresh, _, _ = B.pack(B.GROUPS[4], _dev())
    sdf.tsdf_integrate_batch(*fresh, **kw)
    for k in range(2):
        assert torch.equal(want_v[k], fresh[0][k]) and torch.equal(want_w[k], fresh[1][k])
        assert not np.array_equal(_bits(vols[k]), before[k][0])


def test_volume_fusion_group_does_not_synchronise_and_matches_single_fusions():
    from models.shape_fusion import VolumeFusion, VolumeFusionGroup
    group = B.GROUPS[2]
    dev = _dev()
    cases = [B.sequence_case(group, k) for k in range(4)]
    ins = [None if c is None else B.reference(c)[0] for c in cases]
    tens = [None if a is None else T.to_torch(a, dev) for a in ins]
    a0 = ins[0]
    handed = tens[0][0][0].clone()   # one tensor handed over by every sequence
    keep = handed.clone()

    def frames(k):
        args = tens[k][0]
        return [({"depth": args[3][i], "seg": args[4][i], "intrinsics": args[5][i], "depth_scale": a0["depth_scale"]},
                 {"rotation": args[6][i:i + 1], "translation": args[7][i].reshape(1, 3, 1)}) for i in range(args[3].shape[0])]

    def drive(fusion):   # sequence 0 flushes after two frames and again at its end, with sequences 2 and 3
        for i in range(2):
            fusion.push(0, *frames(0)[i])
        assert fusion.due(0) and not fusion.due(1) and fusion.pending(0) == 2 and fusion.pending(1) == 0
        fusion.flush([0])
        fusion.push(0, *frames(0)[2])
        fusion.push(2, *frames(2)[0])
        for fr in frames(3):
            fusion.push(3, *fr)
        return fusion.flush([0, 2, 3])

    new = lambda: VolumeFusionGroup([handed, None, handed, handed], a0["voxel_scale"], 2.0, a0["trunc"], every=2, obj_class=a0["obj_class"])
    drive(new())   # (first use: whatever is set up once)
    fusion = new()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = drive(fusion)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(handed, keep) and [fusion.state(k)["frames"] for k in (0, 2, 3)] == [3, 1, 2]
    assert len({o.data_ptr() for o in out} | {handed.data_ptr()}) == 4
    for k, vol in zip((0, 2, 3), out):
        alone = VolumeFusion(handed, a0["voxel_scale"], 2.0, a0["trunc"], every=2, obj_class=a0["obj_class"])
        for i, fr in enumerate(frames(k)):
            alone.push(*fr)
            if alone.due():
                alone.flush()
        alone.flush()
        assert vol is fusion.state(k)["volume"] and torch.equal(vol, alone.volume) and torch.equal(fusion.state(k)["weight"], alone.weight)
