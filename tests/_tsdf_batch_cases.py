"""Groups of sequences for the batched TSDF fusion tests (hotrack_amd.sdf.tsdf_integrate_batch, pn2s_tsdf_integrate_batch;
network/models/shape_fusion.VolumeFusionGroup), built from the pieces of tests/_tsdf_cases.py.  Not a test file.

A group is S sequences that share what one launch shares -- res, volume dtype, voxel_scale, image sizes, depth type, seg factor,
flip, trunc, carve_weight, max_weight -- and differ in what a sequence owns: its poses, its number of frames and its prior (the
capsule radius the handed-over volume describes, and the prior weight).  Every sequence is one `_tsdf_cases` case of its own
(`sequence_case`): its inputs come from `_tsdf_cases.build` with the prior swapped, its float64 restatement from `fuse_fp64`,
and both are put where `_tsdf_cases.reference` looks them up, so that `_tsdf_cases.check` -- tolerances, exclusion rule and the
2 % cap -- is applied to a sequence unchanged.

The S = 4 groups have the frame counts (3, 0, 1, 2): sequence 1 sits out.  Sequence 2's one frame is the 'close' pose (part of
the volume behind the camera, part outside the image), sequence 3 ends on 'close2' (the same, off-centre).  The res 5 group has
S = 2: one z tile of 256 for 5 voxels, and the second block of y rows holds one row."""
import numpy as np

import _tsdf_cases as T

COUNTS4 = (3, 0, 1, 2)
_POSES4 = (["front", "side", "top"], [], ["close"], ["oblique", "close2"])
_RADII = (0.03, 0.034, 0.026, 0.038)   # the prior of sequence k: a capsule of this radius (the frames show 0.04)
_PRIOR_W = (1.0, 4.0, 2.0, 8.0)

# name, res, voxel_scale, volume dtype, depth 'f32' / 'u16', seg factor, seg channels, flip, poses per sequence
GROUPS = [
    dict(name="g17_f16_f32_seg1", res=17, scale=0.016, vol="float16", depth="f32", f=1, c=3, flip=False, poses=_POSES4),
    dict(name="g17_f32_u16_seg2", res=17, scale=0.016, vol="float32", depth="u16", f=2, c=3, flip=True, poses=_POSES4),
    dict(name="g33_f16_u16_seg2", res=33, scale=0.008, vol="float16", depth="u16", f=2, c=1, flip=False, poses=_POSES4),
    dict(name="g33_f32_f32_seg1", res=33, scale=0.008, vol="float32", depth="f32", f=1, c=3, flip=True, poses=_POSES4),
    dict(name="g5_f32_f32_S2", res=5, scale=0.06, vol="float32", depth="f32", f=1, c=3, flip=False, poses=(["front", "close"], ["side"])),
]
HW = (24, 32)


def counts(group):
    return tuple(len(p) for p in group["poses"])


def sequence_case(group, k):
    """Sequence k of a group as a `_tsdf_cases` case (None for a sequence without frames)."""
    if not group["poses"][k]:
        return None
    return dict(name="%s/seq%d" % (group["name"], k), res=group["res"], scale=group["scale"], hw=HW, vol=group["vol"], depth=group["depth"],
                f=group["f"], c=group["c"], flip=group["flip"], poses=list(group["poses"][k]), max_w=64.0, carve=1.0,
                prior_w=_PRIOR_W[k], radius=_RADII[k])


def prior_volume(res, scale, trunc, radius, dtype):
    ax = (np.arange(res) - res // 2) * scale
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)
    return np.clip(T.capsule_sdf(g, radius), -trunc, trunc).astype(dtype)


def reference(case):
    """(inputs, V64, W64, compare) of a sequence's case, computed once per process and left where `_tsdf_cases.reference` finds it."""
    hit = T._CACHE.get(case["name"])
    if hit is None:
        a = T.build(case)
        a["volume"] = prior_volume(case["res"], case["scale"], a["trunc"], case["radius"], case["vol"])
        hit = (a,) + T.fuse_fp64(a)
        for x in list(a.values()) + list(hit[1:]):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        T._CACHE[case["name"]] = hit
    return hit


def pack(group, device):
    """The group as tsdf_integrate_batch's arguments -> (args: volumes, weights, voxel_scale, depth, seg, intrinsics, rotation,
    translation, frame_counts; keyword dict; per-sequence (args, kw) of the single entry, None where a sequence sits out).
    The single entry's tensors are copies of their own."""
    import torch
    singles = []
    for k in range(len(group["poses"])):
        case = sequence_case(group, k)
        singles.append(None if case is None else T.to_torch(reference(case)[0], device))
    live = [s for s in singles if s is not None]
    volumes = [None if s is None else s[0][0].clone() for s in singles]
    weights = [None if s is None else s[0][1].clone() for s in singles]
    packed = [torch.cat([s[0][i] for s in live]).contiguous() for i in range(3, 8)]
    kw = live[0][1]
    assert all(s[1] == kw and s[0][2] == live[0][0][2] for s in live)   # what the launch shares
    return (volumes, weights, live[0][0][2], *packed, list(counts(group))), dict(kw), singles
