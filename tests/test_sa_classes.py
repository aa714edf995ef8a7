"""CPU: the class rule of the fused set-abstraction kernel's class walk (ext.sa_class_partition, the plain-torch statement the
GPU kernel pn2x_sa_class_lists is held to in tests/test_gpu_sa_classes.py) against a numpy statement of it, and the argument
validation of the new C entries (no launch happens)."""
import ctypes

import numpy as np
import pytest
import torch


def _numpy_rule(counts):
    """Centroid ids of class 32 (17..32 hits) ascending, then class 16 (9..16), then class 8 (<= 8), and the three sizes."""
    c = counts.reshape(-1)
    ids = np.arange(c.size)
    parts = [ids[c >= 17], ids[(c >= 9) & (c <= 16)], ids[c <= 8]]
    return np.concatenate(parts), np.array([p.size for p in parts])


@pytest.mark.parametrize("seed", range(4))
def test_class_partition_rule(seed):
    from hotrack_amd import ext
    rng = np.random.default_rng(seed)
    B, S = (1, 1) if seed == 0 else (int(rng.integers(1, 6)), int(rng.integers(1, 300)))
    counts = rng.integers(1, 33, size=(B, S)).astype(np.int32)
    edge = np.array([8, 9, 16, 17, 1, 32], dtype=np.int32)
    counts.reshape(-1)[:min(edge.size, counts.size)] = edge[:counts.size]
    ids, sizes = ext.sa_class_partition(torch.from_numpy(counts))
    ref_ids, ref_sizes = _numpy_rule(counts)
    assert ids.dtype == torch.int32 and sizes.dtype == torch.int32
    assert np.array_equal(ids.numpy(), ref_ids) and np.array_equal(sizes.numpy(), ref_sizes)
    assert sorted(ids.tolist()) == list(range(B * S))  # every centroid exactly once


def test_class_partition_boundaries_and_empty_classes():
    from hotrack_amd import ext
    for counts, sizes in (([8, 8, 8], [0, 0, 3]), ([9, 16], [0, 2, 0]), ([17, 32], [2, 0, 0]), ([8, 9], [0, 1, 1]), ([16, 17], [1, 1, 0])):
        ids, got = ext.sa_class_partition(torch.tensor([counts], dtype=torch.int32))
        assert got.tolist() == sizes
        assert ids.tolist() == _numpy_rule(np.array(counts))[0].tolist()


def test_sa_classes_argument_validation_without_gpu(hip_lib_path):
    """pn2x_sa_mlp_max_classes / pn2x_sa_class_lists / pn2x_ball_query_picks_counts refuse invalid arguments before any launch:
    non-null fake pointers, one violation per call."""
    lib = ctypes.CDLL(hip_lib_path)
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    lib.pn2x_sa_mlp_max_classes.argtypes = [ci] * 7 + [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cl, ci, ci, vp]
    p = vp(16)
    good = dict(b=2, n=64, s=4, k=32, c1=64, c2=64, c3=128, a1f=p, a1f_ld=64, xyz=p, cxyz=p, wx=p, b1=p, cadd=p, cadd_ld=64, idx=p,
                cls_list=p, cls_sizes=p, w2=p, b2=p, w3=p, b3=p, out=p, out_b=512, out_s=128, out_c=1, stream=None)

    def call(**change):
        assert set(change) <= set(good)
        return lib.pn2x_sa_mlp_max_classes(*{**good, **change}.values())

    assert call(b=-1) == -1
    assert call(k=0) == -1
    assert call(s=0) == 0 and call(b=0) == 0               # nothing to do
    assert call(idx=None) == -2
    assert call(cls_list=None) == -2 and call(cls_sizes=None) == -2
    assert call(a1f=None, xyz=None) == -2
    assert call(cxyz=None) == -2
    assert call(a1f_ld=60) == -1 and call(a1f_ld=66) == -1
    assert call(cadd_ld=66) == -1
    assert call(k=16) == -3 and call(k=64) == -3           # ball-query lists of 32 slots only
    assert call(c1=128, c2=128, c3=192, a1f_ld=128, cadd_ld=128) == -3              # the 128-128-192 instance keeps the fixed-K launch
    assert call(cls_list=vp(24)) == -1                     # records are read as 16-byte quads
    assert call(b=1 << 20, n=64) == -3                     # b * n beyond the 24-bit row numbers
    assert call(out_b=1 << 31) == -3                       # the whole output must sit behind one 32-bit offset
    # the first b * n and b * s past the 24-bit row numbers, each the call's only fault (a1f / cadd left out: their whole-tensor
    # byte limits would be passed too)
    assert call(b=1 << 12, n=1 << 12, a1f=None) == -3
    assert call(b=1 << 12, s=1 << 12, cadd=None) == -3
    assert call(out_b=-512) == -3
    for name in ("w2", "b2", "w3", "b3", "out", "wx"):
        assert call(**{name: None}) == -2, name
    for name in ("a1f", "cadd", "b1", "w2", "w3"):
        assert call(**{name: vp(20)}) == -1, name
    assert call(n=0) == -1 and call(s=-1) == -1
    assert call(cadd_ld=60) == -1
    assert call(n=1 << 24) == -3 and call(a1f_ld=1 << 23) == -3
    for k in (8, 16, 31, 32, 33, 64):
        for w in ((32, 32, 64), (64, 64, 128), (128, 128, 192), (64, 64, 64), (32, 32, 128)):
            assert lib.pn2x_sa_mlp_max_classes_supported(k, *w) == int(k == 32 and w in ((32, 32, 64), (64, 64, 128))), (k, w)

    lib.pn2x_sa_class_lists.argtypes = [ci, ci, ci, vp, vp, vp, vp]
    assert lib.pn2x_sa_class_lists(-1, 4, 64, p, p, p, None) == -1
    assert lib.pn2x_sa_class_lists(2, 0, 64, p, p, p, None) == -1
    assert lib.pn2x_sa_class_lists(2, 4, 0, p, p, p, None) == -1
    assert lib.pn2x_sa_class_lists(2, 4, 64, None, p, p, None) == -2
    assert lib.pn2x_sa_class_lists(2, 4, 64, p, None, p, None) == -2
    assert lib.pn2x_sa_class_lists(2, 4, 64, p, p, None, None) == -2
    assert lib.pn2x_sa_class_lists(2, 4, 64, p, vp(20), p, None) == -1
    assert lib.pn2x_sa_class_lists(1 << 12, 1 << 12, 64, p, p, p, None) == -3

    lib.pn2x_ball_query_picks_counts.argtypes = [ci, ci, ci, cf, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    assert lib.pn2x_ball_query_picks_counts(1, 16, 4, 0.1, 0, p, p, p, p, None, 0, p, None) == -1       # nsample < 1
    assert lib.pn2x_ball_query_picks_counts(1, 16, 4, float("nan"), 8, p, p, p, p, None, 0, p, None) == -1
    assert lib.pn2x_ball_query_picks_counts(1, 16, 4, 0.1, 8, None, p, p, p, None, 0, p, None) == -2
    assert lib.pn2x_ball_query_picks_counts(0, 16, 4, 0.1, 8, p, p, p, p, None, 0, p, None) == 0         # empty batch
    lib.pn2x_ball_query_picks_ties_counts.argtypes = [ci, ci, ci, cf, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
    assert lib.pn2x_ball_query_picks_ties_counts(1, 16, 4, 0.1, 8, p, p, p, p, None, 0, 5, p, p, p, None) == -1   # m2 > m
    assert lib.pn2x_ball_query_picks_ties_counts(1, 16, 4, 0.1, 8, p, p, p, p, None, 0, 2, None, p, p, None) == -2
