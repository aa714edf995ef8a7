"""CPU: argument validation of the two-problem partition entry (pn2x_sa_class_lists2), of the listed-rows interpolation entry
(pn2x_three_nn_interpolate_pm_rows) and of their bindings ext.sa_class_lists_pair / ext.three_nn_interpolate_pm(rows=...).
Every call is refused before any launch: non-null fake pointers, one violation per call."""
import ctypes

import pytest
import torch

vp, ci = ctypes.c_void_p, ctypes.c_int
P = vp(16)


def test_class_lists2_checks_either_problem(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    lib.pn2x_sa_class_lists2.argtypes = [ci, ci, ci, vp, vp, vp] * 2 + [vp]
    good = (2, 4, 64, P, P, P)
    bad = {
        "b < 0": ((-1, 4, 64, P, P, P), -1),
        "s < 1": ((2, 0, 64, P, P, P), -1),
        "n < 1": ((2, 4, 0, P, P, P), -1),
        "counts null": ((2, 4, 64, None, P, P), -2),
        "list null": ((2, 4, 64, P, None, P), -2),
        "sizes null": ((2, 4, 64, P, P, None), -2),
        "sizes null, empty batch": ((0, 4, 64, None, None, None), -2),
        "list misaligned": ((2, 4, 64, P, vp(20), P), -1),
        "b * s >= 2^24": ((1 << 12, 1 << 12, 64, P, P, P), -3),
        "b * n >= 2^24": ((1 << 12, 4, 1 << 12, P, P, P), -3),
    }
    for name, (args, rc) in bad.items():
        assert lib.pn2x_sa_class_lists2(*args, *good, None) == rc, name + " (first problem)"
        assert lib.pn2x_sa_class_lists2(*good, *args, None) == rc, name + " (second problem)"
    # the one-problem entry keeps the same checks
    lib.pn2x_sa_class_lists.argtypes = [ci, ci, ci, vp, vp, vp, vp]
    for name, (args, rc) in bad.items():
        assert lib.pn2x_sa_class_lists(*args, None) == rc, name


def test_interpolate_rows_entry_checks(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    lib.pn2x_three_nn_interpolate_pm_rows.argtypes = [ci, ci, ci, ci, vp, vp, vp, ci, vp, ci, vp, vp, vp]
    good = dict(b=2, n=64, m=16, c=8, unknown=P, known=P, points=P, ldp=8, out=P, ldo=12, row_list=P, row_counts=P, stream=None)

    def call(**change):
        assert set(change) <= set(good)
        return lib.pn2x_three_nn_interpolate_pm_rows(*{**good, **change}.values())

    assert call(b=-1) == -1 and call(n=-1) == -1
    assert call(m=2) == -1                                  # fewer than three known points
    assert call(c=0) == -1 and call(ldp=4) == -1 and call(ldo=4) == -1
    assert call(b=0) == 0 and call(n=0) == 0                # nothing to do
    for name in ("unknown", "known", "points", "out", "row_list", "row_counts"):
        assert call(**{name: None}) == -2, name
    assert call(b=1 << 16) == -3                            # one grid row per cloud
    assert call(m=4096) == -3                               # the known set must fit one LDS tile
    assert call(c=6, ldp=8) == -3 and call(ldp=10) == -3 and call(ldo=14) == -3   # 16-byte quads
    assert call(points=vp(24)) == -3 and call(out=vp(40)) == -3
    lib.pn2x_three_nn_interpolate_pm_rows_supported.argtypes = [ci] * 6
    ok = lib.pn2x_three_nn_interpolate_pm_rows_supported
    assert ok(1, 7, 5, 4, 4, 12) == 1 and ok(64, 1024, 256, 128, 128, 132) == 1    # no lower bound on the query count
    assert ok(1, 7, 2, 4, 4, 12) == 0 and ok(1, 7, 2049, 4, 4, 12) == 0 and ok(1, 7, 5, 2, 4, 12) == 0


def test_bindings_refuse_wrong_arguments_without_gpu():
    from hotrack_amd import ext
    counts = torch.ones((2, 5), dtype=torch.int32)
    for a, b in ((counts, counts.long()), (counts.long(), counts), (counts.view(-1), counts), (counts, counts.view(1, 2, 5)),
                 (counts, None), (counts.float(), counts)):
        with pytest.raises(TypeError):                      # dtype, rank, not a tensor; and CPU tensors in every case
            ext.sa_class_lists_pair(a, 64, b, 64)
    with pytest.raises(TypeError):
        ext.sa_class_lists_pair(counts, 64, counts, 64)     # well-formed, but not on the GPU
    unknown, known, points, out = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3), torch.zeros(2, 4, 4), torch.zeros(2, 8, 4)
    lst, cnt = torch.zeros((2, 8), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32)
    for rows in (lst, (lst,), (lst, cnt, cnt), (lst, None), "ab", (lst.long(), cnt), (lst, cnt.float())):
        with pytest.raises(TypeError):                      # not the (list, counts) pair of int32 tensors
            ext.three_nn_interpolate_pm(unknown, known, points, out, rows=rows)
    for rows in ((lst[:, :7], cnt), (lst[:1], cnt), (lst, cnt[:, :1]), (lst, cnt[:1]), (lst.view(-1), cnt)):
        with pytest.raises(ValueError):                     # list (B,n) and counts (B,2)
            ext.three_nn_interpolate_pm(unknown, known, points, out, rows=rows)
