"""CPU: the case builders of tests/_iknet_kernel_cases.py do what the GPU tests (tests/test_gpu_iknet_fp64.py) rely on -- the
routing weights select exactly, the quaternion table reaches every branch of the kernel's head, the dense cases cancel -- and
the figures that become the head's tolerances are printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _iknet_kernel_cases as C  # noqa: E402


@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("s", [0, 1, 2])
def test_routing_weights_select_exactly(s, camera):
    kp, R, t = C.keypoints(16, 1)
    pack = C.pack_fp32(kp, R, t, camera)
    w, cols = C.routing(s)
    raw = C.forward_fp64(w, pack)[-1]
    assert raw.shape == (16, 60)
    assert (raw == pack[:, cols].astype(np.float64)).all()
    assert (raw == C.routing_expected(pack, s)).all()
    root_bone = np.isin(np.arange(C.KIN), [63, 84, 105])   # keypoint 0 is its own parent: its bone is exactly zero
    assert (pack[:, root_bone] == 0).all() and (pack[:, ~root_bone] != 0).all()
    live = pack[:, ~root_bone]
    if not camera:   # the camera frame's z is positive throughout
        assert ((live > 0).any(0) & (live < 0).any(0)).mean() > 0.9   # both carriers of nearly every column are used in some row


def test_column_sets_cover_the_pack_and_permutations_differ():
    assert set(np.concatenate([C.column_set(s) for s in range(3)])) == set(range(C.KIN))
    assert len(set(C.HID_K)) == 5 and all(k % 2 == 1 for k in C.HID_K)
    for l in range(5):
        assert sorted(C._perm(l)) == list(range(C.HID))
    assert len(set(C.SELECTED)) == 60 and {0, 1023} <= set(C.SELECTED)
    assert set(C.SELECTED % 4) == {0, 1, 2, 3} and {0, 1, 2, 3, 1020, 1021, 1022, 1023} <= set(C.SELECTED)


def test_pack_fp32_is_the_hand_frame_to_rounding():
    kp, R, t = C.keypoints(5, 2)
    for camera in (False, True):
        pack = C.pack_fp32(kp, R, t, camera)
        x = kp.astype(np.float64)
        hf = x * 5 if camera else np.einsum("mba,mkb->mka", R.astype(np.float64), x - t.astype(np.float64).reshape(5, 1, 3)) / 0.2
        want = np.concatenate([hf.transpose(0, 2, 1).reshape(5, 63), (hf - hf[:, C.PARENT]).transpose(0, 2, 1).reshape(5, 63)], 1)
        assert np.abs(pack - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("p", range(6))
def test_bias_cases_deliver_relu_of_the_bias(p):
    kp, R, t = C.keypoints(3, 3)
    w, want = C.bias_case(p)
    raw = C.forward_fp64(w, C.pack_fp32(kp, R, t, False))[-1]
    assert (raw == want.astype(np.float64)[None]).all()
    assert (want > 0).sum() >= 15 and (want == 0).sum() >= 15   # both signs of the bias among the selected neurons


@pytest.mark.parametrize("p", range(7))
def test_dense_cases_cancel(p):
    """At least a quarter of the selected rows have sum |w x| / |sum w x| >= 1e3 (against the activation row they were built
    for), and the routing around the dense layer is exact: the float64 forward of the whole set gives the reference."""
    kp, R, t = C.keypoints(16, 4)
    pack = C.pack_fp32(kp, R, t, False)
    w, ref, bound, ratio = C.dense_case(p, pack)
    raw = C.forward_fp64(w, pack)[-1]
    np.testing.assert_allclose(raw, ref, rtol=1e-12, atol=1e-15)   # two BLAS sum orders of the dense layer, nothing else
    hard = (ratio.max(0) >= 1e3)
    print(f"position {p}: {int(hard.sum())} of 60 rows cancel (ratio >= 1e3), median ratio of those {np.median(ratio.max(0)[hard]):.3g}, "
          f"worst bound {bound.max():.3g}, |ref| max {np.abs(ref).max():.3g}")
    assert hard.sum() >= 15
    cancelling = ref[np.arange(0, 60, 2) % 16, np.arange(0, 60, 2)]
    assert (cancelling > 0).all()   # the ReLU lets the cancelling rows through


def test_quat_table_reaches_every_branch_of_the_head():
    """Counts per branch of the kernel's head.  0 < s < 1e-8 cannot occur in fp32: cw * cw rounds to at most 1 - 2^-24 when it is
    below 1, so the smallest positive 1 - cw^2 is 2^-24 and s >= 2^-12; the den = 1 branch is reached through s == 0 only."""
    table, groups = C.quat_table()
    assert table.shape == (16, 15, 4) and sum(int(m.sum()) for m in groups.values()) == 240
    th, s2, s, cw = C.head_fp32(table)
    n_s2 = int((s2 <= 0).sum())
    n_tiny = int(((s > 0) & (s < 1e-8)).sum())
    n_cw1 = int((np.abs(cw) == 1).sum())
    n_neg = int((table[..., 0] < 0).sum())
    print(f"s2 <= 0: {n_s2}   0 < s < 1e-8: {n_tiny}   |cw| == 1: {n_cw1}   w < 0: {n_neg}   smallest positive s {s[s > 0].min():.3g}")
    assert n_s2 >= 10 and n_tiny == 0 and n_cw1 >= 10 and n_neg >= 60
    assert s[s > 0].min() >= 2.0 ** -12
    assert int(((s2 <= 0) & (table[..., 0] < 0)).sum()) >= 4   # the degenerate branch from both signs of w
    # s2 < 0 cannot occur either: with correctly rounded * + sqrt and /, |q| rounds to no less than |w| (sqrt(fl(w^2)) lies
    # within half a spacing of |w|), so |cw| <= 1 and 1 - cw^2 >= 0; "s2 > 0 ? sqrt : 0" and a bare sqrt agree on every input.
    # A sweep over 2 x 10^5 values of w, alone and with tiny companions, beside the argument:
    w = (1.0 + 1e-5 * np.arange(1, 200001)).astype(np.float32)
    for scale in (1.0, 0.37, 5.3e3, 1e-3):
        for x in (0.0, 1e-5, 3e-4):
            q = np.stack([w * np.float32(scale), np.full_like(w, x * scale), np.zeros_like(w), np.zeros_like(w)], -1)
            assert (C.head_fp32(q)[1] >= 0).all() and (C.head_fp32(-q)[1] >= 0).all()
    assert int((s2 < 0).sum()) == 0
    assert np.isfinite(th).all()
    assert (th[groups["identity"]] == 0).all()
    for row in range(16):   # every launch of the GPU test holds degenerate and generic joints
        assert (s2[row] <= 0).any() or (np.abs(cw[row]) == 1).any() or groups["random"][row].any()


def test_head_restatement_against_fp64():
    """The figures that become the GPU test's tolerances (4 x each)."""
    table, groups = C.quat_table()
    err = np.abs(C.theta_fp32(table).astype(np.float64) - C.theta_fp64(table)).max(-1)
    tol = C.head_tolerances()
    for nm, mask in groups.items():
        print(f"{nm:14s} n {int(mask.sum()):3d}  max |theta_fp32 - theta_fp64| {err[mask].max():.3e}  max |theta| {np.abs(C.theta_fp64(table))[mask].max():.3e}")
        assert tol[nm] == 4 * err[mask].max()
    assert tol["identity"] == 0.0
    assert tol["rung0+"] < 1e-5 < tol["rung4+"]   # one global tolerance would hide a fault at a = 1
    assert np.isfinite(C.theta_fp64(table)).all()
