"""CPU: the torch route of eval_metrics.hand_sequence_metrics and HandTrackModel.compute_loss_batch against the IMPORTED
reference's HandTrackNet.compute_loss driven frame by frame with track_flag set, and its sequence rule
(tests/golden/hand_eval.npz, make_golden_hand_eval.py).

Tolerances against the fixture (fp32 values of an fp32 torch run):
  lengths and L1 columns   2e-6: each term carries about six fp32 roundings of operands <= 2 (<= 7e-7), a mean does not grow it;
  angle columns            5e-3 degrees: every angle of the fixture lies in [1, 179] degrees (checked), where the cosine's rounding
                           (<= 2.4e-7) over sin 1 degree is 8e-4 degrees and the palm fit's adds as much.
The float64 torch route must agree with the fixture at least as closely (the same bounds)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _hand_eval_cases as C  # noqa: E402

G = C.golden()
REFERENCE_ORDER = ["hand_pred_kp_loss", "hand_pred_kp_diff", "hand_init_kp_diff", "hand_pred_r_loss", "hand_pred_t_loss",
                   "hand_init_r_diff", "hand_init_t_diff", "hand_pred_r_diff", "hand_pred_t_diff", "hand_canon_r_diff",
                   "hand_canon_t_diff", "MANO_theta_diff"]


def check(got, ref, keys):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    for i, k in enumerate(keys):
        tol = 5e-3 if k.endswith("_r_diff") else 2e-6
        err = np.abs(got[..., i] - ref[..., i]).max()
        print("%-20s max |diff| = %.3g (bound %.0e)" % (k, err, tol))
        assert err <= tol, (k, err)


def test_fixture_angles_lie_in_the_interior_range():
    for q in (0, 1):
        keys = [str(k) for k in G[f"s{q}_keys"]]
        ang = G[f"s{q}_frames"][:, [i for i, k in enumerate(keys) if k.endswith("_r_diff")]]
        assert ang.min() >= 1.0 and ang.max() <= 179.0
    assert list(G["lengths"]) == [5, 3] and G["s0_frames"].shape == (5, 10) and G["s1_frames"].shape == (3, 11)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("q", [0, 1])
def test_torch_route_reproduces_the_reference(q, dtype):
    from models import eval_metrics
    frames, palm, keys, per_frame, per_seq = C.fixture_frames(G, q, dtype)
    T = per_frame.shape[0]
    rows, seq, got_keys = eval_metrics.hand_sequence_metrics(frames, [0, T], palm=palm)
    assert rows.shape == (T, 12) and seq.shape == (1, 12) and rows.dtype == dtype
    assert got_keys == keys  # the reference's keys, in its order
    cols = [eval_metrics.HAND_METRIC_KEYS.index(k) for k in keys]
    check(rows[:, cols].numpy(), per_frame, keys)
    check(seq[0, cols].numpy(), per_seq, keys)
    absent = [c for c in range(12) if c not in cols]
    assert (rows[:, absent] == 0).all() and (seq[:, absent] == 0).all()


def test_init_columns_are_the_first_frame_and_the_rest_are_means():
    from models import eval_metrics
    assert list(eval_metrics.HAND_METRIC_KEYS) == REFERENCE_ORDER
    assert eval_metrics.HAND_INIT_COLUMNS == (2, 5, 6)
    frames, offsets, palm = C.make_case((3, 0, 1, 6), pose_mode=False, seed=3)
    f64, p64 = C.to(frames, palm, dtype=torch.float64)
    rows, seq, _ = eval_metrics.hand_sequence_metrics(f64, offsets, palm=p64)
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if a == b:
            assert (seq[q] == 0).all()  # a sequence without frames
            continue
        for c in range(12):
            want = rows[a, c] if c in (2, 5, 6) else rows[a:b, c].mean()
            assert abs(float(seq[q, c] - want)) < 1e-12
    # every sequence's values are those of the sequence evaluated alone
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if a == b:
            continue
        alone, alone_seq, _ = eval_metrics.hand_sequence_metrics({k: v[a:b] for k, v in f64.items()}, [0, b - a], palm=p64[q:q + 1])
        assert torch.allclose(alone, rows[a:b], rtol=0, atol=1e-12) and torch.allclose(alone_seq[0], seq[q], rtol=0, atol=1e-12)


@pytest.mark.parametrize("pose_mode,with_gt,with_theta", [(False, False, False), (False, True, False), (False, False, True),
                                                           (False, True, True), (True, True, False), (True, True, True)])
def test_keys_and_validity_follow_the_inputs(pose_mode, with_gt, with_theta):
    from models import eval_metrics
    frames, offsets, palm = C.make_case((2, 3), pose_mode, with_gt, with_theta, seed=4)
    rows, seq, keys = eval_metrics.hand_sequence_metrics(frames, offsets, palm=palm)
    want = [k for k in REFERENCE_ORDER if not ((pose_mode and k in ("hand_init_r_diff", "hand_init_t_diff"))
                                               or (not with_gt and k.startswith("hand_canon")) or (not with_theta and k == "MANO_theta_diff"))]
    assert keys == want
    for c, k in enumerate(REFERENCE_ORDER):
        if k in keys:
            assert (rows[2:, c] != 0).all(), k  # (frames 0 and 1 are built to sit at 0 / 180 degrees)
        else:
            assert (rows[:, c] == 0).all() and (seq[:, c] == 0).all(), k


def test_empty_inputs_and_bad_offsets():
    from models import eval_metrics
    frames, offsets, palm = C.make_case((0, 0), False, seed=5)
    rows, seq, keys = eval_metrics.hand_sequence_metrics(frames, offsets, palm=palm)
    assert rows.shape == (0, 12) and seq.shape == (2, 12) and (seq == 0).all() and len(keys) == 12
    frames, offsets, palm = C.make_case((2, 3), False, seed=5)
    for bad in ([0, 2], [1, 2, 5], [0, 3, 2, 5], [0, 2, 6], []):
        with pytest.raises(ValueError):
            eval_metrics.hand_sequence_metrics(frames, bad, palm=palm[:max(len(bad) - 1, 0)])
    with pytest.raises(ValueError):  # Kabsch mode without a template per sequence
        eval_metrics.hand_sequence_metrics(frames, offsets, palm=palm[:1])
    with pytest.raises(RuntimeError):  # the kernel route is never a silent fall-back
        eval_metrics.hand_sequence_metrics(frames, offsets, palm=palm, route="kernel")


def _model(fused, use_pred_obj_pose=False):
    from _netinit import make_cfg
    from models.hand_network import HandTrackNet
    from models.track_network import HandTrackModel
    cfg = make_cfg("cpu")
    cfg.update(fused_hand_eval=fused, use_pred_obj_pose=use_pred_obj_pose)
    return HandTrackModel(cfg, handnet=HandTrackNet)


def _fixture_io(q):
    frames, palm, keys, per_frame, per_seq = C.fixture_frames(G, q)
    palm_t = torch.from_numpy(G[f"s{q}_palm_template"])
    gt_theta = torch.from_numpy(G[f"s{q}_gt_mano_pose"]) if q == 0 else None
    data, rets = C.tracker_io(frames, palm_t, gt_theta=gt_theta)
    return data, rets, keys, per_frame, per_seq


def test_compute_loss_batch_equals_the_reference_per_sequence():
    model = _model(fused=True)
    ios = [_fixture_io(q) for q in (0, 1)]
    flags = {"track_flag": True, "test_flag": True, "save_flag": True, "IKNet_flag": True}
    out = model.compute_loss_batch([io[0] for io in ios], [io[1] for io in ios], flags)
    assert len(out) == 2
    for (loss, rets), (data, rets_in, keys, per_frame, per_seq) in zip(out, ios):
        assert list(loss) == keys and rets is rets_in
        assert all(isinstance(v, float) for v in loss.values())
        check([loss[k] for k in keys], per_seq, keys)
        table = rets[0]["frame_errors"]  # kp_error, r_error, t_error per frame
        assert table.shape == (len(data), 3) and table.device.type == "cpu"
        names = ["hand_pred_kp_diff", "hand_pred_r_diff", "hand_pred_t_diff"]
        check(table.numpy(), per_frame[:, [keys.index(k) for k in names]], names)
        assert all(r["gt_kp_handframe"].shape == (1, 3, 21) for r in rets)
    # one sequence through compute_loss with the switch on: the same dictionary; without save_flag no table and no gt_kp_handframe
    data, rets, keys, _, per_seq = _fixture_io(1)
    loss, _ = model.compute_loss(data, rets, dict(flags, save_flag=False))
    assert list(loss) == keys and "frame_errors" not in rets[0] and rets[0]["gt_kp_handframe"] is None
    check([loss[k] for k in keys], per_seq, keys)


def test_compute_loss_batch_reports_the_object_block_after_the_hand_keys():
    model = _model(fused=True, use_pred_obj_pose=True)
    data, rets, keys, _, _ = _fixture_io(0)
    rng = np.random.default_rng(1)
    for d in data:
        R = torch.from_numpy(C.rot(rng.standard_normal(3), 0.7).astype(np.float32))
        d["gt_obj_pose"] = {"rotation": R.reshape(1, 3, 3), "translation": torch.tensor([[0.0], [0.0], [0.5]]).reshape(1, 3, 1)}
        d["pred_obj_pose"] = {"rotation": (R @ torch.from_numpy(C.rot([0, 0, 1.0], 0.05).astype(np.float32))).reshape(1, 3, 3),
                              "translation": torch.tensor([[0.01], [0.0], [0.5]]).reshape(1, 3, 1)}
    flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": True}
    loss, _ = model.compute_loss_batch([data], [rets], flags)[0]
    assert list(loss) == keys + ["obj_pred_tdiff_0", "obj_pred_rdiff_0", "obj_pred_5deg5cm_0", "obj_pred_10deg10cm_0"]
    old, _ = _model(fused=False, use_pred_obj_pose=True).compute_loss(data, rets, flags)
    for k in loss:
        if k.startswith("obj_pred_"):
            assert loss[k] == old[k]


def test_switch_off_is_the_existing_per_frame_loop():
    """cfg['fused_hand_eval'] unset: compute_loss is the per-frame loop over HandTrackNet.compute_loss, value for value."""
    model = _model(fused=False)
    assert model.fused_hand_eval is False
    for q in (0, 1):
        data, rets, keys, _, per_seq = _fixture_io(q)
        flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": q == 0}
        got, _ = model.compute_loss(data, rets, flags)
        total = {}
        for d, r in zip(data, rets):
            loss, _ = model.handnet.compute_loss(d, r, flags)
            for k, v in loss.items():
                total[k] = total[k] + v if k in total else v
        want = {k: float(v) / len(data) for k, v in total.items()}
        assert got == want and list(got) == list(want)
        assert "MANO_theta_diff" not in got and "frame_errors" not in rets[0]
        # ... and it is the mean where the new route reports the first frame
        new, _ = _model(fused=True).compute_loss(data, rets, flags)
        k = "hand_init_kp_diff"
        assert abs(new[k] - per_seq[keys.index(k)]) <= 2e-6 and abs(got[k] - new[k]) > 1e-4


def test_unsupported_sequences_use_the_existing_loop(capsys):
    model = _model(fused=True)
    model.handnet.handframe = "OBB"
    data, rets, keys, _, _ = _fixture_io(1)
    flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": False}
    loss, _ = model.compute_loss(data, rets, flags)
    assert "OBB" in capsys.readouterr().out
    want, _ = model._compute_loss_frames(data, rets, flags)
    assert loss == want and "hand_pred_r_diff" not in loss


def test_command_line_switch():
    import argparse
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    assert p.parse_args([]).fused_hand_eval is None
    assert p.parse_args(["--fused_hand_eval"]).fused_hand_eval is True
