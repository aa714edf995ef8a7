"""CPU: the torch route of network/models/eval_metrics.py against the IMPORTED reference's eval_part_full and compute_chamfer
(tests/golden/eval_metrics.npz, make_golden_eval.py), and the keys ObjTrackModel_Optimization / HandTrackModel report.

Tolerances (fp32 on both sides):
  flags   exactly equal -- the golden holds no pair within 1e-2 degrees / 1e-4 m of a threshold (checked again here);
  tdiff   1e-6 m;
  rdiff   0.01 degrees: the cosine agrees to a few fp32 ulps (<= 6e-7) and d acos / dx = 1 / sin(theta) <= 115 at
          theta >= 0.5 degrees, so the angle differs by <= 7e-5 rad = 0.004 degrees; below 0.5 degrees acos amplifies rounding
          without bound and only "both <= 0.6 degrees" is required;
  chamfer 1e-5 relative: each distance carries <= ~4 ulp, a 2048-term mean in any order adds <= 11 ulp; 1e-5 is ~80 ulp."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
G = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
MODES = [tuple(int(v) for v in m) for m in G["modes"]]
KEYS = ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")


def mode_case(mi, device="cpu"):
    f = lambda k: torch.from_numpy(G[f"m{mi}_{k}"]).to(device)
    return ({"rotation": f("gt_R"), "translation": f("gt_t")}, {"rotation": f("pred_R"), "translation": f("pred_t")},
            G[f"m{mi}_ref"], G[f"m{mi}_mean"])


def check_pose_metrics(got, ref):
    """got, ref: (T,4) arrays [tdiff, rdiff, 5deg5cm, 10deg10cm]."""
    print("max |tdiff - ref| = %.3g m, max |rdiff - ref| = %.3g deg" % (np.abs(got[:, 0] - ref[:, 0]).max(), np.abs(got[:, 1] - ref[:, 1]).max()))
    assert (got[:, 2:] == ref[:, 2:]).all()
    np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=0, atol=1e-6)
    big = ref[:, 1] >= 0.5
    np.testing.assert_allclose(got[big, 1], ref[big, 1], rtol=0, atol=0.01)
    assert (got[~big, 1] <= 0.6).all() and (ref[~big, 1] <= 0.6).all()


def test_golden_covers_every_mode_and_stays_clear_of_the_thresholds():
    assert sorted(MODES) == sorted([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (-1, 0), (5, 0)])
    for mi in range(len(MODES)):
        ref = G[f"m{mi}_ref"]
        assert ref.shape == (24, 4)
        assert np.abs(ref[:, 1:2] - np.array([5.0, 10.0])).min() > 1e-2 and np.abs(ref[:, 0:1] - np.array([0.05, 0.10])).min() > 1e-4
        assert 0 < ref[:, 2].sum() < 24 and ref[:, 3].sum() < 24  # both outcomes of the accuracy flags occur
    assert G["m8_ref"][:, 1].max() > 169 and G["m8_ref"][:, 1].min() < 0.51


@pytest.mark.parametrize("mi", range(len(MODES)))
def test_torch_route_matches_reference_pose_metrics(mi):
    from models import eval_metrics
    axis, sym = MODES[mi]
    gt, pred, ref, mean = mode_case(mi)
    got = eval_metrics.obj_pose_metrics(gt, pred, axis, bool(sym))
    assert got.shape == (24, 4) and got.dtype == torch.float32
    check_pose_metrics(got.numpy(), ref)
    full = eval_metrics.eval_part_full(gt, pred, axis, bool(sym))
    assert tuple(full) == KEYS
    np.testing.assert_allclose([float(full[k]) for k in KEYS], mean, rtol=1e-5, atol=1e-4)
    # the reference's (T,1,3,3) / (T,1,3,1) layout is accepted as it is
    gt4 = {"rotation": gt["rotation"].reshape(24, 1, 3, 3), "translation": gt["translation"].reshape(24, 1, 3, 1)}
    assert torch.equal(eval_metrics.obj_pose_metrics(gt4, pred, axis, bool(sym)), got)


def test_flips_are_the_minimisers_where_the_golden_says_so():
    """In the box / bottle modes some pairs sit near a flipped copy: their symmetric error is far below the plain angle."""
    from models import eval_metrics
    for mi, (axis, _) in enumerate(MODES):
        if axis not in (3, -1):
            continue
        gt, pred, ref, _ = mode_case(mi)
        plain = eval_metrics.obj_pose_metrics(gt, pred, 5, False)[:, 1].numpy()
        assert (plain >= ref[:, 1] - 0.01).all() and (plain - ref[:, 1] > 30).sum() >= 4


def test_torch_route_matches_reference_chamfer():
    from models import eval_metrics
    f = lambda k: torch.from_numpy(G["cf_" + k])
    got = eval_metrics.posed_chamfer(f("A"), f("B"), f("Ra"), f("ta"), f("Rb"), f("tb")).numpy()
    print("chamfer rel. err:", np.abs(got / G["cf_ref"] - 1).max())
    np.testing.assert_allclose(got, G["cf_ref"], rtol=1e-5, atol=0)
    eye, zero = torch.eye(3)[None], torch.zeros(1, 3)
    raw = eval_metrics.posed_chamfer(f("A"), f("B"), eye, zero, eye, zero).numpy()
    np.testing.assert_allclose(raw, G["cf_raw"], rtol=1e-5, atol=0)


def test_torch_route_chunks_over_frames(monkeypatch):
    from models import eval_metrics
    f = lambda k: torch.from_numpy(G["cf_" + k])
    whole = eval_metrics.posed_chamfer(f("A"), f("B"), f("Ra"), f("ta"), f("Rb"), f("tb"))
    monkeypatch.setattr(eval_metrics, "CHUNK_FLOATS", 512 * 384 * 3 * 2)  # two frames per chunk
    assert torch.equal(eval_metrics.posed_chamfer(f("A"), f("B"), f("Ra"), f("ta"), f("Rb"), f("tb")), whole)
    assert eval_metrics.posed_chamfer(f("A"), f("B"), f("Ra")[:0], f("ta")[:0], f("Rb")[:0], f("tb")[:0]).shape == (0,)
    with pytest.raises(ValueError, match="empty cloud"):
        eval_metrics.posed_chamfer(f("A")[:0], f("B"), f("Ra"), f("ta"), f("Rb"), f("tb"))
    same = eval_metrics.posed_chamfer(f("A"), f("A"), f("Ra"), f("ta"), f("Ra"), f("ta"))
    assert (same == 0).all()


def test_forced_kernel_route_refuses_cpu_tensors_and_fallback_is_said_once(capsys):
    from models import eval_metrics
    gt, pred, _, _ = mode_case(0)
    with pytest.raises(RuntimeError, match="kernel route needs fp32 GPU tensors"):
        eval_metrics.obj_pose_metrics(gt, pred, 0, False, route="kernel")
    eval_metrics._said.clear()
    capsys.readouterr()
    eval_metrics.obj_pose_metrics(gt, pred, 0, False)
    eval_metrics.obj_pose_metrics(gt, pred, 0, False)
    assert capsys.readouterr().out.count("the torch route runs") == 1


def test_eval_frame_change_is_the_references():
    """R <- R R_c^T, t <- t - R T_c with the new R (reference track_network.py:417-425)."""
    from models import eval_metrics
    gt, _, _, _ = mode_case(8)
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Rc, Tc = torch.from_numpy(q.astype(np.float32)), torch.from_numpy(rng.uniform(-0.05, 0.05, 3).astype(np.float32))
    out = eval_metrics.to_eval_frame(gt, {"rotation": Rc, "translation": Tc})
    R64, t64 = gt["rotation"].double().numpy(), gt["translation"].double().numpy()
    R2 = R64 @ q.astype(np.float32).astype(np.float64).T
    np.testing.assert_allclose(out["rotation"].numpy(), R2, atol=1e-6)
    np.testing.assert_allclose(out["translation"].numpy(), t64 - R2 @ Tc.double().numpy(), atol=1e-6)


def test_synthetic_sequences_carry_model_points_without_disturbing_the_other_draws():
    from datasets.synthetic import SyntheticObjectSequences, capsule_surface, model_points
    cfg = {"num_points": 64, "obj_category": ["bottle"]}
    seq = SyntheticObjectSequences(cfg, 1, 2, res=11, stride=0.04)[0]
    mp = seq[0]["obj_model_points"]
    assert mp.shape == (2048, 3) and mp.dtype == torch.float32 and "obj_model_points" not in seq[1]
    assert torch.equal(mp, model_points(70_000))
    z = mp[:, 2].clamp(-0.07, 0.07)  # noise-free: on the capsule surface
    np.testing.assert_allclose(((mp[:, :2] ** 2).sum(-1) + (mp[:, 2] - z) ** 2).sqrt().numpy(), 0.04, atol=1e-6)
    # the first frame's cloud is still the first draw of the sequence's own generator after the pose draws
    rng = np.random.default_rng(40_000)
    from datasets.synthetic import _rot
    R = _rot(rng.standard_normal(3), rng.uniform(0, np.pi))
    t = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, 3)
    rng.standard_normal(3), rng.normal(0, 0.01), rng.normal(0, 0.002, 3)
    pts = capsule_surface(rng, 64) @ R.T + t
    np.testing.assert_allclose(seq[0]["obj_points"][0].numpy(), pts.astype(np.float32), atol=0)


class _Opt:
    """ObjTrackModel_Optimization without its optimiser (compute_loss does not use it): CPU tensors, the torch route."""

    def __new__(cls, sym=-1):
        from models.track_network import ObjTrackModel_Optimization
        m = ObjTrackModel_Optimization.__new__(ObjTrackModel_Optimization)
        torch.nn.Module.__init__(m)
        m.device, m.sym = torch.device("cpu"), sym
        return m


def _tracked_sequence(with_points, n_model=300):
    gt, pred, _, _ = mode_case(7)  # the bottle mode
    seq, rets = [], []
    for k in range(6):
        seq.append({"gt_obj_pose": {"rotation": gt["rotation"][k].reshape(1, 1, 3, 3), "translation": gt["translation"][k].reshape(1, 1, 3, 1)}})
        rets.append({"rotation": pred["rotation"][k].reshape(1, 3, 3), "translation": pred["translation"][k].reshape(1, 3, 1)})
    if with_points:
        seq[0]["obj_model_points"] = torch.from_numpy(G["cf_A"][:n_model])
    return seq, rets


def test_obj_track_compute_loss_reports_the_reference_keys():
    from models import eval_metrics
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    seq, rets = _tracked_sequence(False)
    base, _ = _Opt().compute_loss(seq, rets, flags)
    assert list(base) == ["obj_pred_r_diff", "obj_pred_axis_diff", "obj_pred_t_diff", *KEYS]
    ref = G["m7_ref"][:6]
    np.testing.assert_allclose([base[k] for k in KEYS], ref.mean(0), rtol=1e-5, atol=0.01)
    # the three figures of before, computed as before
    r = a = t = 0.0
    for d, ret in zip(seq, rets):
        gR, gt = d["gt_obj_pose"]["rotation"].reshape(3, 3), d["gt_obj_pose"]["translation"].reshape(3)
        R, tt = ret["rotation"].reshape(3, 3), ret["translation"].reshape(3)
        r = r + torch.rad2deg(torch.arccos((((R.t() @ gR).diagonal().sum() - 1) / 2).clamp(-1, 1)))
        a = a + torch.rad2deg(torch.arccos((R[:, 2] * gR[:, 2]).sum().clamp(-1, 1)))
        t = t + (tt - gt).norm()
    assert (base["obj_pred_r_diff"], base["obj_pred_axis_diff"], base["obj_pred_t_diff"]) == (float(r) / 6, float(a) / 6, float(t) / 6)

    seq, rets = _tracked_sequence(True)
    full, _ = _Opt().compute_loss(seq, rets, flags)
    assert list(full) == [*base, "raw_obj_chamfer(mm)", "pred_obj_chamfer(mm)"]
    assert all(full[k] == base[k] for k in base) and all(np.isfinite(v) for v in full.values())
    assert full["raw_obj_chamfer(mm)"] == 0.0  # the predicted cloud defaults to the model points
    A = seq[0]["obj_model_points"]
    want = eval_metrics.posed_chamfer(A, A, torch.from_numpy(G["m7_gt_R"][:6]), torch.from_numpy(G["m7_gt_t"][:6]),
                                      torch.from_numpy(G["m7_pred_R"][:6]), torch.from_numpy(G["m7_pred_t"][:6])).mean() * 1000
    assert full["pred_obj_chamfer(mm)"] == pytest.approx(float(want), rel=1e-6)
    # a reconstruction of its own, the symmetry mode, up_and_down_sym and the evaluation frame are read from the sequence
    seq[0]["obj_recon_points"] = torch.from_numpy(G["cf_B"][:200])
    recon, _ = _Opt().compute_loss(seq, rets, flags)
    assert recon["raw_obj_chamfer(mm)"] > 1.0
    seq2, rets2 = _tracked_sequence(False)
    for d in seq2:
        d["gt_obj_pose"]["up_and_down_sym"] = torch.tensor([True])
    sym, _ = _Opt(sym=2).compute_loss(seq2, rets2, flags)
    gt, pred, _, _ = mode_case(7)
    want = eval_metrics.obj_pose_metrics({k: v[:6] for k, v in gt.items()}, {k: v[:6] for k, v in pred.items()}, 2, True).mean(0)
    np.testing.assert_allclose([sym[k] for k in KEYS], want.numpy(), rtol=1e-6)
    seq3, rets3 = _tracked_sequence(False)
    seq3[0]["eval_frame"] = {"rotation": torch.eye(3), "translation": torch.tensor([0.0, 0.0, 0.03])}
    moved, _ = _Opt().compute_loss(seq3, rets3, flags)
    assert moved["rdiff_0"] == pytest.approx(base["rdiff_0"], abs=1e-4) and moved["tdiff_0"] != base["tdiff_0"]
    assert moved["obj_pred_t_diff"] == base["obj_pred_t_diff"]


def test_missing_model_points_are_said_once(capsys):
    from models.track_network import ObjTrackModel_Optimization
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    ObjTrackModel_Optimization._said_no_points = False
    seq, rets = _tracked_sequence(False)
    _Opt().compute_loss(seq, rets, flags)
    _Opt().compute_loss(seq, rets, flags)
    assert capsys.readouterr().out.count("no 'obj_model_points'") == 1


def test_hand_track_compute_loss_adds_the_obj_pred_block():
    from models.track_network import HandTrackModel

    class Net(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()

        def compute_loss(self, data, ret, flags):
            return {"hand_pred_kp_diff": torch.tensor(0.25)}, ret

    gt, pred, ref, _ = mode_case(7)
    seq = [{"gt_obj_pose": {"rotation": gt["rotation"][k][None], "translation": gt["translation"][k].reshape(1, 3, 1)},
            "pred_obj_pose": {"rotation": pred["rotation"][k][None], "translation": pred["translation"][k].reshape(1, 3, 1)}} for k in range(8)]
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    plain, _ = HandTrackModel({"device": "cpu"}, Net).compute_loss(seq, [{}] * 8, flags)
    assert plain == {"hand_pred_kp_diff": 0.25}
    loss, _ = HandTrackModel({"device": "cpu", "use_pred_obj_pose": True, "obj_sym": -1}, Net).compute_loss(seq, [{}] * 8, flags)
    assert list(loss) == ["hand_pred_kp_diff", *["obj_pred_" + k for k in KEYS]]
    np.testing.assert_allclose([loss["obj_pred_" + k] for k in KEYS], ref[:8].mean(0), rtol=1e-5, atol=0.01)
    for d in seq[3:]:
        del d["pred_obj_pose"]  # frames without a supplied pose: unchanged output
    assert HandTrackModel({"device": "cpu", "use_pred_obj_pose": True}, Net).compute_loss(seq, [{}] * 8, flags)[0] == plain
