"""GPU: the kernel route of the sequence evaluation (hotrack_amd/csrc/seq_eval.hip through network/models/eval_metrics.py)
against the IMPORTED reference (tests/golden/eval_metrics.npz, tolerances of tests/test_eval_metrics.py) and against an fp64
torch evaluation at shapes that cover partial tiles, several LDS chunks and many frames; determinism, graph capture, and the
keys the two tracking models and the objopt entry point report."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
MODES = [tuple(int(v) for v in m) for m in G["modes"]]
KEYS = ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")
NEW_LINES = ("rdiff_0", "tdiff_0", "5deg5cm_0", "10deg10cm_0", "raw_obj_chamfer(mm)", "pred_obj_chamfer(mm)")


def _rotations(rng, T, max_angle=np.pi):
    ax = rng.standard_normal((T, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    ang = rng.uniform(0, max_angle, T)
    K = np.zeros((T, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)


def _case(seed, N, M, T):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 0.05, (N, 3)).astype(np.float32)
    B = rng.normal(0, 0.05, (M, 3)).astype(np.float32)
    Ra = _rotations(rng, T).astype(np.float32)
    Rb = (Ra @ _rotations(rng, T, 0.3)).astype(np.float32)
    ta = (np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, (T, 3))).astype(np.float32)
    tb = (ta + rng.normal(0, 0.005, (T, 3))).astype(np.float32)
    return [torch.from_numpy(x).cuda() for x in (A, B, Ra, ta, Rb, tb)]


def _chamfer_fp64(A, B, Ra, ta, Rb, tb):
    """The reference's expression in fp64 from the same fp32 inputs: the (c, M, N, 3) difference tensor and its norm, a few
    frames at a time (at most 2^25 doubles, 256 MB, per chunk).  Plain elementwise operations and reductions on purpose:
    torch.cdist takes one workgroup per distance, and 8 frames of 2048 x 2048 distances are more workgroups than one launch
    may hold."""
    A, B, Ra, ta, Rb, tb = (x.double() for x in (A, B, Ra, ta, Rb, tb))
    frames = max(1, (1 << 25) // (A.shape[0] * B.shape[0] * 3))
    out = []
    for f0 in range(0, Ra.shape[0], frames):
        pa = A @ Ra[f0:f0 + frames].transpose(-1, -2) + ta[f0:f0 + frames, None]
        pb = B @ Rb[f0:f0 + frames].transpose(-1, -2) + tb[f0:f0 + frames, None]
        d = (pa[:, None, :, :] - pb[:, :, None, :]).square().sum(-1).sqrt()  # (c,M,N)
        out.append(d.min(1)[0].mean(-1) + d.min(2)[0].mean(-1))
    return torch.cat(out)


@pytest.mark.parametrize("mi", range(len(MODES)))
def test_kernel_route_matches_reference_pose_metrics(mi):
    from models import eval_metrics
    from test_eval_metrics import check_pose_metrics, mode_case
    axis, sym = MODES[mi]
    gt, pred, ref, mean = mode_case(mi, "cuda")
    got = eval_metrics.obj_pose_metrics(gt, pred, axis, bool(sym), route="kernel")
    assert got.shape == (24, 4) and got.is_cuda
    check_pose_metrics(got.cpu().numpy(), ref)
    assert torch.equal(eval_metrics.obj_pose_metrics(gt, pred, axis, bool(sym)), got)  # fp32 GPU tensors take the kernel route
    full = eval_metrics.eval_part_full(gt, pred, axis, bool(sym))
    np.testing.assert_allclose([float(full[k]) for k in KEYS], mean, rtol=1e-5, atol=1e-4)
    torch_route = eval_metrics.obj_pose_metrics(gt, pred, axis, bool(sym), route="torch").cpu().numpy()
    check_pose_metrics(torch_route, ref)


def test_kernel_route_matches_reference_chamfer():
    from models import eval_metrics
    f = lambda k: torch.from_numpy(G["cf_" + k]).cuda()
    got = eval_metrics.posed_chamfer(f("A"), f("B"), f("Ra"), f("ta"), f("Rb"), f("tb"), route="kernel").cpu().numpy()
    print("chamfer rel. err vs reference:", np.abs(got / G["cf_ref"] - 1).max())
    np.testing.assert_allclose(got, G["cf_ref"], rtol=1e-5, atol=0)
    eye, zero = torch.eye(3, device="cuda")[None], torch.zeros(1, 3, device="cuda")
    raw = eval_metrics.posed_chamfer(f("A"), f("B"), eye, zero, eye, zero).cpu().numpy()
    np.testing.assert_allclose(raw, G["cf_raw"], rtol=1e-5, atol=0)
    tr = eval_metrics.posed_chamfer(f("A"), f("B"), f("Ra"), f("ta"), f("Rb"), f("tb"), route="torch").cpu().numpy()
    np.testing.assert_allclose(tr, G["cf_ref"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("N,M,T", [(2048, 2048, 1), (2048, 2048, 257), (1, 3000, 4), (777, 2049, 5), (4097, 130, 2)])
def test_kernel_route_matches_fp64(N, M, T):
    from models import eval_metrics
    args = _case(100 + N + M + T, N, M, T)
    got = eval_metrics.posed_chamfer(*args, route="kernel")
    assert got.shape == (T,)
    want = _chamfer_fp64(*args)
    rel = ((got.double() - want).abs() / want).max().item()
    print(f"N {N} M {M} T {T}: max rel. err vs fp64 {rel:.3g}")
    assert rel <= 1e-5
    assert torch.equal(eval_metrics.posed_chamfer(*args, route="kernel"), got)  # two runs bitwise equal


def test_identical_clouds_and_duplicated_points():
    from models import eval_metrics
    A, _, Ra, ta, Rb, tb = _case(7, 1500, 8, 9)
    same = eval_metrics.posed_chamfer(A, A.clone(), Ra, ta, Ra.clone(), ta.clone())
    assert (same == 0).all()  # the same points posed by the same arithmetic: exactly zero
    dup = torch.cat([A, A[:700], A[:1]]).contiguous()  # duplicates change neither nearest distances nor the mean over A
    assert (eval_metrics.posed_chamfer(A, dup, Ra, ta, Ra, ta) == 0).all()
    B = _case(8, 8, 600, 9)[1]
    one = eval_metrics.posed_chamfer(A, B, Ra, ta, Rb, tb)
    two = eval_metrics.posed_chamfer(A, torch.cat([B, B]).contiguous(), Ra, ta, Rb, tb)
    want = _chamfer_fp64(A, B, Ra, ta, Rb, tb)
    assert ((one.double() - want).abs() / want).max() <= 1e-5 and ((two.double() - want).abs() / want).max() <= 1e-5


def test_graph_capture_replays_to_the_eager_result():
    from models import eval_metrics
    args = _case(11, 2048, 1100, 16)
    gt = {"rotation": args[2], "translation": args[3]}
    pred = {"rotation": args[4], "translation": args[5]}
    eager = (eval_metrics.posed_chamfer(*args), eval_metrics.obj_pose_metrics(gt, pred, 3, False))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eval_metrics.posed_chamfer(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = (eval_metrics.posed_chamfer(*args), eval_metrics.obj_pose_metrics(gt, pred, 3, False))
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    # new poses in the captured buffers: the replay evaluates them
    fresh = _case(12, 2048, 1100, 16)
    for dst, src in zip(args[2:], fresh[2:]):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eval_metrics.posed_chamfer(*args))


def test_obj_track_model_reports_every_new_key():
    from models.track_network import ObjTrackModel_Optimization
    from test_track_obj import G as S, _sequence
    cfg = {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False}}
    model = ObjTrackModel_Optimization(cfg)
    model.optimizer.pre_sampled_particle = torch.from_numpy(S["pre"]).cuda()
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    seq = _sequence()
    with torch.no_grad():
        rets = model(seq, flags)
    base, _ = model.compute_loss(seq, rets, flags)
    assert list(base) == ["obj_pred_r_diff", "obj_pred_axis_diff", "obj_pred_t_diff", *KEYS]
    from datasets.synthetic import model_points
    seq[0]["obj_model_points"] = model_points(5, 3000)  # more than 2048: cut by the FPS operator
    seq[0]["obj_recon_points"] = model_points(6, 2048) * 1.01
    full, _ = model.compute_loss(seq, rets, flags)
    assert list(full) == [*base, "raw_obj_chamfer(mm)", "pred_obj_chamfer(mm)"]
    assert all(np.isfinite(v) for v in full.values())
    assert all(full[k] == base[k] for k in base)  # the old keys and the pose metrics do not depend on the model points
    assert 0.5 < full["raw_obj_chamfer(mm)"] < 10 and 0.5 < full["pred_obj_chamfer(mm)"] < 15
    assert full["tdiff_0"] == pytest.approx(full["obj_pred_t_diff"], abs=1e-6)  # the same quantity by both paths
    assert full["rdiff_0"] <= full["obj_pred_r_diff"] + 1e-3                      # the bottle mode can only lower the angle


def test_objopt_entry_point_prints_the_reference_lines(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    import test as test_entry
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    a = p.parse_args(["--config", "objopt_test_HO3D.yml"])
    a.synthetic_frames = 4
    test_entry.main(a)
    out = capsys.readouterr().out
    vals = {}
    for name in NEW_LINES + ("obj_pred_t_diff", "obj_pred_r_diff", "obj_pred_axis_diff"):
        line = [l for l in out.splitlines() if l.startswith(f"Test {name} is ")]
        assert len(line) == 1, name
        vals[name] = float(line[0].split()[-1])
        assert np.isfinite(vals[name])
    assert vals["raw_obj_chamfer(mm)"] == 0.0 and vals["pred_obj_chamfer(mm)"] < 10.0 and vals["tdiff_0"] < 0.01


def test_hand_track_model_reports_the_obj_pred_block():
    from models import eval_metrics
    from models.track_network import HandTrackModel
    from test_eval_metrics import mode_case

    class Net(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()

        def compute_loss(self, data, ret, flags):
            return {"hand_pred_kp_diff": torch.tensor(0.25, device="cuda")}, ret

    gt, pred, ref, _ = mode_case(6, "cuda")  # the box mode
    seq = [{"gt_obj_pose": {"rotation": gt["rotation"][k][None], "translation": gt["translation"][k].reshape(1, 3, 1)},
            "pred_obj_pose": {"rotation": pred["rotation"][k][None], "translation": pred["translation"][k].reshape(1, 3, 1)}} for k in range(24)]
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    cfg = {"device": torch.device("cuda", 0), "use_pred_obj_pose": True, "obj_sym": 3}
    eval_metrics._said.clear()
    loss, _ = HandTrackModel(cfg, Net).compute_loss(seq, [{}] * 24, flags)
    assert not eval_metrics._said  # the kernel route ran
    assert list(loss) == ["hand_pred_kp_diff", *["obj_pred_" + k for k in KEYS]]
    np.testing.assert_allclose([loss["obj_pred_" + k] for k in KEYS], ref.mean(0), rtol=1e-5, atol=0.01)
    assert loss["obj_pred_5deg5cm_0"] == pytest.approx(ref[:, 2].sum() / 24, abs=1e-6)  # flags exact: the mean is a count / 24
    assert loss["obj_pred_10deg10cm_0"] == pytest.approx(ref[:, 3].sum() / 24, abs=1e-6)
