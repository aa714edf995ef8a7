"""GPU: the IKNet kernel route (hotrack_amd/csrc/iknet.hip through models/iknet.IKNet) against an fp64 evaluation of the same
module and against the reference (tests/golden/iknet_reference.npz), its determinism and graph capture, the torch fallback
above 16 rows, IKNet in the tracking loop (optimisation on and off), the train.py / test.py entry points, and learning."""
import argparse
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

from _iknet_cases import load_into  # noqa: E402
from models.hand_model import SyntheticLBSHand  # noqa: E402
from models.iknet import PARENT, IKNet, quat2axisang  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "iknet_reference.npz"))
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}
TRACK = {"track_flag": True, "opt_flag": True}


def _net(frame="kp", hm=None):
    m = IKNet({"device": "cuda", "network": {"iknetframe": frame}}, hand_model=hm)
    load_into(m)
    return m.cuda().eval()


def _kp(M, seed):
    hm = SyntheticLBSHand()
    rng = np.random.default_rng(seed)
    glob = rng.normal(0, 1.0, (M, 3))
    pose = rng.uniform(-0.5, 0.5, (M, 45))
    with torch.no_grad():
        _, kp = hm.forward(th_pose_coeffs=torch.from_numpy(np.concatenate([glob, pose], 1)).float(),
                           th_trans=torch.from_numpy(np.array([0, 0, 0.5]) + rng.uniform(-0.1, 0.1, (M, 3))).float())
        _, rest = hm.forward(th_pose_coeffs=torch.zeros(1, 48), th_trans=torch.zeros(1, 3))
    return kp.cuda(), rest[:, [0, 1, 5, 9, 13, 17]].cuda()


def _fp64(m, kp, R, t, frame):
    """The same module in float64 on the CPU, from the kernel route's palm fit (R, t)."""
    kp, R, t = kp.double().cpu(), R.double().cpu(), t.double().cpu()
    x = kp.transpose(-1, -2)
    hf = torch.matmul(R.transpose(-1, -2), x - t) / 0.2 if frame == "kp" else x * 5
    B = kp.shape[0]
    h = torch.cat([hf.reshape(B, -1), (hf - hf[..., PARENT]).reshape(B, -1)], -1)
    m64 = copy.deepcopy(m).double().cpu().eval()
    with torch.no_grad():
        for i in range(6):
            h = torch.relu(m64.bn[i](m64.linear[i](h)))
        return m64.linear[6](h), hf


@pytest.mark.parametrize("frame", ["kp", "camera"])
@pytest.mark.parametrize("M", [1, 2, 5, 16])
def test_kernel_matches_fp64(M, frame):
    """Bound: an fp32 dot product of length K carries at most ~K u |w|.|x| of rounding error (u = 2^-24); with He-scaled
    weights and folded BatchNorm the activations stay O(1) and the errors of the seven layers add, so 1e-4 x the output scale
    (max |raw_quat|) bounds raw_quat with margin (K = 1024: K u = 6.1e-5 per layer in the worst case, ~sqrt(K) u typical)."""
    from hotrack_amd import pointnet2_hip
    m = _net(frame)
    kp, palm = _kp(M, 10 + M)
    pointnet2_hip.PROFILE = []
    try:
        with torch.no_grad():
            raw, theta, canon, hf = m.solve(kp, palm)
        assert "iknet_forward" in [p[0] for p in pointnet2_hip.PROFILE]
    finally:
        pointnet2_hip.PROFILE = None
    ref, hf64 = _fp64(m, kp, canon["rotation"], canon["translation"], frame)
    scale = float(ref.abs().max())
    np.testing.assert_allclose(raw.cpu().double().numpy(), ref.numpy(), rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(hf.cpu().double().numpy(), hf64.numpy(), rtol=0, atol=1e-5 * float(hf64.abs().max()))
    th64 = quat2axisang(ref)
    ok = (torch.sqrt(torch.clamp(1 - (ref.reshape(M, 15, 4)[..., 0] / ref.reshape(M, 15, 4).norm(dim=-1)) ** 2, min=0)) > 1e-3)
    ok = ok.repeat_interleave(3, dim=1)  # away from the degenerate angles (covered by the helper cases)
    assert ok.float().mean() > 0.9
    np.testing.assert_allclose(theta.cpu().double()[ok].numpy(), th64[ok].numpy(), rtol=0, atol=2e-3)


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("frame", ["kp", "camera"])
def test_kernel_matches_the_reference(B, frame):
    m = _net(frame)
    for pname in ("zero", "shaped"):
        key = f"B{B}_{frame}_{pname}"
        data = {"baseline_pred_kp": torch.from_numpy(G[f"B{B}_kp"]).cuda(), "pred_palm_template": torch.from_numpy(G[f"palm_{pname}"]).cuda()}
        with torch.no_grad():
            r = m(data, dict(TRACK))
        scale = float(np.abs(G[f"{key}_raw_quat"]).max())
        np.testing.assert_allclose(r["raw_quat"].cpu().numpy(), G[f"{key}_raw_quat"], rtol=0, atol=2e-4 * scale)
        np.testing.assert_allclose(r["MANO_theta"].cpu().numpy(), G[f"{key}_MANO_theta"], rtol=0, atol=2e-3)
        np.testing.assert_allclose(r["global_pose"]["rotation"].cpu().numpy(), G[f"{key}_R"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(r["init_kp_handframe"].cpu().numpy(), G[f"{key}_init_kp_handframe"], rtol=0, atol=1e-5)


def test_kernel_is_deterministic_and_graph_capturable():
    m = _net("kp")
    kp, palm = _kp(8, 3)
    with torch.no_grad():
        a = m.solve(kp, palm)
        b = m.solve(kp, palm)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
        static = kp.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.solve(static, palm)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.solve(static, palm)
        kp2, _ = _kp(8, 4)
        for k in (kp, kp2):
            static.copy_(k)
            graph.replay()
            want = m.solve(k, palm)
            torch.cuda.synchronize()
            assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


def test_more_than_16_rows_take_the_torch_route():
    from hotrack_amd import pointnet2_hip
    m = _net("kp")
    kp, palm = _kp(17, 5)
    pointnet2_hip.PROFILE = []
    try:
        with torch.no_grad():
            raw, theta, canon, _ = m.solve(kp, palm)
        assert "iknet_forward" not in [p[0] for p in pointnet2_hip.PROFILE]
    finally:
        pointnet2_hip.PROFILE = None
    with torch.no_grad():
        raw16 = m.solve(kp[:16], palm)[0]
    scale = float(raw.abs().max())
    np.testing.assert_allclose(raw[:16].cpu().numpy(), raw16.cpu().numpy(), rtol=0, atol=1e-4 * scale)
    m.use_kernel = False
    with torch.no_grad():
        torch_raw = m.solve(kp[:16], palm)[0]
    np.testing.assert_allclose(torch_raw.cpu().numpy(), raw16.cpu().numpy(), rtol=0, atol=1e-4 * scale)


@pytest.fixture(autouse=True)
def _no_fused_handnet():
    """The oracle 'HandTrackNet' below is not graph-capturable: keep HandTrackModel from capturing it when an earlier test left
    the fused backend set (IKNet's own graph does not depend on it)."""
    from models import pointnet_utils
    prev = pointnet_utils.fused_backend()
    pointnet_utils.set_fused_backend(None)
    yield
    pointnet_utils.set_fused_backend(prev)


class _OracleNet(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.device = cfg["device"]

    def forward(self, data, flags):
        kp = data["gt_hand_kp"].to(self.device).float() + 0.002
        return {"pred_kp": kp, "pred_kp_vis_mask": torch.ones(1, 21, dtype=torch.bool, device=self.device)}


def _sequence(frames, use_opt):
    from datasets.synthetic import SyntheticHandObjectSequences
    hm = SyntheticLBSHand()
    cfg = {"device": torch.device("cuda"), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
           "use_optimization": use_opt, "hand_particles": 256, "hand_model": hm, "opt": {"energy_weight": dict(ENERGY_WEIGHT)},
           "network": {"iknetframe": "kp"}}
    return cfg, hm, SyntheticHandObjectSequences(cfg, 1, frames)[0]


def test_tracking_seeds_the_optimiser_with_iknet():
    from models.track_network import HandTrackModel
    cfg, hm, seq = _sequence(3, True)
    ik = _net("kp", hm)
    model = HandTrackModel(cfg, handnet=_OracleNet, IKnet=ik, hand_model=hm).eval()
    seen = []
    orig = model.optimizer.optimize

    def spy(theta0, pose0, kp, *a, **k):
        seen.append((theta0.clone(), {kk: v.clone() for kk, v in pose0.items()}, kp.clone()))
        return orig(theta0, pose0, kp, *a, **k)
    model.optimizer.optimize = spy
    with torch.no_grad():
        rets = model(seq, {"track_flag": True, "test_flag": True, "save_flag": False})
    assert len(seen) == 3
    palm = seq[0]["gt_hand_pose"]["palm_template"].cuda().float()
    for (theta0, pose0, kp), r in zip(seen, rets):
        with torch.no_grad():
            _, theta, canon, _ = ik.solve(kp, palm)
        assert torch.equal(theta0, theta)
        assert torch.equal(pose0["rotation"], canon["rotation"]) and torch.equal(pose0["translation"], canon["translation"])
        assert torch.equal(kp, r["baseline_pred_kp"])
    assert any(k[0] == "iknet" for k in model._graphs)


def test_tracking_without_optimisation_drives_the_hand_model():
    from models.track_network import HandTrackModel
    cfg, hm, seq = _sequence(4, False)
    ik = _net("kp", hm)
    model = HandTrackModel(cfg, handnet=_OracleNet, IKnet=ik, hand_model=hm).eval()
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    with torch.no_grad():
        g = model(copy.deepcopy(seq), dict(flags))
        assert len(model._graphs) == 1
        model.use_graph = False
        e = model(copy.deepcopy(seq), dict(flags))
    for rg, re_ in zip(g, e):
        assert torch.equal(rg["raw_quat"], re_["raw_quat"]) and torch.equal(rg["pred_kp"], re_["pred_kp"])
        coeffs = quat2axisang(torch.cat([__import__("models.rotations", fromlist=["x"]).matrix_to_unit_quaternion(
            re_["global_pose"]["rotation"]), re_["raw_quat"]], 1))
        with torch.no_grad():
            _, kp = hm.forward(th_pose_coeffs=coeffs, th_trans=re_["global_pose"]["translation"].reshape(1, 3))
        assert torch.equal(re_["pred_kp"], kp)
    # a weight change re-captures the IKNet graph
    with torch.no_grad():
        ik.linear[6].bias.add_(0.1)
        model.use_graph = True
        g2 = model(copy.deepcopy(seq), dict(flags))
    assert not torch.equal(g2[0]["raw_quat"], g[0]["raw_quat"])


def test_train_then_track_entry_points(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    import test as test_entry
    import train
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    a = p.parse_args(["--config", "handiknet_train_SimGrasp.yml", "--batch_size", "8", "--total_epoch", "1"])
    a.synthetic_frames, a.max_iters = 32, 3
    setattr(a, "freq/save", 1)
    train.main(a)
    ckpt = os.path.join(str(tmp_path), "exps", "pretrained_iknet_SimGrasp", "ckpt", "model_0001.pt")
    assert os.path.exists(ckpt)
    assert set(torch.load(ckpt)["model"]) == {str(k) for k in G["state_keys"]}
    p.add_argument("--mode_name", default="test")
    t = p.parse_args(["--config", "handiknet_test_HO3D.yml", "--hand_model", "synthetic"])
    t.synthetic_frames = 3
    capsys.readouterr()
    test_entry.main(t)
    out = capsys.readouterr().out
    assert "Load IKNet model from" in out and ckpt in out and "[Hand Tracking] Use IKNet: True" in out and "Network Forwarding" in out


def test_iknet_learns_on_synthetic_frames():
    from datasets.synthetic import SyntheticIKFrames
    torch.manual_seed(0)
    hm = SyntheticLBSHand()
    cfg = {"device": torch.device("cuda"), "network": {"iknetframe": "kp"}, "hand_model": hm, "hand_jitter_cfg": {"rand_scale": 0.005}}
    batch = lambda ds, idx: torch.utils.data.default_collate([ds[i] for i in idx])
    train, held = SyntheticIKFrames(cfg, 1024, base_seed=0), SyntheticIKFrames(cfg, 256, base_seed=10 ** 6)
    tr = batch(train, range(1024))
    ho = batch(held, range(256))
    m = IKNet(cfg).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    flags = {"track_flag": False}

    def held_loss():
        m.eval()
        with torch.no_grad():
            return float(m.compute_loss(ho, m(ho, flags), flags)[0]["quat_loss"])
    first = held_loss()
    g = torch.Generator().manual_seed(0)
    for _ in range(300):
        m.train()
        idx = torch.randint(0, 1024, (64,), generator=g)
        b = {"gt_hand_kp": tr["gt_hand_kp"][idx], "jittered_hand_kp": tr["jittered_hand_kp"][idx],
             "gt_hand_pose": {k: v[idx] for k, v in tr["gt_hand_pose"].items()}}
        loss, _ = m.compute_loss(b, m(b, flags), flags)
        opt.zero_grad()
        loss["quat_loss"].backward()
        opt.step()
    last = held_loss()
    print(f"held-out quat_loss {first:.4f} -> {last:.4f} ({last / first:.3f})")
    assert last < 0.5 * first  # measured on the MI355X: 0.334 -> 0.105 (0.315)
