"""GPU: the hand shape-code search kernel (hotrack_amd/csrc/hand_shape.hip through gf_optimize_hand_shape's GPU route)
against the reference's recorded calls (tests/golden/hand_shape_opt.npz) and against the torch route, its determinism and
graph capture, and shape estimation in the tracking loop (HandTrackModel, use_pred_hand_shape 1 / 2 / 3)."""
import argparse
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

from models.hand_model import SyntheticLBSHand  # noqa: E402
from models.optimization_hand import gf_optimize_hand_shape, kp2length  # noqa: E402

ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}


def _lengths(hm, beta):
    with torch.no_grad():
        _, kp = hm(th_pose_coeffs=torch.zeros(beta.shape[0], 48, dtype=torch.float64),
                   th_betas=torch.as_tensor(beta, dtype=torch.float64).cpu())
    return kp2length(kp)


def _opt(P, pre=None, hm=None):
    opt = gf_optimize_hand_shape({"device": "cuda"}, hand_model=hm or SyntheticLBSHand(num_betas=10), particle_size=P)
    if pre is not None:
        opt.pre_sampled_particle = torch.as_tensor(pre).cuda()
    opt.keep_trace = True
    return opt


CALLS = [("m1_768", 768, None), ("m3_768", 768, 3), ("fail_768", 768, None), ("m1_5120", 5120, None)]


@pytest.mark.parametrize("name,P,history", CALLS, ids=[c[0] for c in CALLS])
def test_kernel_matches_the_reference(name, P, history):
    g = np.load(os.path.join(G, "hand_shape_opt.npz"))
    opt = _opt(P, g[f"pre_{P}"])
    assert opt.use_kernel()
    keys = [f"{name}_{i}" for i in range(history)] if history else [name]
    for i, key in enumerate(keys):
        with torch.no_grad():
            shape = opt.optimize(torch.from_numpy(g[f"{key}_pred_kp"]).cuda(), use_old=history is not None)
        assert opt.old_pred_length.shape == (1, i + 1, 15) and opt.old_pred_length.is_cuda
        got, ref = shape.cpu().double().reshape(1, 10), torch.from_numpy(g[f"{key}_shape"]).double()[None]
        np.testing.assert_allclose(got.numpy()[0], ref.numpy()[0], rtol=0, atol=1e-4)
        hm = opt.mano_layer_right.cpu()
        assert float((_lengths(hm, got) - _lengths(hm, ref)).abs().max()) < 1e-6
        opt.mano_layer_right.cuda()
        # search sizes: continuous in the energies, which the kernel forms from the affine basis instead of a forward pass
        np.testing.assert_allclose(opt.trace[:-1, 3:].cpu().numpy(), g[f"{key}_search"][1:], rtol=1e-3, atol=1e-5)
        if name == "fail_768":
            assert torch.equal(shape.cpu(), torch.zeros(1, 10)) and not opt.trace[:, 2].any()


@pytest.mark.parametrize("T", [1, 10])
def test_kernel_matches_the_torch_route(T):
    hm = SyntheticLBSHand(num_betas=10)
    rng = np.random.default_rng(T)
    beta = torch.from_numpy(rng.normal(0, 1.0, (1, 10)).astype(np.float32))
    with torch.no_grad():
        _, kp = hm(th_pose_coeffs=torch.zeros(T, 48), th_betas=beta.expand(T, -1))
    kps = (kp + torch.from_numpy(rng.normal(0, 0.001, kp.shape).astype(np.float32))).cuda()
    res = {}
    for route in ("kernel", "torch"):
        opt = _opt(5120, hm=copy.deepcopy(hm))
        if route == "torch":
            opt.use_kernel = lambda: False
        for t in range(T):
            with torch.no_grad():
                shape = opt.optimize(kps[t:t + 1], use_old=True)
        assert opt.old_pred_length.shape == (1, T, 15)
        res[route] = (shape.cpu().double(), opt.trace.cpu())
    np.testing.assert_allclose(res["kernel"][0].numpy(), res["torch"][0].numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(res["kernel"][1][:, 3:].numpy(), res["torch"][1][:, 3:].numpy(), rtol=1e-3, atol=1e-5)
    e_k = (_lengths(hm, res["kernel"][0]) - _lengths(hm, beta.double())).abs().mean()
    e_0 = (_lengths(hm, torch.zeros(1, 10)) - _lengths(hm, beta.double())).abs().mean()
    assert e_k < 0.5 * e_0


def _kernel_inputs():
    from hotrack_amd import ext  # noqa: F401
    opt = _opt(5120)
    k0, k = opt.keypoint_basis()
    g = torch.Generator().manual_seed(0)
    beta = torch.randn(1, 10, generator=g).expand(3, -1) + 0.05 * torch.randn(3, 10, generator=g)  # three noisy views of one hand
    targets = (kp2length(opt.mano_layer_right(th_pose_coeffs=torch.zeros(3, 48, device="cuda"), th_betas=beta.cuda())[1])).contiguous()
    return opt, k0, k, targets


def test_kernel_is_bitwise_deterministic():
    from hotrack_amd import ext
    opt, k0, k, targets = _kernel_inputs()
    runs = [ext.hand_shape_opt(k0, k, opt.pre_sampled_particle, targets, opt.initial_scale, 2000, 0.9, 20, trace=True)
            for _ in range(3)]
    for h, tr in runs[1:]:
        assert torch.equal(h, runs[0][0]) and torch.equal(tr, runs[0][1])
    assert runs[0][1][:, 2].any() and torch.isfinite(runs[0][1]).all()


def test_kernel_call_is_graph_capturable():
    """One launch, no host synchronisation: the call captures into a graph, and replays follow new targets."""
    from hotrack_amd import ext
    from hotrack_amd import pointnet2_hip
    opt, k0, k, targets = _kernel_inputs()
    static_t = targets.clone()
    args = (k0, k, opt.pre_sampled_particle, static_t, opt.initial_scale, 2000, 0.9, 20)
    pointnet2_hip.PROFILE = []
    try:
        ext.hand_shape_opt(*args)  # warm-up (the LDS attribute is raised on first use)
        assert [p[0] for p in pointnet2_hip.PROFILE] == ["hand_shape_kernel"]
    finally:
        pointnet2_hip.PROFILE = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, _ = ext.hand_shape_opt(*args)
    for t in (targets, targets.flip(0) * 1.01):
        static_t.copy_(t)
        graph.replay()
        want, _ = ext.hand_shape_opt(k0, k, opt.pre_sampled_particle, t.contiguous(), opt.initial_scale, 2000, 0.9, 20)
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def _shaped_sequence(frames, beta_true):
    from datasets.synthetic import SyntheticHandObjectSequences
    hm = SyntheticLBSHand(num_betas=10)
    cfg = {"device": torch.device("cuda"), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
           "use_optimization": True, "hand_particles": 256, "hand_model": hm, "opt": {"energy_weight": dict(ENERGY_WEIGHT)}}
    return cfg, hm, SyntheticHandObjectSequences(cfg, 1, frames, hand_beta=beta_true)[0]


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_tracking_loop_estimates_the_hand_shape(mode):
    """HandTrackNet replaced by an oracle returning jittered ground-truth keypoints of a hand with shape beta*: the estimated
    shape's bone lengths are closer to beta*'s than the zero shape's, and the palm template and pred_beta change exactly
    on the frames the mode names (frame 0; frames 0 and 10)."""
    from models.track_network import HandTrackModel
    beta_true = np.array([1.5, -1.0, 0.8, 1.2, -1.3, 0.4, -0.7, 1.1, -0.9, 0.6])
    cfg, hm, seq = _shaped_sequence(12, beta_true)
    cfg["use_pred_hand_shape"] = mode
    assert torch.allclose(seq[0]["gt_hand_pose"]["mano_beta"].double(), torch.from_numpy(beta_true)[None].double())

    class OracleNet(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.device = cfg["device"]

        def forward(self, data, flags):
            kp = data["gt_hand_kp"].to(self.device) + 0.002 * torch.randn(1, 21, 3, device=self.device, generator=self.g)
            return {"pred_kp": kp, "pred_kp_vis_mask": torch.ones(1, 21, dtype=torch.bool, device=self.device)}

    model = HandTrackModel(cfg, handnet=OracleNet, hand_model=hm).eval()
    assert model.opt_shape is not None and model.opt_shape.use_kernel()
    model.handnet.g = torch.Generator(device="cuda").manual_seed(0)
    model.use_graph = False
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    with torch.no_grad():
        rets = model(seq, flags)
    due = [i for i in range(12) if (mode == 1 and i == 0) or (mode > 1 and i % 10 == 0)]
    for i in range(1, 12):
        changed_palm = not torch.equal(seq[i]["pred_palm_template"], seq[i - 1]["pred_palm_template"])
        changed_beta = not torch.equal(rets[i]["pred_beta"], rets[i - 1]["pred_beta"])
        assert changed_palm == (i - 1 in due), (i, changed_palm)   # the template estimated on frame i-1 is used from frame i
        assert changed_beta == (i in due), (i, changed_beta)
    assert seq[0]["pred_beta"] is rets[0]["pred_beta"]
    est = rets[-1]["pred_beta"].cpu().double()
    ref = _lengths(hm.cpu(), torch.from_numpy(beta_true)[None])
    e_est = float((_lengths(hm, est) - ref).abs().mean())
    e_zero = float((_lengths(hm, torch.zeros(1, 10)) - ref).abs().mean())
    assert e_est < 0.5 * e_zero, (e_est, e_zero)
    if mode == 3:
        assert model.opt_shape.old_pred_length.shape == (1, 2, 15)


def test_graph_step_follows_a_changed_palm_template():
    """Modes 2 and 3 change the palm template mid-sequence: it goes through the captured graph's static input buffer, so a
    replay with a new template equals the eager network on that template."""
    from _netinit import deterministic_init, make_cfg
    from hotrack_amd import fused, pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    from models.track_network import HandTrackModel
    pointnet_utils.set_operator_backend(pointnet2_utils)
    cfg, hm, seq = _shaped_sequence(2, np.linspace(-1, 1, 10))
    cfg.update(make_cfg(torch.device("cuda", 0)))
    cfg.update(num_points=512, use_pred_hand_shape=2)
    model = HandTrackModel(cfg, handnet=HandTrackNet, hand_model=hm)
    deterministic_init(model.handnet)
    model = model.cuda().eval()
    flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": True}
    pts = seq[0]["hand_points"].cuda().float()
    kp = seq[0]["jittered_hand_kp"].cuda().float()
    palms = [model._shaped_palm_template(torch.zeros(1, 10, device="cuda")),
             model._shaped_palm_template(torch.linspace(-2, 2, 10, device="cuda")[None])]
    assert not torch.equal(palms[0], palms[1])
    try:
        pointnet_utils.set_fused_backend(fused)
        with torch.no_grad():
            for palm in palms + palms[:1]:
                got = model._graph_step(pts, kp, palm, flags)
                want = model.handnet({"hand_points": pts, "jittered_hand_kp": kp, "pred_palm_template": palm}, flags)
                assert len(model._graphs) == 1
                assert torch.allclose(got["pred_kp"], want["pred_kp"], atol=1e-5)
    finally:
        pointnet_utils.set_fused_backend(None)


def test_handopt_entry_point_with_a_shaped_hand_model(tmp_path, monkeypatch, capsys):
    """handopt_test_HO3D.yml (use_pred_hand_shape: 1) with --hand_model synthetic_shaped runs shape estimation on the GPU
    through the unchanged test.py entry point."""
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    import test as test_entry
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    a = p.parse_args(["--config", "handopt_test_HO3D.yml", "--hand_model", "synthetic_shaped", "--hand_particles", "512"])
    a.synthetic_frames = 3
    test_entry.main(a)
    out = capsys.readouterr().out
    assert "hand shape estimation: use_pred_hand_shape = 1 (GPU kernel)" in out and "Network Forwarding" in out
    line = [l for l in out.splitlines() if l.startswith("Test hand_pred_kp_diff")][0]
    assert np.isfinite(float(line.split()[-1]))
