"""GPU: the device-resident route of the hand-pose particle optimiser (hotrack_amd/csrc/hand_pose.hip through
gf_optimize_hand_pose with opt.fused_pose) against a float64 evaluation of the hand model, against the imported reference's
recorded outputs (tests/golden/hand_opt_sequence.npz) and against the torch route on the same GPU; its branches, determinism,
graph capture, the shape space and the tracking loop.

Bounds.  Geometry: 3e-7 m against float64 (perturbing the fixture's candidate set by that much moves no energy by more than
1.5e-6; at 1e-6 m a silhouette pixel flips for up to 2 of 768 candidates; the fp32 torch route sits at 7.2e-8 m).  Energies:
1e-5 (the existing GPU test's tolerance for the torch route) for all but at most 2 candidates, and an excluded candidate
must differ by a whole discrete step.  Tracking: the existing GPU test's tolerances (2e-5 keypoints / translation, 1e-4
rotation, 4e-4 pose code)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

GEOM_TOL = 3e-7
E_TOL = 1e-5
KP_TOL, R_TOL, THETA_TOL = 2e-5, 1e-4, 4e-4
SIL_STEP = 0.1 / 778
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}


def _setup(fused, hand_model=None, device="cuda"):
    from models.hand_model import SyntheticLBSHand
    from models.optimization_hand import gf_optimize_hand_pose
    g = np.load(os.path.join(ROOT, "tests", "golden", "hand_opt_sequence.npz"))
    res, stride = int(g["meta"][0]), float(g["meta"][1])
    cfg = {"device": device, "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": fused}}
    opt = gf_optimize_hand_pose(cfg, hand_model=hand_model or SyntheticLBSHand(), particle_size=g["pre_sampled_particle"].shape[0])
    opt.pre_sampled_particle = torch.from_numpy(g["pre_sampled_particle"]).to(device)
    opt.load_volume(torch.from_numpy(g["volume"]).reshape(res, res, res), stride)
    proj = dict(zip(("fx", "fy", "cx", "cy", "w", "h"), g["proj"].tolist()))
    obj_pose = {"rotation": torch.from_numpy(g["R_obj"])[None].to(device), "translation": torch.from_numpy(g["t_obj"]).reshape(1, 3, 1).to(device)}
    mask = torch.from_numpy(g["background_mask"]).to(device)
    return g, opt, proj, obj_pose, mask


def _frame_inputs(g, f, device="cuda"):
    t = lambda k: torch.from_numpy(g[f"f{f}_{k}"]).to(device)
    last = g[f"f{f}_last_kp"]
    return (t("init_mano"), {"rotation": t("init_rot"), "translation": t("init_trans")}, t("init_kp"),
            None if last.size == 0 else torch.from_numpy(last).to(device), t("vis_mask"))


def _sample(opt, dtype=None):
    sp = opt.pre_sampled_particle * opt.initial_scale
    if dtype is not None:
        sp = opt.pre_sampled_particle.to(dtype) * opt.initial_scale.to(dtype)
    return torch.cat([torch.sqrt(1 - sp[:, 0] ** 2 - sp[:, 1] ** 2 - sp[:, 2] ** 2).unsqueeze(1), sp], 1)


def _kernel_eval(opt):
    from hotrack_amd import ext
    state = opt._pack_state(opt.initial_scale)
    return ext.hand_pose_energy(state=state, with_geometry=True, **opt._kernel_frame())


def _float64_geometry(g, hand_model, beta=None):
    """get_kp_from_delta in double on the CPU at frame 0's state."""
    _, o, proj, obj_pose, mask = _setup(False, hand_model=hand_model.double(), device="cpu")
    mano, pose, kp0, last, vis = _frame_inputs(g, 0, "cpu")
    o.set_init_para(mano.double(), {k: v.double() for k, v in pose.items()}, kp0.double(), last, vis, obj_pose, None, proj, mask)
    if beta is not None:
        o.mano_layer_right.register_beta(beta.double())
    with torch.no_grad():
        return o.get_kp_from_delta(_sample(o, torch.float64))


def _voxel_step(g):
    v = g["volume"].astype(np.float32).reshape(int(g["meta"][0]), -1)
    d = np.abs(np.diff(v, axis=-1))
    return float(d[d > 0].min())


def _assert_energies(got, want, g, what):
    """1e-5 for all but at most 2 candidates; an excluded candidate differs by a whole discrete step: a multiple of one
    silhouette pixel (0.1 / 778), or at least a voxel's worth of penetration / attraction (weight 0.05)."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bad = np.nonzero(~(diff <= E_TOL))[0]
    print(f"{what}: max |dE| = {diff.max():.3e}, candidates beyond {E_TOL:g}: {len(bad)} {diff[bad].tolist()}")
    assert len(bad) <= 2, f"{what}: {len(bad)} candidates differ by more than {E_TOL:g}"
    vox = _voxel_step(g)
    for q in bad:
        k = round(diff[q] / SIL_STEP)
        whole = (k >= 1 and abs(diff[q] - k * SIL_STEP) <= E_TOL) or diff[q] >= 0.05 * vox - 1e-9
        assert whole, f"{what}: candidate {q} differs by {diff[q]:.3e}, not a whole discrete step"


def _start_frame0(fused, hand_model=None, beta=None):
    g, opt, proj, obj_pose, mask = _setup(fused, hand_model=hand_model)
    mano, pose, kp0, last, vis = _frame_inputs(g, 0)
    opt.set_init_para(mano, pose, kp0, last, vis, obj_pose, beta, proj, mask)
    return g, opt


def test_candidate_geometry_matches_float64():
    from models.hand_model import SyntheticLBSHand
    g, opt = _start_frame0(True)
    assert opt.use_kernel()
    with torch.no_grad():
        _, verts, kp = _kernel_eval(opt)
        v64, k64 = _float64_geometry(g, SyntheticLBSHand())
        tv, tk = opt.get_kp_from_delta(_sample(opt))
    dv, dk = float((verts.cpu().double() - v64).abs().max()), float((kp.cpu().double() - k64).abs().max())
    print(f"kernel vs float64: vertices {dv:.3e} m, keypoints {dk:.3e} m; torch route vs float64: vertices "
          f"{float((tv.cpu().double() - v64).abs().max()):.3e} m, keypoints {float((tk.cpu().double() - k64).abs().max()):.3e} m")
    assert verts.shape == (768, 778, 3) and kp.shape == (768, 21, 3)
    assert dv <= GEOM_TOL and dk <= GEOM_TOL


def test_candidate_energies_match_the_reference_and_the_torch_route():
    g, opt = _start_frame0(True)
    with torch.no_grad():
        energy, _, _ = _kernel_eval(opt)
        torch_e = opt.evaluate(*opt.get_kp_from_delta(_sample(opt))).float()
    assert (g["e0_penetration"] > 0).all()
    _assert_energies(energy.cpu().numpy(), g["e0_energy"], g, "kernel vs reference")
    _assert_energies(energy.cpu().numpy(), torch_e.cpu().numpy(), g, "kernel vs torch route")


def _track(fused):
    g, opt, proj, obj_pose, mask = _setup(fused)
    out, prev = [], None
    with torch.no_grad():
        for f in range(4):
            mano, pose, kp0, _, vis = _frame_inputs(g, f)
            kp, theta, R, t = opt.optimize(mano, pose, kp0, prev, vis, obj_pose, None, proj, mask)
            out.append((kp.cpu().numpy(), theta.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()))
            prev = kp  # our result feeds the next frame
    return g, out


def test_tracking_parity_with_the_reference():
    g, fused = _track(True)
    _, eager = _track(False)
    names = ("final_kp", "theta", "R", "t")
    dist = lambda run: [max(float(np.abs(run[f][i] - g[f"f{f}_{n}"]).max()) for f in range(4)) for i, n in enumerate(names)]
    df, dt = dist(fused), dist(eager)
    print("distance to the reference (keypoints, pose code, rotation, translation): fused %s, torch route %s"
          % (["%.3e" % v for v in df], ["%.3e" % v for v in dt]))
    for f in range(4):
        kp, theta, R, t = fused[f]
        np.testing.assert_allclose(kp, g[f"f{f}_final_kp"], rtol=0, atol=KP_TOL, err_msg=f"frame {f} keypoints")
        np.testing.assert_allclose(theta, g[f"f{f}_theta"], rtol=0, atol=THETA_TOL, err_msg=f"frame {f} pose code")
        np.testing.assert_allclose(R, g[f"f{f}_R"], rtol=0, atol=R_TOL, err_msg=f"frame {f} rotation")
        np.testing.assert_allclose(t, g[f"f{f}_t"], rtol=0, atol=KP_TOL, err_msg=f"frame {f} translation")


def _one_frame(fused, f=0, pre_zero=False, obj_shift=None):
    g, opt, proj, obj_pose, mask = _setup(fused)
    opt.keep_trace = True
    if pre_zero:
        opt.pre_sampled_particle = torch.zeros_like(opt.pre_sampled_particle)
    if obj_shift is not None:
        obj_pose = dict(obj_pose, translation=obj_pose["translation"] + obj_shift)
    mano, pose, kp0, last, vis = _frame_inputs(g, f)
    with torch.no_grad():
        out = opt.optimize(mano, pose, kp0, last, vis, obj_pose, None, proj, mask)
    return opt, (mano, pose), out


def _assert_same_result(a, b):
    for x, y, tol in zip(a, b, (KP_TOL, THETA_TOL, R_TOL, KP_TOL)):
        assert float((x - y).abs().max()) <= tol


def test_no_better_candidate_leaves_the_state_alone():
    """All pre-sampled rows zero: every candidate is the current estimate, none is better."""
    fo, (mano, pose), f_out = _one_frame(True, pre_zero=True)
    to, _, t_out = _one_frame(False, pre_zero=True)
    assert fo.use_kernel() and not to.use_kernel()
    assert not fo.trace[:, 2].any() and not to.trace[:, 2].any()
    assert all(torch.isfinite(x).all() for x in f_out) and torch.isfinite(fo.trace).all()
    assert torch.equal(fo.curr_theta, mano) and torch.equal(fo.curr_r, pose["rotation"])
    assert torch.equal(fo.curr_t.reshape(-1), pose["translation"].reshape(-1))
    assert torch.equal(fo.prev_search_size, fo.initial_scale) and bool(fo.prev_success) is False
    assert torch.allclose(fo.search_size, to.search_size, rtol=1e-5, atol=0)
    assert torch.allclose(fo.trace, to.trace, rtol=1e-5, atol=1e-6)
    _assert_same_result(f_out, t_out)


def test_first_frame_without_a_previous_frame():
    fo, _, f_out = _one_frame(True, f=0)
    to, _, t_out = _one_frame(False, f=0)
    assert fo.last_frame_kp is None and fo.trace[:, 2].any()
    _assert_same_result(f_out, t_out)


def test_attraction_is_gated_off_when_candidate_zero_does_not_penetrate():
    shift = torch.tensor([0.0, 0.0, 1.0], device="cuda").reshape(1, 3, 1)  # the object a metre behind the hand
    g, opt, proj, obj_pose, mask = _setup(True)
    obj_pose = dict(obj_pose, translation=obj_pose["translation"] + shift)
    mano, pose, kp0, last, vis = _frame_inputs(g, 1)
    with torch.no_grad():
        opt.set_init_para(mano, pose, kp0, last, ~vis, obj_pose, None, proj, mask)  # fingertips invisible: attraction is formed
        hand, kp = opt.get_kp_from_delta(_sample(opt))
        sdf, pen = opt.query_sdf_and_penetration(hand)
        assert float(pen[0]) == 0 and float(opt.get_attraction_loss(sdf).float().abs().max()) > 0
        torch_e = opt.evaluate(hand, kp).float()
        energy, _, _ = _kernel_eval(opt)
    _assert_energies(energy.cpu().numpy(), torch_e.cpu().numpy(), g, "gated attraction, kernel vs torch route")
    fo, _, f_out = _one_frame(True, f=1, obj_shift=shift)
    to, _, t_out = _one_frame(False, f=1, obj_shift=shift)
    _assert_same_result(f_out, t_out)


def test_two_runs_are_bitwise_equal():
    from hotrack_amd import ext
    g, opt = _start_frame0(True)
    runs = []
    for _ in range(2):
        state = opt._pack_state(opt.initial_scale)
        tr = ext.hand_pose_opt(state=state, iterations=5, scaling_coefficient2=opt.scaling_coefficient2, beta=opt.beta, trace=True,
                               **opt._kernel_frame())
        runs.append((state, tr))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1][:, 2].any() and torch.isfinite(runs[0][1]).all() and torch.isfinite(runs[0][0]).all()


def test_optimize_captures_into_a_graph_and_never_syncs():
    g, opt, proj, obj_pose, mask = _setup(True)
    mano, pose, kp0, _, vis = _frame_inputs(g, 1)
    last = torch.from_numpy(g["f0_final_kp"]).cuda()
    args = (mano, pose, kp0, last, vis, obj_pose, None, proj, mask)
    with torch.no_grad():
        eager = [x.clone() for x in opt.optimize(*args)]  # (also the warm-up: tables, LDS attribute)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = opt.optimize(*args)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = opt.optimize(*args)
        graph.replay()
        torch.cuda.synchronize()
    for a, b, c in zip(eager, again, out):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_shape_space_matches_float64_and_the_torch_route():
    from models.hand_model import SyntheticLBSHand
    beta = torch.tensor([[1.5, -1.0, 0.8, 1.2, -1.3, 0.4, -0.7, 1.1, -0.9, 0.6]])
    g, opt = _start_frame0(True, hand_model=SyntheticLBSHand(num_betas=10), beta=beta.cuda())
    assert opt.use_kernel()
    with torch.no_grad():
        energy, verts, kp = _kernel_eval(opt)
        v64, k64 = _float64_geometry(g, SyntheticLBSHand(num_betas=10), beta=beta)
        torch_e = opt.evaluate(*opt.get_kp_from_delta(_sample(opt))).float()
        v0, _ = _float64_geometry(g, SyntheticLBSHand(num_betas=10))
    dv, dk = float((verts.cpu().double() - v64).abs().max()), float((kp.cpu().double() - k64).abs().max())
    print(f"shaped hand, kernel vs float64: vertices {dv:.3e} m, keypoints {dk:.3e} m")
    assert float((v64 - v0).abs().max()) > 1e-3   # the shape code moves the hand
    assert dv <= GEOM_TOL and dk <= GEOM_TOL
    _assert_energies(energy.cpu().numpy(), torch_e.cpu().numpy(), g, "shaped hand, kernel vs torch route")


def test_tracking_loop_with_the_switch_on_and_off(capsys):
    """HandTrackModel with an oracle handnet on the synthetic sequence, 512 particles, switch on and off.  (On this sequence the
    stand-in for IKNet starts every frame from a rigid least-squares fit, which no candidate of either route improves on, so the
    two routes agree exactly; the routes' updates are compared in the tests above.)"""
    from datasets.synthetic import SyntheticHandObjectSequences
    from models.hand_model import SyntheticLBSHand
    from models.track_network import HandTrackModel

    class OracleNet(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.device = cfg["device"]

        def forward(self, data, flags):
            kp = data["gt_hand_kp"].to(self.device) + 0.002 * torch.randn(1, 21, 3, device=self.device, generator=self.g)
            return {"pred_kp": kp, "pred_kp_vis_mask": torch.ones(1, 21, dtype=torch.bool, device=self.device)}

    def run(fused):
        hm = SyntheticLBSHand()
        cfg = {"device": torch.device("cuda"), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
               "use_optimization": True, "hand_particles": 512, "hand_model": hm,
               "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": fused}}
        seq = SyntheticHandObjectSequences(cfg, 1, 4)[0]
        model = HandTrackModel(cfg, handnet=OracleNet, hand_model=hm).eval()
        assert model.optimizer.use_kernel() == fused
        model.handnet.g = torch.Generator(device="cuda").manual_seed(0)
        model.use_graph = False
        with torch.no_grad():
            return [r["pred_kp"].cpu() for r in model(seq, {"track_flag": True, "test_flag": True, "save_flag": False})]

    on = run(True)
    assert "device-resident route" in capsys.readouterr().out
    off = run(False)
    assert "device-resident route" not in capsys.readouterr().out
    d = [float((a - b).abs().max()) for a, b in zip(on, off)]
    print("per-frame |pred_kp(on) - pred_kp(off)|:", ["%.3e" % v for v in d])
    assert all(torch.isfinite(a).all() for a in on) and max(d) <= KP_TOL
