"""GPU: the MANO entry points of the device-resident hand-pose optimiser (pn2x_hand_pose_mano_energy / _opt, hotrack_amd/csrc/
hand_pose.hip: pose-offset pre-pass on the matrix cores, MANO instantiation of the evaluation) with SyntheticManoHand.

Small cases hit the edges: V = 97 (a partial 64-lane stripe, a partial unroll group), a fingertip vertex at index V - 1,
K in {1, 4}, P = 67 (no multiple of the four waves, a partial 64-candidate group of the pre-pass), a 17^3 volume in fp16 and
fp32, a 24 x 32 mask; one case has the workload's hand (V = 778) and P = 768.

Bounds.  Geometry against the model's forward() in float64: GEOM_TOL = max(3e-7 m, 4 x the fp32 torch forward()'s own distance
to float64) -- measured on the CPU at these cases' candidates: 6.8e-8 m (V = 97) and 7.4e-8 m (V = 778), so 3e-7 m binds.
Energies against evaluate()'s terms on the float64 geometry: 1e-5; a candidate beyond it must have a float64 vertex within
1e-6 m of a voxel face or 1e-4 px of a pixel edge (the nearest-voxel and pixel reads are discontinuous), and at most 2 % of the
candidates may be left out this way.  Tracking: the plain route's tolerances (keypoints and translation 2e-5, pose code 4e-4,
rotation 1e-4)."""
import copy
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_pose_cases as C  # noqa: E402

from models.hand_model import SyntheticManoHand, rodrigues  # noqa: E402
from models.optimization_hand import gf_optimize_hand_pose  # noqa: E402

pytestmark = pytest.mark.gpu

# fp32 torch forward() vs float64, measured on the CPU over these cases' candidates: 7.4e-8 m at most
TORCH_FP32_VS_F64 = 7.4e-8
GEOM_TOL = max(3e-7, 4 * TORCH_FP32_VS_F64)
E_TOL = 1e-5
LEFT_OUT_SHARE = 0.02
VOXEL_EDGE_M, PIXEL_EDGE_PX = 1e-6, 1e-4
KP_TOL, R_TOL, THETA_TOL = 2e-5, 1e-4, 4e-4

#         name            V    K  tips at            P    dtype           h   w   focal  seed
CASES = {"small-k4-fp16": (97, 4, (5, 20, 40, 60, 96), 67, torch.float16, 24, 32, 40.0, 3),
         "small-k1-fp32": (97, 1, (5, 20, 40, 60, 96), 67, torch.float32, 24, 32, 40.0, 4),
         "small-k4-fp32": (97, 4, None, 67, torch.float32, 24, 32, 40.0, 5),
         "workload-hand": (778, 4, None, 768, torch.float16, 96, 128, 150.0, 6)}
_BUILT = {}


def _case(name):
    """The case's model, CPU inputs (SimpleNamespace, as tests/_hand_pose_cases.py builds them) and its float64 reference,
    built once and left unchanged."""
    if name in _BUILT:
        return _BUILT[name]
    V, K, tips, P, dt, h, w, focal, seed = CASES[name]
    model = SyntheticManoHand(num_verts=V, weights_per_vertex=K, tip_vertices=tips)
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(name=name, P=P, V=V, K=K, res=17, h=h, w=w, theta_scale=C.THETA_SCALE, weights=dict(C.ENERGY_WEIGHT),
                        tables=model.skinning_tables(), pre=C._pre_rows(P, seed))
    assert c.tables is not None and c.tables["skin_idx"].shape == (V, K)
    R0 = rodrigues(torch.tensor((0.25, -0.3, 0.35), dtype=torch.float64)).float()
    c.state = C.pack_state(R0, torch.tensor((-0.02, -0.09, 0.5)), 0.15 * torch.randn(45, generator=g), torch.full((16,), 0.005))
    c.beta = 0.8 * torch.randn(1, 10, generator=g)
    v64, k64 = _float64_geometry(model, c)
    v0, k0 = v64[0], k64[0]
    c.pred_kp = (k0.float() + torch.tensor([0.006, -0.004, 0.005]) + 0.002 * torch.randn(21, 3, generator=g)).contiguous()
    c.last_kp = (k0.float() + 0.003 * torch.randn(21, 3, generator=g)).contiguous()
    c.vis = torch.ones(21, dtype=torch.bool)
    c.vis[[3, 8, 10, 20]] = False
    # a sphere of 4 cm that candidate 0's palm penetrates by about a centimetre (tests/_hand_pose_cases.py: make_case)
    rad, c_obj = 0.04, torch.tensor([0.016, -0.012, 0.008], dtype=torch.float64)
    anchor = v0[(v0 - v0.mean(dim=0)).norm(dim=1).argmin()]
    centre = anchor + R0.double() @ torch.tensor([0.0, 0.0, rad - 0.012], dtype=torch.float64)
    Ro = rodrigues(torch.tensor([0.3, -0.5, 0.4], dtype=torch.float64))
    c.obj_r, c.obj_t = Ro.float().contiguous(), (centre - Ro @ c_obj).float().contiguous()
    c.voxel_scale = round(0.25 / c.res, 4)
    ax = (torch.arange(c.res, dtype=torch.float64) - c.res // 2 + 0.5) * c.voxel_scale
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c.volume = (torch.sqrt((X - c_obj[0]) ** 2 + (Y - c_obj[1]) ** 2 + (Z - c_obj[2]) ** 2) - rad).to(dt).contiguous()
    mid = v0.mean(dim=0)
    cx, cy = round(w / 2.0 - float(mid[0] / mid[2]) * focal, 2), round(h / 2.0 - float(mid[1] / mid[2]) * focal, 2)
    c.proj = {"fx": focal, "fy": focal, "cx": cx, "cy": cy, "w": w, "h": h}
    px, py = v0[:, 0] / v0[:, 2] * focal + cx, v0[:, 1] / v0[:, 2] * focal + cy
    a, b = 1.2 * float(px.std()), 1.2 * float(py.std())
    rows, cols = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    mx, my = float(px.median()), float(py.median())
    c.mask = (((cols - mx) / a) ** 2 + ((rows - my) / b) ** 2 > 1) | ((cols - mx - 0.3 * (rows - my)).abs() < 0.15 * a)
    terms = C.reference_terms(c, v64, k64)
    assert terms["gate"] and 0.2 < float(c.mask.float().mean()) < 0.98
    _BUILT[name] = (model, c, v64, k64, terms)
    return _BUILT[name]


def _float64_geometry(model, c):
    """The model's forward() in float64 at every candidate's pose, composed as get_kp_from_delta composes it."""
    opt = gf_optimize_hand_pose({"device": "cpu"}, hand_model=copy.deepcopy(model).double(), particle_size=c.P)
    st = c.state.double()
    opt.curr_r, opt.curr_t, opt.curr_theta = st[C.S_R:C.S_R + 9].view(1, 3, 3), st[C.S_T:C.S_T + 3].view(1, 3, 1), st[C.S_THETA:C.S_THETA + 45].view(1, 45)
    opt.mano_layer_right.register_beta(c.beta.double())
    with torch.no_grad():
        return opt.get_kp_from_delta(C.candidate_samples(c.state, c.pre))


def _optimiser(model, c, fused=True, device="cuda"):
    cfg = {"device": device, "opt": {"energy_weight": dict(C.ENERGY_WEIGHT), "fused_pose": fused}}
    opt = gf_optimize_hand_pose(cfg, hand_model=copy.deepcopy(model), particle_size=c.P)
    opt.pre_sampled_particle = c.pre.to(device)
    opt.load_volume(c.volume, c.voxel_scale)
    return opt


def _frame_args(c, device="cuda", last=True):
    st = c.state.to(device)
    return (st[C.S_THETA:C.S_THETA + 45].view(1, 45).clone(),
            {"rotation": st[C.S_R:C.S_R + 9].view(1, 3, 3).clone(), "translation": st[C.S_T:C.S_T + 3].view(1, 3).clone()},
            c.pred_kp[None].to(device), c.last_kp[None].to(device) if last else None, c.vis[None].to(device),
            {"rotation": c.obj_r[None].to(device), "translation": c.obj_t.reshape(1, 3, 1).to(device)}, c.beta.to(device), c.proj,
            c.mask.to(device))


def _started(name):
    model, c, *_ = _case(name)
    opt = _optimiser(model, c)
    opt.set_init_para(*_frame_args(c))
    assert opt.use_kernel()
    return opt


def _kernel_eval(opt, **kw):
    from hotrack_amd import ext
    out = ext.hand_pose_energy(state=opt._pack_state(opt.initial_scale), with_geometry=True, **opt._kernel_frame(), **kw)
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


def test_the_mano_route_exists_and_is_taken():
    from hotrack_amd import ext
    assert callable(ext.hand_pose_opt) and callable(ext.hand_pose_energy)
    from models.hand_model import named_hand_model
    cfg = {"device": "cuda", "opt": {"fused_pose": True}}
    opt = gf_optimize_hand_pose(cfg, hand_model=named_hand_model("synthetic_mano"), particle_size=64)
    assert opt.use_kernel() and opt._kernel_model()["mano"]
    assert not gf_optimize_hand_pose({"device": "cuda"}, hand_model=named_hand_model("synthetic_mano"), particle_size=64).use_kernel()


def _near_an_edge(c, verts):
    """Per candidate: a float64 vertex within VOXEL_EDGE_M of a voxel face or PIXEL_EDGE_PX of a pixel edge."""
    u = ((verts - c.obj_t.double().reshape(1, 1, 3)) @ c.obj_r.double()) / c.voxel_scale
    voxel = ((u - torch.round(u)).abs() * c.voxel_scale < VOXEL_EDGE_M).any(dim=-1)
    p = c.proj
    x, y = verts[..., 0] / verts[..., 2] * p["fx"] + p["cx"], verts[..., 1] / verts[..., 2] * p["fy"] + p["cy"]
    pixel = ((x - torch.round(x)).abs() < PIXEL_EDGE_PX) | ((y - torch.round(y)).abs() < PIXEL_EDGE_PX)
    return (voxel | pixel).any(dim=-1)


@pytest.mark.parametrize("name", list(CASES))
def test_geometry_and_energies_match_float64(name):
    model, c, v64, k64, terms = _case(name)
    energy, verts, kp = _kernel_eval(_started(name))
    assert verts.shape == (c.P, c.V, 3) and kp.shape == (c.P, 21, 3) and energy.shape == (c.P,)
    assert all(bool(torch.isfinite(x).all()) for x in (energy, verts, kp))
    dv, dk = float((verts.double() - v64).abs().max()), float((kp.double() - k64).abs().max())
    print(f"{name}: kernel vs float64 forward(): vertices {dv:.3e} m, keypoints {dk:.3e} m (bound {GEOM_TOL:.2e})")
    assert dv <= GEOM_TOL and dk <= GEOM_TOL
    diff = (energy.double() - terms["energy"].double()).abs()
    out = torch.nonzero(~(diff <= E_TOL)).flatten()
    near = _near_an_edge(c, v64)
    print(f"{name}: max |dE| = {float(diff.max()):.3e}; beyond {E_TOL:g}: {len(out)} of {c.P} {diff[out][:8].tolist()}; candidates with "
          f"a vertex near an edge: {int(near.sum())}")
    assert all(bool(near[q]) for q in out), f"{name}: a candidate away from every edge differs by more than {E_TOL:g}"
    assert len(out) <= LEFT_OUT_SHARE * c.P, f"{name}: {len(out)} of {c.P} candidates left out"


def test_the_pose_blend_shapes_are_used():
    """posedirs scaled by 0 in the kernel's arguments only: the geometry misses its bound by more than 100 x."""
    model, c, v64, k64, _ = _case("small-k4-fp16")
    opt = _started("small-k4-fp16")
    zero = torch.zeros_like(opt._kernel_model()["posedirs_pack"])
    _, verts, kp = _kernel_eval(opt, posedirs=zero)
    dv = float((verts.double() - v64).abs().max())
    print(f"without the pose blend shapes the vertices are off by {dv:.3e} m")
    assert dv > 100 * GEOM_TOL


def _track(name, fused, frames=4):
    """`frames` frames of a hand sliding past the object: each frame's target keypoints are the float64 hand moved on, each
    result feeds the next frame's start and previous keypoints."""
    model, c, v64, k64, _ = _case(name)
    opt = _optimiser(model, c, fused=fused)
    theta, pose, _, _, vis, obj, beta, proj, mask = _frame_args(c)
    g = torch.Generator().manual_seed(99)
    out, last = [], None
    with torch.no_grad():
        for f in range(frames):
            target = (k64[0].float() + (f + 1) * torch.tensor([0.004, -0.003, 0.003]) + 0.001 * torch.randn(21, 3, generator=g))[None].cuda()
            kp, theta, R, t = opt.optimize(theta, pose, target, last, vis, obj, beta, proj, mask)
            assert opt.use_kernel() == fused
            pose, last = {"rotation": R[None].clone(), "translation": t.clone()}, kp.clone()
            theta = theta.clone()
            out.append([x.cpu() for x in (kp, theta, R, t)])
    return out


def test_tracking_matches_the_torch_route():
    fused, eager = _track("small-k4-fp16", True), _track("small-k4-fp16", False)
    for f, (a, b) in enumerate(zip(fused, eager)):
        d = [float((x - y).abs().max()) for x, y in zip(a, b)]
        print(f"frame {f}: |fused - torch| keypoints {d[0]:.3e}, pose code {d[1]:.3e}, rotation {d[2]:.3e}, translation {d[3]:.3e}")
        assert d[0] <= KP_TOL and d[1] <= THETA_TOL and d[2] <= R_TOL and d[3] <= KP_TOL
    assert float((fused[-1][3] - fused[0][3]).abs().max()) > 1e-3  # the hand did move


def test_two_runs_are_bitwise_equal_and_a_graph_replays_them():
    model, c, *_ = _case("small-k4-fp16")
    opt = _optimiser(model, c)
    args = _frame_args(c)
    with torch.no_grad():
        first = [x.clone() for x in opt.optimize(*args)]  # (also the warm-up: tables, workspace, LDS attribute)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            second = [x.clone() for x in opt.optimize(*args)]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = opt.optimize(*args)
        graph.replay()
        torch.cuda.synchronize()
    assert opt.use_kernel() and all(bool(torch.isfinite(x).all()) for x in first)
    for a, b, g in zip(first, second, out):
        assert torch.equal(a, b) and torch.equal(a, g)
    assert float((first[1] - args[0]).abs().max()) > 0  # the pose code moved: candidates were better


def test_lockstep_batches_fall_back_to_single_calls(capsys):
    model, c, *_ = _case("small-k4-fp16")
    opt = _optimiser(model, c)
    with torch.no_grad():
        one = opt.optimize(*_frame_args(c))
        two = opt.optimize_batch([_frame_args(c), None, _frame_args(c)])
    assert "MANO entries" in capsys.readouterr().out and two[1] is None
    for k in (0, 2):
        assert all(torch.equal(a, b) for a, b in zip(one, two[k]))
