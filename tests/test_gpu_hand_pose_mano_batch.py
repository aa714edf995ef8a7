"""GPU: the batched MANO hand-pose optimiser (hotrack_amd.ext.hand_pose_mano_opt_batch, pn2x_hand_pose_mano_opt_batch;
gf_optimize_hand_pose.optimize_batch with opt.lockstep_mano) against S single calls on the MANO route (ext.hand_pose_opt /
optimize()): the same device functions run in both and every output element of the pose-offset pre-pass is the same sequence of
matrix-core accumulations whatever the grid, so every comparison here is of BITS -- states and traces -- never of values to a
tolerance.  The hand is SyntheticManoHand(num_verts=97) with one fingertip at vertex 96: 97 vertices are 19 row tiles of the
pre-pass, no multiple of 4, so its wave-strided tile loop and the grid's y both meet a remainder.  The problems of a batch differ
in everything the record holds (state, shape of the rest hand, keypoints, a previous frame or none, object pose, volume, mask
size, intrinsics); P 1 (no better candidate: the update's "no success" selects), 6 (less than one 16-row group of the
pre-pass), 67 (one full group of 64 candidates plus 3), 130 (the last group nearly empty); K 1 / 4; res 9 / 17 in fp16 / fp32."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import _hand_pose_cases as C  # noqa: E402
from _hand_pose_cases import BETA, C2, F16, F32  # noqa: E402

from models.hand_model import SyntheticManoHand, rodrigues  # noqa: E402

pytestmark = pytest.mark.gpu
V, TIPS = 97, (5, 20, 40, 60, 96)
MASKS = ((12, 16), (16, 24))
PRE_SEED = 100
_MODELS, _CASES, _FRAMES = {}, {}, {}


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _hand(K):
    if K not in _MODELS:
        _MODELS[K] = SyntheticManoHand(num_verts=V, weights_per_vertex=K, tip_vertices=TIPS)
    return _MODELS[K]


def mano_case(q, K, res, dt):
    """Problem q on the CPU, for any number of candidates (the candidates are the batch's, the first P rows of one seeded
    table): tests/_hand_pose_cases.make_case's scene around a MANO-structured hand.  Per q: its own seed (state, keypoints,
    object pose), visibility pattern, mask size, focal length and principal point, a rest hand scaled by 1 + 0.03 q (a shape),
    no previous frame for odd q, and from q = 2 on a volume moved by 1.5 mm q."""
    key = (q, K, res, dt)
    if key in _CASES:
        return _CASES[key]
    h, w = MASKS[q % 2]
    focal, centred, vis = 18.0 + 3 * q, q % 2 == 1, ("mixed", "all", "none")[q % 3]
    base = _hand(K).skinning_tables()
    assert base is not None and base["skin_idx"].shape == (V, K) and int(base["kp_vertex"].max()) == V - 1
    c = SimpleNamespace(name=f"mano-q{q}-K{K}-res{res}", V=V, K=K, res=res, h=h, w=w, theta_scale=C.THETA_SCALE,
                        weights=dict(C.ENERGY_WEIGHT), tables=dict(base))
    c.tables["rest_joints"] = (base["rest_joints"].float() * (1 + 0.03 * q)).contiguous()
    c.tables["rest_verts"] = (base["rest_verts"].float() * (1 + 0.03 * q)).contiguous()
    g = torch.Generator().manual_seed(100 + q)
    R0 = rodrigues(torch.tensor((0.25, -0.3, 0.35), dtype=torch.float64)).float()
    c.state = C.pack_state(R0, torch.tensor((-0.02, -0.09, 0.5)), 0.15 * torch.randn(45, generator=g), torch.full((16,), 0.005))
    v0, k0 = (x[0] for x in C.reference_geometry(SimpleNamespace(tables=c.tables, state=c.state, pre=torch.zeros(1, 16),
                                                                 theta_scale=C.THETA_SCALE)))
    c.pred_kp = (k0.float() + torch.tensor([0.006, -0.004, 0.005]) + 0.002 * torch.randn(21, 3, generator=g)).contiguous()
    c.last_kp = (k0.float() + 0.003 * torch.randn(21, 3, generator=g)).contiguous() if q % 2 == 0 else None
    c.vis = torch.ones(21, dtype=torch.bool)
    if vis == "mixed":
        c.vis[[3, 8, 10, 20]] = False
    elif vis == "none":
        c.vis[:] = False
    # a sphere of 4 cm that candidate 0's palm penetrates by about a centimetre (tests/_hand_pose_cases.py: make_case)
    rad, c_obj = 0.04, torch.tensor([0.016, -0.012, 0.008], dtype=torch.float64)
    anchor = v0[(v0 - v0.mean(dim=0)).norm(dim=1).argmin()]
    centre = anchor + R0.double() @ torch.tensor([0.0, 0.0, rad - 0.012], dtype=torch.float64)
    Ro = rodrigues(torch.tensor([0.3 + 0.05 * q, -0.5, 0.4], dtype=torch.float64))
    c.obj_r, c.obj_t = Ro.float().contiguous(), (centre - Ro @ c_obj).float().contiguous()
    c.voxel_scale = round(0.25 / res, 4)
    ax = (torch.arange(res, dtype=torch.float64) - res // 2 + 0.5) * c.voxel_scale
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c.volume = (torch.sqrt((X - c_obj[0]) ** 2 + (Y - c_obj[1]) ** 2 + (Z - c_obj[2]) ** 2) - rad + (0.0015 * q if q >= 2 else 0.0)).to(dt).contiguous()
    cx, cy = w / 2.0, h / 2.0
    if centred:
        mid = v0.mean(dim=0)
        cx, cy = round(cx - float(mid[0] / mid[2]) * focal, 2), round(cy - float(mid[1] / mid[2]) * focal, 2)
    c.proj = {"fx": focal, "fy": focal, "cx": cx, "cy": cy, "w": w, "h": h}
    px, py = v0[:, 0] / v0[:, 2] * focal + cx, v0[:, 1] / v0[:, 2] * focal + cy
    mx, my = float(px.median()), float(py.median())
    a, b = min(max(1.2 * float(px.std()), 6.0), w / 3.0), min(max(1.2 * float(py.std()), 6.0), h / 3.0)
    rows, cols = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    c.mask = (((cols - mx) / a) ** 2 + ((rows - my) / b) ** 2 > 1) | ((cols - mx - 0.3 * (rows - my)).abs() < 0.15 * a)
    _CASES[key] = c
    return c


def candidates(P):
    return C._pre_rows(P, PRE_SEED)


def _batch(S, P, K, res, dt):
    """-> (model, frames, states (S, 90)) on the GPU: one model, one `pre`, problems 0 and 1 on one volume tensor."""
    from hotrack_amd import ext
    key = (K, res, dt)
    if key not in _FRAMES:
        _FRAMES[key] = {"model": ext.hand_pose_model(mano_case(0, K, res, dt).tables, "cuda"), "pre": candidates(C.MAXP).cuda()}
    store = _FRAMES[key]
    frames, states = [], []
    for q in range(S):
        if q not in store:
            c = mano_case(q, K, res, dt)
            fr = C.to_kernel(SimpleNamespace(**vars(c), pre=torch.zeros(1, 16)))   # (its own model: only the scaled rest hand is kept)
            del fr["model"], fr["pre"]
            store[q] = (fr, c.state.cuda())
        fr = dict(store[q][0], pre=store["pre"][:P])
        if q == 1:
            fr["volume"] = store[0][0]["volume"]
        frames.append(fr)
        states.append(store[q][1])
    return store["model"], frames, torch.stack(states).contiguous()


def _singles(model, frames, states, iterations):
    """Every problem alone through ext.hand_pose_opt (the single MANO kernels) -> (states, traces); None entries stay."""
    from hotrack_amd import ext
    out, traces = states.clone(), torch.zeros((len(frames), iterations, 19), device="cuda")
    for q, fr in enumerate(frames):
        if fr is not None:
            traces[q] = ext.hand_pose_opt(model=model, state=out[q], iterations=iterations, scaling_coefficient2=C2, beta=BETA, trace=True, **fr)
    return out, traces


def _shape_of(i):
    """K, res of sweep row i, on periods (6, 10) against the sweep's (2, 4, 16, 64): every value of each meets every dtype,
    iteration count, P and S, and every K every res."""
    return (1, 4)[(i // 3) % 2], (9, 17)[(i // 5) % 2]


SWEEP = [(S, P, it, dt) for S in (1, 2, 3, 5) for P in (1, 6, 67, 130) for it in (1, 3) for dt in (F16, F32)]


def test_every_value_of_the_sweep_meets_every_other():
    rows = [(*SWEEP[i], *_shape_of(i)) for i in range(len(SWEEP))]
    for a in range(6):
        for b in range(a + 1, 6):
            va, vb = {r[a] for r in rows}, {r[b] for r in rows}
            assert {(r[a], r[b]) for r in rows} == {(x, y) for x in va for y in vb}, (a, b)


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=["S%d-P%d-it%d-%s" % (S, P, it, "fp16" if dt == F16 else "fp32") for S, P, it, dt in SWEEP])
def test_batch_equals_single_calls_bit_for_bit(i):
    from hotrack_amd import ext
    S, P, it, dt = SWEEP[i]
    K, res = _shape_of(i)
    model, frames, states = _batch(S, P, K, res, dt)
    assert model["mano"] and model["mano_ok"]
    want, want_tr = _singles(model, frames, states, it)
    got = states.clone()
    tr = ext.hand_pose_mano_opt_batch(model, frames, got, it, C2, BETA, trace=True)
    assert tr.shape == (S, it, 19)
    assert np.array_equal(_bits(got), _bits(want)), f"states differ (K {K}, res {res})"
    assert np.array_equal(_bits(tr), _bits(want_tr)), f"traces differ (K {K}, res {res})"
    assert torch.isfinite(got).all()
    if P == 1:   # no candidate can be better than candidate 0: pose unchanged, "previous success" cleared
        assert np.array_equal(_bits(got[:, :57]), _bits(states[:, :57])) and bool((got[:, 89] == 0).all()) and bool((tr[:, :, 2] == 0).all())
    if P >= 64:  # (the comparison is of an optimiser that moves)
        assert bool((tr[:, :, 2] == 1).any()) and not np.array_equal(_bits(got[:, :57]), _bits(states[:, :57]))
    assert ext.hand_pose_mano_opt_batch(model, frames, states.clone(), it, C2, BETA) is None


def test_problems_differ_where_the_record_does():
    """The batch of the sweep is not S copies of one problem."""
    model, frames, states = _batch(5, 67, 4, 17, F16)
    assert frames[0]["volume"] is frames[1]["volume"] and frames[2]["volume"] is not frames[0]["volume"]
    assert not torch.equal(frames[2]["volume"], frames[3]["volume"])
    assert {tuple(f["mask"].shape) for f in frames} == set(MASKS)
    assert [f["last_kp"] is None for f in frames] == [False, True, False, True, False]
    assert len({f["proj"]["fx"] for f in frames}) == 5 and len({float(f["rest"][0].abs().sum()) for f in frames}) == 5
    assert len({float(f["obj_t"].sum()) for f in frames}) == 5 and len({float(s.sum()) for s in states}) == 5


def _workspace(model, S, P, fill):
    from hotrack_amd import ext
    return ext.hand_pose_mano_batch_workspace(P, model["V"], S, "cuda").fill_(fill)


@pytest.mark.parametrize("sit_out", [(0,), (2,), (4,), (0, 2, 4), (0, 1, 2, 3, 4)], ids=["first", "middle", "last", "first-middle-last", "all"])
def test_inactive_problems_are_not_touched(sit_out):
    from hotrack_amd import ext
    S, P = 5, 67
    model, frames, states = _batch(S, P, 4, 17, F16)
    frames = [None if q in sit_out else fr for q, fr in enumerate(frames)]
    want, want_tr = _singles(model, frames, states, 3)
    got, ws = states.clone(), _workspace(model, S, P, float("nan"))
    tr = ext.hand_pose_mano_opt_batch(model, frames, got, 3, C2, BETA, trace=True, offsets=ws)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(tr), _bits(want_tr))
    slices = ws.view(S, -1)
    for q in range(S):
        if q in sit_out:   # rows and trace untouched, the slice of the workspace still what it was filled with
            assert np.array_equal(_bits(got[q]), _bits(states[q])) and not bool(tr[q].any()) and bool(torch.isnan(slices[q]).all()), q
        else:              # (a slice is P rows of ceil16(3 V) floats, and the pre-pass writes every one)
            assert bool(torch.isfinite(slices[q]).all()), q
    if len(sit_out) == S:   # nobody active: no launch (the profile hook sees every launch of the binding)
        from hotrack_amd import pointnet2_hip
        pointnet2_hip.PROFILE = []
        try:
            ext.hand_pose_mano_opt_batch(model, frames, got, 3, C2, BETA, offsets=ws)
            assert pointnet2_hip.PROFILE == []
        finally:
            pointnet2_hip.PROFILE = None


def test_the_result_does_not_depend_on_what_the_workspace_held():
    """NaN and 1e30 in the offsets workspace before the call: the same bits, so every element the evaluation reads is one the
    pre-pass wrote."""
    from hotrack_amd import ext
    S, P = 3, 130
    model, frames, states = _batch(S, P, 4, 17, F32)
    want, want_tr = _singles(model, frames, states, 3)
    for fill in (float("nan"), 1e30):
        got = states.clone()
        tr = ext.hand_pose_mano_opt_batch(model, frames, got, 3, C2, BETA, trace=True, offsets=_workspace(model, S, P, fill))
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(tr), _bits(want_tr)), fill
    with pytest.raises(ValueError, match="offsets has"):
        ext.hand_pose_mano_opt_batch(model, frames, states.clone(), 3, C2, BETA, offsets=_workspace(model, S - 1, P, 0.0))


def test_permuting_the_problems_permutes_the_results():
    from hotrack_amd import ext
    model, frames, states = _batch(5, 130, 1, 9, F32)
    base = states.clone()
    base_tr = ext.hand_pose_mano_opt_batch(model, frames, base, 3, C2, BETA, trace=True)
    perm = [3, 0, 4, 2, 1]
    got = states[perm].contiguous()
    tr = ext.hand_pose_mano_opt_batch(model, [frames[q] for q in perm], got, 3, C2, BETA, trace=True)
    assert np.array_equal(_bits(got), _bits(base[perm])) and np.array_equal(_bits(tr), _bits(base_tr[perm]))


# ---- gf_optimize_hand_pose.optimize_batch with opt.lockstep_mano ------------------------------------------------------------------
P_OPT = 67


def _optimiser(lockstep=True):
    from models.optimization_hand import gf_optimize_hand_pose
    c = mano_case(0, 4, 17, F16)
    cfg = {"device": "cuda", "opt": {"energy_weight": dict(C.ENERGY_WEIGHT), "fused_pose": True, "lockstep_mano": lockstep}}
    opt = gf_optimize_hand_pose(cfg, hand_model=copy.deepcopy(_hand(4)), particle_size=P_OPT)
    opt.pre_sampled_particle = candidates(P_OPT).cuda()
    opt.load_volume(c.volume, c.voxel_scale)
    assert opt.use_kernel() and opt._kernel_model()["mano"] and opt.lockstep_mano == lockstep
    return opt


def _call(q, own_volume):
    """Problem q as an optimize_batch entry (a dict by name); the model's own rest hand with a shape code for q > 0."""
    c, dev = mano_case(q, 4, 17, F16), "cuda"
    st = c.state.to(dev)
    g = torch.Generator().manual_seed(500 + q)
    call = dict(init_mano=st[C.S_THETA:C.S_THETA + 45].view(1, 45).clone(),
                init_hand_pose={"rotation": st[C.S_R:C.S_R + 9].view(1, 3, 3).clone(), "translation": st[C.S_T:C.S_T + 3].view(1, 3).clone()},
                init_kp=c.pred_kp[None].to(dev), last_frame_kp=None if c.last_kp is None else c.last_kp[None].to(dev),
                vis_mask=c.vis[None].to(dev), init_obj_pose={"rotation": c.obj_r[None].to(dev), "translation": c.obj_t.reshape(1, 3, 1).to(dev)},
                hand_shape=None if q == 0 else (0.5 * torch.randn(1, 10, generator=g)).to(dev), projection=c.proj,
                background_mask=c.mask.to(dev))
    if own_volume:
        call.update(sdf_volume=c.volume.to(dev), voxel_scale=c.voxel_scale)
    return call


def _calls():
    return [_call(0, False), None, _call(2, True)]


def _one_by_one(calls):
    """optimize() per entry, each on an optimiser of its own with the entry's volume loaded."""
    out = []
    for call in calls:
        if call is None:
            out.append(None)
            continue
        opt = _optimiser(False)
        opt.mano_layer_right.register_beta(torch.full((1, 10), 0.25))
        if "sdf_volume" in call:
            opt.load_volume(call["sdf_volume"], call["voxel_scale"])
        out.append([x.clone() for x in opt.optimize(**{k: v for k, v in call.items() if k not in ("sdf_volume", "voxel_scale")})])
    return out


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        for x, y in zip(a or (), b or ()):
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def test_optimize_batch_runs_mano_sequences_in_lockstep(capsys):
    from hotrack_amd import pointnet2_hip
    calls = _calls()
    with torch.no_grad():
        want = _one_by_one(calls)
        opt = _optimiser()
        opt.mano_layer_right.register_beta(torch.full((1, 10), 0.25))
        capsys.readouterr()
        pointnet2_hip.PROFILE = []
        try:
            got = opt.optimize_batch(calls)
            names = [p[0] for p in pointnet2_hip.PROFILE]
        finally:
            pointnet2_hip.PROFILE = None
        got = [None if r is None else [x.clone() for x in r] for r in got]
        assert capsys.readouterr().out == ""
        assert names.count("hand_pose_problems_fill") == 1 and names.count("hand_pose_mano_opt_batch") == 1
        assert "hand_pose_opt" not in names and "hand_pose_opt_batch" not in names
        assert got[1] is None and torch.equal(opt.mano_layer_right.registered_beta.cpu(), torch.full((1, 10), 0.25))
        _same(got, want)
        assert not np.array_equal(_bits(got[0][1]), _bits(calls[0]["init_mano"]))   # the pose code moved: candidates were better
        assert not np.array_equal(_bits(got[0][0]), _bits(got[2][0]))
        assert opt._mano_batch_work_key == (3, P_OPT, V) and opt._mano_batch_work.numel() == 3 * P_OPT * 304
        # a second call: the same bits, no host sync, the workspace kept
        ws = opt._mano_batch_work
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            second = [None if r is None else [x.clone() for x in r] for r in opt.optimize_batch(calls)]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        _same(second, want)
        assert opt._mano_batch_work is ws
        # a captured call (one stream, launches only) replays to the eager result
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = opt.optimize_batch(calls)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, want)
