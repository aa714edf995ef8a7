"""GPU: the batched hand-pose optimiser (hotrack_amd.ext.hand_pose_opt_batch, pn2x_hand_pose_opt_batch;
gf_optimize_hand_pose.optimize_batch) against S single calls (ext.hand_pose_opt / optimize()): the same device functions run in
both, so every comparison here is of BITS -- states and traces -- never of values to a tolerance.  The problems of a batch differ
in everything the record holds (state, shape of the rest hand, keypoints, a previous frame or none, object pose, volume, mask
size, intrinsics); shapes are the smallest that reach every path: V 40 / 70, K 1 / 2 / 4, res 9 / 17, masks 12x16 and 16x24,
P 1 (no better candidate: the update's "no success" selects), 6 and 260 (no multiples of four), 64."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from _hand_pose_cases import BETA, C2, F16, F32, KP_TOL, R_TOL, THETA_TOL, make_case, to_kernel  # noqa: E402

pytestmark = pytest.mark.gpu
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}
MASKS = ((12, 16), (16, 24))
_PROBLEMS = {}


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _problem(q, P, V, K, res, dt):
    """Problem q of a batch with the shared sizes (P, V, K, res, dt): (frame dict of GPU tensors, initial state (90,) on the GPU).
    Per q: its own seed (state, keypoints, visibility, object pose), mask size, focal length and principal point, a rest hand
    scaled by 1 + 0.03 q (a shape), no previous frame for odd q, and a volume of its own from q = 2 on (problems 0 and 1 share
    one tensor)."""
    key = (q, P, V, K, res, dt)
    if key not in _PROBLEMS:
        h, w = MASKS[q % 2]
        c = make_case(P, V, K, res, dt, h, w, seed=100 + q, last_kp=q % 2 == 0, vis=("mixed", "all", "none")[q % 3], focal=18.0 + 3 * q,
                      centred=q % 2 == 1)
        fr = to_kernel(c)
        fr["rest"] = tuple((r * (1 + 0.03 * q)).contiguous() for r in fr["rest"])
        if q >= 2:
            fr["volume"] = (fr["volume"].float() + 0.0015 * q).to(dt).contiguous()
        _PROBLEMS[key] = (fr, c.state.cuda())
    return _PROBLEMS[key]


def _batch(S, P, V, K, res, dt):
    """-> (model, frames, states (S, 90)): one model, one `pre`, problems 0 and 1 on one volume tensor."""
    probs = [_problem(q, P, V, K, res, dt) for q in range(S)]
    model, pre, vol = probs[0][0]["model"], probs[0][0]["pre"], probs[0][0]["volume"]
    frames = []
    for q, (fr, _) in enumerate(probs):
        fr = {k: v for k, v in fr.items() if k != "model"}
        fr["pre"] = pre
        if q == 1:
            fr["volume"] = vol
        frames.append(fr)
    return model, frames, torch.stack([s for _, s in probs]).contiguous()


def _singles(model, frames, states, iterations):
    """Every problem alone through ext.hand_pose_opt -> (states (S, 90), traces (S, iterations, 19)); None entries stay."""
    from hotrack_amd import ext
    out, traces = states.clone(), torch.zeros((len(frames), iterations, 19), device="cuda")
    for q, fr in enumerate(frames):
        if fr is not None:
            traces[q] = ext.hand_pose_opt(model=model, state=out[q], iterations=iterations, scaling_coefficient2=C2, beta=BETA, trace=True, **fr)
    return out, traces


def _shape_of(i):
    """V, K, res of sweep row i, on periods (6, 3, 10) against the sweep's (2, 4, 16, 64): every value of each meets every dtype,
    iteration count, P and S."""
    return (40, 70)[(i // 3) % 2], (1, 2, 4)[i % 3], (9, 17)[(i // 5) % 2]


SWEEP = [(S, P, it, dt) for S in (1, 2, 3, 5) for P in (1, 6, 64, 260) for it in (1, 3) for dt in (F16, F32)]


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=["S%d-P%d-it%d-%s" % (S, P, it, "fp16" if dt == F16 else "fp32") for S, P, it, dt in SWEEP])
def test_batch_equals_single_calls_bit_for_bit(i):
    from hotrack_amd import ext
    S, P, it, dt = SWEEP[i]
    V, K, res = _shape_of(i)
    model, frames, states = _batch(S, P, V, K, res, dt)
    want, want_tr = _singles(model, frames, states, it)
    got = states.clone()
    tr = ext.hand_pose_opt_batch(model, frames, got, it, C2, BETA, trace=True)
    assert tr.shape == (S, it, 19)
    assert np.array_equal(_bits(got), _bits(want)), f"states differ (V {V}, K {K}, res {res})"
    assert np.array_equal(_bits(tr), _bits(want_tr)), f"traces differ (V {V}, K {K}, res {res})"
    assert torch.isfinite(got).all()
    if P == 1:   # no candidate can be better than candidate 0: pose unchanged, "previous success" cleared
        assert np.array_equal(_bits(got[:, :57]), _bits(states[:, :57])) and bool((got[:, 89] == 0).all()) and bool((tr[:, :, 2] == 0).all())
    if P >= 64:  # (the comparison is of an optimiser that moves)
        assert bool((tr[:, :, 2] == 1).any()) and not np.array_equal(_bits(got[:, :57]), _bits(states[:, :57]))
    assert ext.hand_pose_opt_batch(model, frames, states.clone(), it, C2, BETA) is None


def test_problems_differ_where_the_record_does():
    """The batch of the sweep is not S copies of one problem."""
    model, frames, states = _batch(5, 64, 70, 2, 17, F16)
    assert frames[0]["volume"] is frames[1]["volume"] and frames[2]["volume"] is not frames[0]["volume"]
    assert not torch.equal(frames[2]["volume"], frames[3]["volume"])
    assert {tuple(f["mask"].shape) for f in frames} == set(MASKS)
    assert [f["last_kp"] is None for f in frames] == [False, True, False, True, False]
    assert len({f["proj"]["fx"] for f in frames}) == 5 and len({float(f["rest"][0].abs().sum()) for f in frames}) == 5
    assert len({float(f["obj_t"].sum()) for f in frames}) == 5 and len({float(s.sum()) for s in states}) == 5


@pytest.mark.parametrize("sit_out", [(0, 2, 4), (0, 1, 2, 3, 4)], ids=["first-middle-last", "all"])
def test_inactive_problems_are_not_touched(sit_out):
    from hotrack_amd import ext
    model, frames, states = _batch(5, 64, 70, 2, 17, F16)
    frames = [None if q in sit_out else fr for q, fr in enumerate(frames)]
    want, want_tr = _singles(model, frames, states, 3)
    got = states.clone()
    tr = ext.hand_pose_opt_batch(model, frames, got, 3, C2, BETA, trace=True)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(tr), _bits(want_tr))
    for q in sit_out:
        assert np.array_equal(_bits(got[q]), _bits(states[q])) and not bool(tr[q].any())
    if len(sit_out) == 5:   # nobody active: no launch (the profile hook sees every launch of the binding)
        from hotrack_amd import pointnet2_hip
        pointnet2_hip.PROFILE = []
        try:
            ext.hand_pose_opt_batch(model, frames, got, 3, C2, BETA)
            assert pointnet2_hip.PROFILE == []
        finally:
            pointnet2_hip.PROFILE = None


def test_permuting_the_problems_permutes_the_results():
    from hotrack_amd import ext
    model, frames, states = _batch(5, 260, 40, 4, 9, F32)
    base = states.clone()
    base_tr = ext.hand_pose_opt_batch(model, frames, base, 3, C2, BETA, trace=True)
    perm = [3, 0, 4, 2, 1]
    got = states[perm].contiguous()
    tr = ext.hand_pose_opt_batch(model, [frames[q] for q in perm], got, 3, C2, BETA, trace=True)
    assert np.array_equal(_bits(got), _bits(base[perm])) and np.array_equal(_bits(tr), _bits(base_tr[perm]))


def test_a_second_call_with_the_same_buffers_gives_the_same_bits():
    from hotrack_amd import ext
    model, frames, states = _batch(3, 260, 70, 2, 17, F16)
    runs = []
    for _ in range(2):
        st = states.clone()
        tr = ext.hand_pose_opt_batch(model, frames, st, 3, C2, BETA, trace=True)
        runs.append((_bits(st), _bits(tr)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_capture_and_replay_reads_the_persistent_buffers():
    """One captured call (a linear graph: one stream, launches only); the frames' tensors are the persistent buffers.  A replay
    after new keypoints were copied into them equals an eager call on the new inputs."""
    from hotrack_amd import ext
    model, frames, states = _batch(3, 64, 70, 2, 17, F16)
    frames = [dict(fr, pred_kp=fr["pred_kp"].clone()) for fr in frames]   # (the cached problems stay as they are)
    buf = states.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.hand_pose_opt_batch(model, frames, buf, 3, C2, BETA, trace=True)   # warm-up: LDS attribute, compute-unit count
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    buf.copy_(states)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr = ext.hand_pose_opt_batch(model, frames, buf, 3, C2, BETA, trace=True)
    for step in range(2):
        for q, fr in enumerate(frames):
            fr["pred_kp"].add_(0.002 * (step + 1) * (q + 1))
        buf.copy_(states)
        graph.replay()
        want = states.clone()
        want_tr = ext.hand_pose_opt_batch(model, frames, want, 3, C2, BETA, trace=True)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(buf), _bits(want)) and np.array_equal(_bits(tr), _bits(want_tr)), step
    first, _ = _singles(model, [dict(fr, pred_kp=_problem(q, 64, 70, 2, 17, F16)[0]["pred_kp"]) for q, fr in enumerate(frames)], states, 3)
    assert not np.array_equal(_bits(buf), _bits(first))   # (the new keypoints do change the result)


def test_mixed_volumes_are_refused_naming_both_entries():
    from hotrack_amd import ext
    model, frames, states = _batch(3, 6, 40, 2, 9, F16)
    other_res = _batch(3, 6, 40, 2, 17, F16)[1][2]["volume"]
    cases = {"volume resolution": dict(volume=other_res), "volume dtype": dict(volume=frames[2]["volume"].float()),
             "voxel_scale": dict(voxel_scale=2 * frames[2]["voxel_scale"])}
    for what, change in cases.items():
        bad = [frames[0], None, dict(frames[2], **change)]
        st = states.clone()
        with pytest.raises(ValueError, match=r"frames\[0\] and frames\[2\] differ in " + what):
            ext.hand_pose_opt_batch(model, bad, st, 1, C2, BETA)
        assert np.array_equal(_bits(st), _bits(states))   # refused before any launch
    with pytest.raises(ValueError, match=r"states .* is not \(3, 90\)"):
        ext.hand_pose_opt_batch(model, frames, states[:2].contiguous(), 1, C2, BETA)
    with pytest.raises(ValueError, match=r"frames\[1\] lacks"):
        ext.hand_pose_opt_batch(model, [frames[0], {"pre": frames[0]["pre"]}, frames[2]], states.clone(), 1, C2, BETA)


def _setup(hand_model=None):
    """The committed fixture's optimiser on the device-resident route, as tests/test_gpu_hand_pose.py sets it up."""
    from models.hand_model import SyntheticLBSHand
    from models.optimization_hand import gf_optimize_hand_pose
    g = np.load(os.path.join(ROOT, "tests", "golden", "hand_opt_sequence.npz"))
    res, stride = int(g["meta"][0]), float(g["meta"][1])
    cfg = {"device": "cuda", "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": True}}
    opt = gf_optimize_hand_pose(cfg, hand_model=hand_model or SyntheticLBSHand(), particle_size=g["pre_sampled_particle"].shape[0])
    opt.pre_sampled_particle = torch.from_numpy(g["pre_sampled_particle"]).cuda()
    opt.load_volume(torch.from_numpy(g["volume"]).reshape(res, res, res), stride)
    proj = dict(zip(("fx", "fy", "cx", "cy", "w", "h"), g["proj"].tolist()))
    obj_pose = {"rotation": torch.from_numpy(g["R_obj"])[None].cuda(), "translation": torch.from_numpy(g["t_obj"]).reshape(1, 3, 1).cuda()}
    return g, opt, proj, obj_pose, torch.from_numpy(g["background_mask"]).cuda()


def _frame_inputs(g, f):
    t = lambda k: torch.from_numpy(g[f"f{f}_{k}"]).cuda()
    last = g[f"f{f}_last_kp"]
    return (t("init_mano"), {"rotation": t("init_rot"), "translation": t("init_trans")}, t("init_kp"),
            None if last.size == 0 else torch.from_numpy(last).cuda(), t("vis_mask"))


def test_optimize_batch_of_one_on_the_committed_fixture():
    """tests/golden/hand_opt_sequence.npz through optimize_batch with S = 1: inside the tolerances tests/test_gpu_hand_pose.py
    applies to optimize() (2e-5 keypoints / translation, 4e-4 pose code, 1e-4 rotation) and bit-equal to optimize()."""
    runs = {}
    for batched in (False, True):
        g, opt, proj, obj_pose, mask = _setup()
        assert opt.use_kernel()
        out, prev = [], None
        with torch.no_grad():
            for f in range(4):
                mano, pose, kp0, _, vis = _frame_inputs(g, f)
                args = (mano, pose, kp0, prev, vis, obj_pose, None, proj, mask)
                res = opt.optimize_batch([args])[0] if batched else opt.optimize(*args)
                out.append([x.clone() for x in res])
                prev = res[0]
        runs[batched] = out
    for f in range(4):
        kp, theta, R, t = (x.cpu().numpy() for x in runs[True][f])
        np.testing.assert_allclose(kp, g[f"f{f}_final_kp"], rtol=0, atol=KP_TOL, err_msg=f"frame {f} keypoints")
        np.testing.assert_allclose(theta, g[f"f{f}_theta"], rtol=0, atol=THETA_TOL, err_msg=f"frame {f} pose code")
        np.testing.assert_allclose(R, g[f"f{f}_R"], rtol=0, atol=R_TOL, err_msg=f"frame {f} rotation")
        np.testing.assert_allclose(t, g[f"f{f}_t"], rtol=0, atol=KP_TOL, err_msg=f"frame {f} translation")
        for a, b in zip(runs[True][f], runs[False][f]):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"frame {f}"


def test_optimize_batch_keeps_shape_volume_and_none_per_sequence():
    """Three entries with their own shape code and volume, one None: each equals optimize() on an optimiser set up for it alone,
    and the hand model's registered shape is what it was."""
    from models.hand_model import SyntheticLBSHand
    g, _, proj, obj_pose, mask = _setup()
    res, stride = int(g["meta"][0]), float(g["meta"][1])
    vol = torch.from_numpy(g["volume"]).reshape(res, res, res).cuda()
    vols = [vol, (vol.float() + 0.002).to(vol.dtype), vol]
    betas = [torch.linspace(-1, 1, 10)[None] * s for s in (0.5, -1.0, 1.5)]
    fresh = lambda: _setup(SyntheticLBSHand(num_betas=10))[1]

    calls, want = [], []
    with torch.no_grad():
        for k in range(3):
            mano, pose, kp0, last, vis = _frame_inputs(g, k)
            calls.append(dict(init_mano=mano, init_hand_pose=pose, init_kp=kp0, last_frame_kp=last, vis_mask=vis, init_obj_pose=obj_pose,
                              hand_shape=betas[k], projection=proj, background_mask=mask, sdf_volume=vols[k], voxel_scale=stride))
            opt = fresh()
            opt.load_volume(vols[k], stride)
            want.append([x.clone() for x in opt.optimize(**{a: v for a, v in calls[k].items() if a not in ("sdf_volume", "voxel_scale")})])
        opt = fresh()
        opt.load_volume(vol, stride)
        opt.mano_layer_right.register_beta(torch.full((1, 10), 0.25))
        got = opt.optimize_batch([calls[0], None, calls[1], calls[2]])
    assert got[1] is None and torch.equal(opt.mano_layer_right.registered_beta.cpu(), torch.full((1, 10), 0.25))
    assert opt.sdf_volume is vol
    for k, res_k in zip((0, 1, 2), (got[0], got[2], got[3])):
        for a, b in zip(res_k, want[k]):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
    assert not np.array_equal(_bits(want[0][0]), _bits(want[2][0]))
