"""GPU: the observed surface of tracked object sequences (network/models/obs_surface.py, opt.accumulate_surface of
ObjTrackModel_Optimization): the tracked poses do not depend on the switch, the merged cloud keeps its size, `add` against a
numpy restatement given the same random draws, a frame in which nothing passes the filter, lockstep groups against single
sequences, and no host synchronisation in `add`.  Small: a 41^3 volume, 256 points, 4 frames."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import _cloud_normals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

pytestmark = pytest.mark.gpu
RES, STRIDE, N = 41, 0.01, 256
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}
NEW_COLUMNS = {"obs_surface_residual(mm)", "obs_surface_normal_agree"}


def _cfg(on):
    return {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False, "accumulate_surface": on},
            "num_points": N, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt"}


def _sequences(count=2, frames=4):
    from datasets.synthetic import SyntheticObjectSequences
    data = SyntheticObjectSequences(_cfg(False), count, frames, res=RES, stride=STRIDE)
    return [data[s] for s in range(count)]


def _model(on):
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    model = ObjTrackModel_Optimization(_cfg(on))
    model.optimizer = gf_optimize_obj(_cfg(on), seed=7)
    model.optimizer.volume_size = RES
    return model


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


@pytest.fixture(scope="module")
def tracked():
    """Sequence 0 tracked with the switch off and on, each on a fresh model with the same particles."""
    out = {}
    with torch.no_grad():
        for on in (False, True):
            seq = copy.deepcopy(_sequences(1)[0])
            model = _model(on)
            rets = model(seq, dict(FLAGS))
            out[on] = (rets, model.compute_loss(seq, rets, dict(FLAGS))[0])
    return out


def test_poses_do_not_depend_on_the_switch(tracked):
    (off, loss_off), (on, loss_on) = tracked[False], tracked[True]
    assert len(off) == len(on) == 4
    for a, b in zip(off, on):
        assert np.array_equal(_bits(a["rotation"]), _bits(b["rotation"])) and np.array_equal(_bits(a["translation"]), _bits(b["translation"]))
    assert "obj_surface" not in off[0] and not NEW_COLUMNS & loss_off.keys()
    assert NEW_COLUMNS <= loss_on.keys() and loss_on.keys() - NEW_COLUMNS == loss_off.keys()
    for k in loss_off:
        assert float(loss_off[k]) == float(loss_on[k]), k
    surf = on[0]["obj_surface"]
    assert {"points", "normals", "frames"} <= surf.keys() and surf["frames"] == 5   # start, then one add per frame
    assert surf["points"].shape == (N, 3) and surf["normals"].shape == (N, 3) and surf["points"].is_cuda
    # the capsule's own clouds under poses a few millimetres off: the merged points lie on the model, the normals exist
    assert 0 <= loss_on["obs_surface_residual(mm)"] < 10 and 0 < loss_on["obs_surface_normal_agree"] <= 1 + 1e-5


def _tracked_surface(orient="view", seed=3):
    """A surface started on frame 0 of sequence 0 at its ground-truth pose, the volume and the sequence."""
    from hotrack_amd import sdf
    from models.obs_surface import ObservedSurface
    dev = torch.device("cuda", 0)
    seq = _sequences(1)[0]
    vol = sdf.CornerVolume(seq[0]["sdf_volume"].to(dev).contiguous())
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    surf = ObservedSurface(N, orient=orient, generator=gen)
    pose = lambda fr, dt=0.0: {"rotation": fr["gt_obj_pose"]["rotation"].reshape(1, 3, 3).to(dev),
                               "translation": fr["gt_obj_pose"]["translation"].reshape(1, 3, 1).to(dev) + dt}
    surf.start(seq[0]["obj_points"].to(dev), pose(seq[0]))
    return surf, vol, seq, pose, dev


def _unit_or_zero(normals):
    lens = normals.norm(dim=1)
    return bool((((lens - 1).abs() < 1e-5) | (lens == 0)).all())


def test_surface_keeps_its_size_and_counts_frames():
    surf, vol, seq, pose, dev = _tracked_surface(orient="reference")
    assert surf.frames == 1 and surf.points.shape == (N, 3) and _unit_or_zero(surf.normals) and (surf.normals.norm(dim=1) > 0).all()
    for t, fr in enumerate(seq):
        surf.add(fr["obj_points"].to(dev), pose(fr), vol, STRIDE)
        assert surf.frames == t + 2
        assert surf.points.shape == (N, 3) and surf.normals.shape == (N, 3)
        assert torch.isfinite(surf.points).all() and torch.isfinite(surf.normals).all() and _unit_or_zero(surf.normals)
    # choose = M // frames shrinks below a neighbourhood: two points get zero normals, then nothing is drawn any more
    surf.frames = N // 2 - 1
    surf.add(seq[0]["obj_points"].to(dev), pose(seq[0]), vol, STRIDE)
    assert int((surf.normals.norm(dim=1) == 0).sum()) == 2
    surf.frames = N
    before = surf.points.clone()
    surf.add(seq[0]["obj_points"].to(dev), pose(seq[0]), vol, STRIDE)
    assert surf.frames == N + 1 and torch.equal(before, surf.points)


def test_add_against_numpy_with_the_same_draws():
    from hotrack_amd import sdf
    from models.obs_surface import KEY_RANGE, to_object_frame
    tol_n = 4 * max(R.case_reference(c)[2] for c in R.CASES)
    surf, vol, seq, pose, dev = _tracked_surface(orient="view")
    rng = np.random.default_rng(9)
    for fr in seq[1:3]:
        cloud = fr["obj_points"].to(dev).clone()
        cloud[0, ::5] += 0.03   # a fifth of the points 3 cm off the surface: the filter has something to refuse
        draws = (rng.integers(0, KEY_RANGE, N), rng.integers(0, KEY_RANGE, N))
        old_p, old_n = surf.points.cpu().numpy().copy(), surf.normals.cpu().numpy().copy()
        pts, cam = to_object_frame(cloud, pose(fr))
        usable = (sdf.distance(pts, vol, STRIDE).abs() < 0.02).cpu().numpy()
        assert 0.7 * N < usable.sum() < 0.9 * N
        surf.add(cloud, pose(fr), vol, STRIDE, keys=tuple(torch.from_numpy(d).to(dev) for d in draws))
        # the restatement: python integers, so nothing about int64 is assumed
        choose = N // surf.frames
        new_keys = [int(draws[0][i]) * N + i + (0 if usable[i] else 1 << 62) for i in range(N)]
        slot_keys = [int(draws[1][i]) * N + i for i in range(N)]
        sel = sorted(range(N), key=new_keys.__getitem__)[:choose]
        slots = sorted(range(N), key=slot_keys.__getitem__)[:choose]
        p = pts.cpu().numpy()
        want_p, replaced = old_p.copy(), []
        for i, s in zip(sel, slots):
            if usable[i]:
                want_p[s] = p[i]
                replaced.append((i, s))
        assert usable[sel].all()   # (enough usable points: every drawn point passes, every drawn slot is replaced)
        got_p, got_n = surf.points.cpu().numpy(), surf.normals.cpu().numpy()
        assert np.array_equal(got_p.view(np.int32), want_p.view(np.int32))
        untouched = np.setdiff1d(np.arange(N), slots)
        assert np.array_equal(got_n[untouched].view(np.int32), old_n[untouched].view(np.int32))
        # normals: estimated among the chosen points only
        sub = p[sel]
        ref = R.normals_fp64(sub, 30)
        want_n = R.orient_numpy(ref["normal"], sub, cam.cpu().numpy(), "view")
        cmp = ref["compare"] & (np.abs((ref["normal"] * (cam.cpu().numpy().astype(np.float64) - sub)).sum(1)) > tol_n)
        assert cmp.sum() >= 0.95 * len(sel)
        got_new = got_n[np.array(slots)].astype(np.float64)
        n32 = R.normals_fp32(sub, ref["idx"], ref["usable"])[0]
        tol_here = min(tol_n, 4 * R.cross_norm(n32[cmp], ref["normal"][cmp]).max())   # the same rule, on these very points
        cross = R.cross_norm(got_new[cmp], ref["normal"][cmp]).max()
        print("add: %d points replaced, cross-norm %.3e (tol %.3e on these points, %.3e over the kernel test's cases)"
              % (len(replaced), cross, tol_here, tol_n))
        assert 0 < tol_here and cross <= tol_here
        assert ((got_new[cmp] * want_n[cmp]).sum(1) > 0).all()   # the sign rule, apart from the direction


def test_a_frame_that_fails_the_filter_changes_nothing():
    surf, vol, seq, pose, dev = _tracked_surface()
    surf.add(seq[1]["obj_points"].to(dev), pose(seq[1]), vol, STRIDE)
    p, n, frames = surf.points.clone(), surf.normals.clone(), surf.frames
    surf.add(seq[2]["obj_points"].to(dev), pose(seq[2], 0.5), vol, STRIDE)   # the pose 0.5 m off: no point within 2 cm
    assert surf.frames == frames + 1
    assert np.array_equal(_bits(surf.points), _bits(p)) and np.array_equal(_bits(surf.normals), _bits(n))


def test_lockstep_surfaces_equal_single_sequences():
    seqs = _sequences(2)
    seqs = [seqs[0][:3], seqs[1][:4]]
    alone = []
    with torch.no_grad():
        for seq in copy.deepcopy(seqs):
            rets = _model(True)(seq, dict(FLAGS))
            alone.append(rets[0]["obj_surface"])
        group = _model(True).forward_batch(copy.deepcopy(seqs), dict(FLAGS))
    for s in range(2):
        got = group[s][0]["obj_surface"]
        assert got["frames"] == alone[s]["frames"] == len(seqs[s]) + 1
        for key in ("points", "normals", "fit"):
            assert np.array_equal(_bits(got[key]), _bits(alone[s][key])), (s, key)
    assert not np.array_equal(_bits(alone[0]["points"]), _bits(alone[1]["points"]))


def test_add_issues_no_host_synchronisation():
    surf, vol, seq, pose, dev = _tracked_surface(orient="reference")
    cloud, ps = seq[1]["obj_points"].to(dev), pose(seq[1])
    surf.add(cloud, ps, vol, STRIDE)   # (first use: whatever is set up once)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        surf.add(cloud, ps, vol, STRIDE)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert surf.frames == 3


def test_save_writes_the_surface_into_the_sequences_pickle(tmp_path):
    import pickle
    seq = copy.deepcopy(_sequences(1)[0])
    model = _model(True)
    model.save_folder = str(tmp_path / "results")
    with torch.no_grad():
        rets = model(seq, dict(FLAGS))
        model.compute_loss(seq, rets, dict(FLAGS))
        assert not os.path.exists(model.save_folder)          # save_flag off: nothing is written
        model.compute_loss(seq, rets, dict(FLAGS, save_flag=True))
    assert os.listdir(model.save_folder) == ["synthetic_obj_000.pkl"]   # the frames are synthetic_obj_000/0000 ...
    with open(os.path.join(model.save_folder, "synthetic_obj_000.pkl"), "rb") as f:
        saved = pickle.load(f)
    assert saved["CAD_ID"] == "bottle" and len(saved["pred_obj_poses"]) == 4
    assert np.array_equal(saved["pred_obj_poses"][3]["rotation"], rets[3]["rotation"].cpu().numpy())
    surf = rets[0]["obj_surface"]
    assert saved["obj_surface"]["frames"] == 5 and saved["obj_surface"]["fit"].shape == (2,)
    for key in ("points", "normals"):
        assert isinstance(saved["obj_surface"][key], np.ndarray) and np.array_equal(saved["obj_surface"][key], surf[key].cpu().numpy())
    # switch off: no surface, and --save writes nothing for it
    off = _model(False)
    off.save_folder = str(tmp_path / "off")
    with torch.no_grad():
        seq = copy.deepcopy(_sequences(1)[0])
        off.compute_loss(seq, off(seq, dict(FLAGS)), dict(FLAGS, save_flag=True))
    assert not os.path.exists(off.save_folder)
