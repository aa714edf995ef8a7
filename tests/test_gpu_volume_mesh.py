"""GPU: SDF volume -> triangle mesh (hotrack_amd/csrc/sdf_mesh.hip, hotrack_amd.sdf.volume_mesh) against the float64 restatement
of tests/_volume_mesh_cases.py: vertex count, face count and the face index array exactly, vertices to vertex_tolerance; closed
cases closed and positively oriented; the capsule volumes against the capsule's float64 distance, its analytic volume and a
mesh -> volume round trip; and object tracking with opt.extract_mesh on.  Tolerances are derived in _volume_mesh_cases.py."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _volume_mesh_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _extract(vol, voxel_scale, level=0.0):
    from hotrack_amd import sdf
    v, f = sdf.volume_mesh(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), voxel_scale, level)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    return v.cpu().numpy(), f.cpu().numpy()


def _compare(vol, voxel_scale, level, label, want=None):
    keys, verts, faces = C.restate(vol, voxel_scale, level) if want is None else want
    v, f = _extract(vol, voxel_scale, level)
    assert len(v) == len(keys) and len(f) == len(faces), (label, len(v), len(keys), len(f), len(faces))
    assert np.array_equal(f, faces), label
    if len(keys):
        err = float(np.abs(v - verts).max())
        assert err <= C.vertex_tolerance(vol.shape[0], voxel_scale), (label, err)
    return v, f


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
def test_single_cells_all_patterns(dtype):
    for pattern in range(256):
        _compare(C.single_cell(pattern, dtype), 0.01, 0.0, f"pattern {pattern}")


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", sorted(C.CLOSED))
def test_closed_cases(name, dtype):
    vol, vs, level, chi = C.CLOSED[name]
    v, f = _compare(vol.astype(dtype), vs, level, name)
    assert len(C.unpaired_edges(f)) == 0
    assert C.signed_volume(v, f) > 0
    if chi is not None:
        assert C.euler_characteristic(len(v), f) == chi


def test_open_surface_is_unpaired_only_on_the_box():
    vol, vs, level = C.OPEN["open9"]
    vol = vol.astype(np.float32)
    keys = C.restate(vol, vs, level)[0]
    v, f = _compare(vol, vs, level, "open9")
    bad = C.unpaired_edges(f)
    assert len(bad) > 0 and C.on_box_face(keys[np.unique(bad)], vol.shape[0]).all()


def test_no_surface_returns_empty_outputs():
    for fill in (-1.0, 1.0):
        for dtype in (np.float32, np.float16):
            v, f = _extract(np.full((7, 7, 7), fill, dtype=dtype), 0.01)
            assert v.shape == (0, 3) and f.shape == (0, 3)


def test_two_runs_are_bitwise_equal_and_the_volume_is_untouched():
    vol, vs, level, _ = C.CLOSED["torus33"]
    a = _extract(vol.astype(np.float16), vs, level)
    b = _extract(vol.astype(np.float16), vs, level)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def test_refusals():
    from hotrack_amd import sdf
    good = torch.zeros((5, 5, 5), device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        sdf.volume_mesh(torch.zeros((5, 5, 10), device="cuda")[:, :, ::2], 0.01)
    with pytest.raises(RuntimeError, match="GPU"):
        sdf.volume_mesh(torch.zeros((5, 5, 5)), 0.01)
    with pytest.raises(ValueError, match=r"\[2, 512\]"):
        sdf.volume_mesh(torch.zeros((1, 1, 1), device="cuda"), 0.01)
    with pytest.raises(TypeError, match="float16 or float32"):
        sdf.volume_mesh(good.double(), 0.01)
    with pytest.raises(ValueError, match="res,res,res"):
        sdf.volume_mesh(torch.zeros((125,), device="cuda"), 0.01)
    for bad in (0.0, -0.01, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="voxel_scale"):
            sdf.volume_mesh(good, bad)
    with pytest.raises(ValueError, match="level"):
        sdf.volume_mesh(good, 0.01, float("nan"))
    assert sdf.volume_mesh_work_bytes(201) >= 5 * 201 ** 3
    with pytest.raises(ValueError):
        sdf.volume_mesh_work_bytes(513)


# ---- the capsule the synthetic sequences track ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _capsule(res, voxel_scale):
    """(volume fp16, restatement, kernel output) of the capsule volume, computed once."""
    from datasets.synthetic import capsule_volume
    vol = capsule_volume(res, voxel_scale)
    want = C.restate(vol, voxel_scale)
    return vol, want, _compare(vol, voxel_scale, 0.0, f"capsule {res}", want)


@pytest.mark.parametrize("res,voxel_scale", [(101, 0.004), (201, 0.002)])
def test_capsule_vertices_lie_on_the_capsule(res, voxel_scale):
    vol, (keys, verts, faces), (v, f) = _capsule(res, voxel_scale)
    bound = C.capsule_surface_bound(voxel_scale)
    ref_worst, worst = float(np.abs(C.capsule_sdf(verts)).max()), float(np.abs(C.capsule_sdf(v)).max())
    print(f"capsule {res}^3: {len(v)} vertices, {len(f)} triangles; max |sdf(vertex)| restatement {ref_worst:.3e} m, kernel {worst:.3e} m, bound {bound:.3e} m")
    assert ref_worst <= bound  # the derivation holds for the restatement alone
    assert worst <= bound
    assert len(C.unpaired_edges(f)) == 0 and C.euler_characteristic(len(v), f) == 2


def test_capsule_signed_volume():
    _, (keys, verts, faces), (v, f) = _capsule(201, 0.002)
    got, ref = C.signed_volume(v, f), C.signed_volume(verts, faces)
    analytic = np.pi * 0.04 ** 2 * 0.14 + 4.0 / 3.0 * np.pi * 0.04 ** 3
    print(f"capsule 201^3: signed volume kernel {got:.9e}, restatement {ref:.9e}, analytic {analytic:.9e} m^3 "
          f"(relative {got / analytic - 1:+.3e} and {got / ref - 1:+.3e})")
    assert abs(got / analytic - 1) <= 5e-3
    assert abs(got / ref - 1) <= 1e-5


def test_round_trip_through_the_mesh_distance():
    """mesh -> volume of volume -> mesh against the volume, on the voxels within two voxels of the surface.  Those voxels go
    through the point entry, whose value is bit for bit what the volume entry clamps and rounds at the same centre
    (include/pn2_sdf.h; tests/test_gpu_mesh_sdf.py holds the two to that): the volume entry would spend its time on the other
    99 % of the voxels.  Bound: one voxel; expected: the on-surface error plus the fp16 step."""
    from hotrack_amd import sdf
    res, vs = 101, 0.004
    vol, _, (v, f) = _capsule(res, vs)
    near = np.abs(vol.astype(np.float32)) < 2 * vs
    pts = C.grid(res, vs)[near].astype(np.float32)
    d = sdf.mesh_signed_distance(torch.from_numpy(pts).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda())
    back = d.clamp(-0.1, 0.1).to(torch.float16).float().cpu().numpy()
    diff = float(np.abs(back - vol[near].astype(np.float32)).max())
    print(f"round trip, 101^3 capsule, {int(near.sum())} voxels within two voxels of the surface: max difference {diff:.3e} m "
          f"(one voxel {vs:.1e} m; on-surface bound + fp16 step {C.capsule_surface_bound(vs) + 2.0 ** -17:.3e} m)")
    assert diff <= vs


# ---- tracking with opt.extract_mesh ------------------------------------------------------------------------------------------
RES, STRIDE, N = 41, 0.01, 256
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


def _cfg(on, save_dir=None):
    return {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False, "extract_mesh": on},
            "num_points": N, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "save_dir": save_dir}


def _sequences(count, frames=4):
    from datasets.synthetic import SyntheticObjectSequences
    data = SyntheticObjectSequences(_cfg(False), count, frames, res=RES, stride=STRIDE)
    seqs = [copy.deepcopy(data[s]) for s in range(count)]
    for seq in seqs:
        del seq[0]["obj_model_points"]  # only the volume: the chamfer columns need the extracted mesh
        seq[0]["sdf_volume"] = seqs[0][0]["sdf_volume"]
    return seqs


def _model(on, save_dir=None):
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    model = ObjTrackModel_Optimization(_cfg(on, save_dir))
    model.optimizer = gf_optimize_obj(_cfg(on), seed=7)
    model.optimizer.volume_size = RES
    return model


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def test_tracking_with_the_switch_on(tmp_path):
    from models import mesh_sdf
    from models.track_network import ObjTrackModel_Optimization
    ObjTrackModel_Optimization._said_no_points = True
    out = {}
    with torch.no_grad():
        for on in (False, True):
            seq = _sequences(1)[0]
            model = _model(on, str(tmp_path))
            flags = dict(FLAGS, save_flag=on)
            rets = model(seq, flags)
            out[on] = (rets, model.compute_loss(seq, rets, dict(FLAGS))[0], model)
    (off, loss_off, _), (on, loss_on, model) = out[False], out[True]
    assert len(off) == len(on) == 4
    for a, b in zip(off, on):
        assert np.array_equal(_bits(a["rotation"]), _bits(b["rotation"])) and np.array_equal(_bits(a["translation"]), _bits(b["translation"]))
    assert "obj_info" not in off[0] and "raw_obj_chamfer(mm)" not in loss_off
    assert list(loss_on) == [*loss_off, "raw_obj_chamfer(mm)", "pred_obj_chamfer(mm)"]
    assert all(float(loss_on[k]) == float(loss_off[k]) for k in loss_off)
    assert loss_on["raw_obj_chamfer(mm)"] == 0.0 and np.isfinite(loss_on["pred_obj_chamfer(mm)"]) and 0 <= loss_on["pred_obj_chamfer(mm)"] < 30
    info = on[0]["obj_info"]
    vol = model.optimizer.sdf_volume
    keys, verts, faces = C.restate(vol.cpu().numpy(), STRIDE)
    assert info["recon_mesh"]["vertices"].is_cuda and np.array_equal(info["recon_mesh"]["faces"].cpu().numpy(), faces)
    assert info["recon_path"] == os.path.join(str(tmp_path), "synthetic_obj_000_recon.ply")
    lv, lf = mesh_sdf.load_mesh(info["recon_path"])
    assert np.array_equal(lf, faces) and np.array_equal(lv, info["recon_mesh"]["vertices"].cpu().numpy())
    # the reference's name, on the optimiser
    sv, sf = model.optimizer.sdf2mesh(str(tmp_path / "again.ply"))
    assert torch.equal(sv, info["recon_mesh"]["vertices"]) and torch.equal(sf, info["recon_mesh"]["faces"])
    assert open(tmp_path / "again.ply", "rb").read() == open(info["recon_path"], "rb").read()


def test_a_group_in_lockstep_shares_one_extraction(monkeypatch):
    from models import mesh_sdf
    calls = []
    real = mesh_sdf.volume_to_mesh
    monkeypatch.setattr(mesh_sdf, "volume_to_mesh", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        single = [_model(True)(seq, dict(FLAGS)) for seq in _sequences(2)]
        n_single = len(calls)
        group = _model(True).forward_batch(_sequences(2), dict(FLAGS))
    assert n_single == 2 and len(calls) == 3  # one per sequence alone; one for the group's shared volume
    assert group[0][0]["obj_info"]["recon_mesh"] is group[1][0]["obj_info"]["recon_mesh"]
    for a, b in zip(single, group):
        assert torch.equal(a[0]["obj_info"]["recon_mesh"]["faces"], b[0]["obj_info"]["recon_mesh"]["faces"])
        assert torch.equal(a[0]["obj_info"]["recon_mesh"]["vertices"], b[0]["obj_info"]["recon_mesh"]["vertices"])
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x["rotation"]), _bits(y["rotation"])) and np.array_equal(_bits(x["translation"]), _bits(y["translation"]))
