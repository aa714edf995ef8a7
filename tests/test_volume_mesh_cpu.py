"""CPU: SDF volume -> triangle mesh -- the torch route of network/models/mesh_sdf.volume_to_mesh against the
float64 restatement of tests/_volume_mesh_cases.py (counts and faces exactly, vertices to vertex_tolerance), the mesh checks
on the restatement itself, save_mesh / load_mesh, the argument checks of the C entries, and the --extract_obj_mesh switch."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _volume_mesh_cases as C  # noqa: E402


def _compare(vol, voxel_scale, level, label):
    from models import mesh_sdf
    keys, verts, faces = C.restate(vol, voxel_scale, level)
    tv, tf = mesh_sdf.volume_to_mesh(torch.from_numpy(np.ascontiguousarray(vol)), voxel_scale, level, route="torch")
    assert tv.dtype == torch.float32 and tf.dtype == torch.int32 and tv.shape[1:] == (3,) and tf.shape[1:] == (3,)
    assert tv.shape[0] == len(keys) and tf.shape[0] == len(faces), label
    assert np.array_equal(tf.numpy(), faces), label
    if len(keys):
        err = float(np.abs(tv.numpy() - verts).max())
        assert err <= C.vertex_tolerance(vol.shape[0], voxel_scale), (label, err)
    return keys, verts, faces


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["fp32", "fp16"])
def test_single_cells_all_patterns(dtype):
    """res = 2, all 256 corner patterns: every inside set of every tetrahedron, one and two triangles."""
    seen = set()
    for pattern in range(256):
        vol = C.single_cell(pattern, dtype)
        keys, verts, faces = _compare(vol, 0.01, 0.0, f"pattern {pattern}")
        assert (len(keys) == 0) == (pattern in (0, 255))
        seen.add(len(faces))
    assert min(seen) == 0 and max(seen) >= 8  # (up to two triangles in each of the six tetrahedra)


@pytest.mark.parametrize("name", sorted(C.CLOSED))
def test_closed_cases(name):
    vol, vs, level, chi = C.CLOSED[name]
    for dtype in (np.float32, np.float16):
        keys, verts, faces = _compare(vol.astype(dtype), vs, level, name)
        assert len(C.unpaired_edges(faces)) == 0
        assert C.signed_volume(verts, faces) > 0
        if chi is not None:
            assert C.euler_characteristic(len(keys), faces) == chi


def test_octahedron_has_coincident_vertices_and_stays_closed():
    vol, vs, level, _ = C.CLOSED["octahedron9"]
    assert (vol == 0).sum() > 0
    keys, verts, faces = C.restate(vol, vs, level)
    assert len(np.unique(np.round(verts / vs * 1024), axis=0)) < len(verts)
    area = np.linalg.norm(np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]), axis=1)
    assert (area == 0).any() and len(C.unpaired_edges(faces)) == 0
    # the octahedron |x|+|y|+|z| <= 3 voxels is reproduced exactly by linear interpolation: volume (4/3) 27 voxel^3
    assert C.signed_volume(verts, faces) == pytest.approx(36 * float(np.float32(vs)) ** 3, rel=1e-12)


def test_open_surface_is_unpaired_only_on_the_box():
    vol, vs, level = C.OPEN["open9"]
    keys, verts, faces = _compare(vol.astype(np.float32), vs, level, "open9")
    bad = C.unpaired_edges(faces)
    assert len(bad) > 0 and C.on_box_face(keys[np.unique(bad)], vol.shape[0]).all()


def test_no_surface_and_refusals():
    from models import mesh_sdf
    for fill in (-1.0, 1.0):
        v, f = mesh_sdf.volume_to_mesh(torch.full((5, 5, 5), fill), 0.01, route="torch")
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32
    with pytest.raises(ValueError, match="res,res,res"):
        mesh_sdf.volume_to_mesh(torch.zeros((1, 1, 1)), 0.01, route="torch")
    with pytest.raises(ValueError, match="res,res,res"):
        mesh_sdf.volume_to_mesh(torch.zeros((4, 4, 5)), 0.01, route="torch")
    with pytest.raises(ValueError, match="voxel_scale"):
        mesh_sdf.volume_to_mesh(torch.zeros((4, 4, 4)), 0.0, route="torch")
    with pytest.raises(RuntimeError, match="kernel route needs"):
        mesh_sdf.volume_to_mesh(torch.zeros((4, 4, 4)), 0.01, route="kernel")


def test_restatement_meets_the_capsule_surface_bound():
    """The derivation of capsule_surface_bound, checked on the float64 restatement alone (101^3; the 201^3 volume is checked next
    to the kernel, tests/test_gpu_volume_mesh.py)."""
    from datasets.synthetic import capsule_volume
    keys, verts, faces = C.restate(capsule_volume(101, 0.004), 0.004)
    worst, bound = float(np.abs(C.capsule_sdf(verts)).max()), C.capsule_surface_bound(0.004)
    print(f"101^3 capsule, restatement: max |sdf(vertex)| {worst:.3e} m, bound {bound:.3e} m")
    assert worst <= bound
    assert len(C.unpaired_edges(faces)) == 0 and C.euler_characteristic(len(keys), faces) == 2


def test_save_mesh_round_trip(tmp_path):
    from models import mesh_sdf
    vol, vs, level, _ = C.CLOSED["sphere9"]
    v, f = mesh_sdf.volume_to_mesh(torch.from_numpy(vol), vs, level, route="torch")
    ply, obj = tmp_path / "m.ply", tmp_path / "m.obj"
    mesh_sdf.save_mesh(ply, v, f)
    mesh_sdf.save_mesh(obj, v, f)
    assert open(ply, "rb").read(32).startswith(b"ply\nformat binary_little_endian")
    lv, lf = mesh_sdf.load_mesh(ply)
    assert lv.dtype == np.float32 and lf.dtype == np.int32
    assert np.array_equal(lv.view(np.int32), v.numpy().view(np.int32)) and np.array_equal(lf, f.numpy())
    ov, of = mesh_sdf.load_mesh(obj)
    assert np.array_equal(ov, v.numpy()) and np.array_equal(of, f.numpy())  # (%.9g prints an fp32 exactly)


def test_c_entries_refuse_bad_arguments(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    ci, cl, cf, vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    lib.pn2s_volume_mesh_work_bytes.argtypes, lib.pn2s_volume_mesh_work_bytes.restype = [ci], cl
    lib.pn2s_volume_mesh_count.argtypes, lib.pn2s_volume_mesh_count.restype = [vp, ci, ci, cf, cf, vp, cl, vp], ci
    lib.pn2s_volume_mesh_emit.argtypes, lib.pn2s_volume_mesh_emit.restype = [vp, ci, ci, cf, cf, vp, cl, ci, ci, vp, vp, vp], ci
    EINVAL, ENULL, ERANGE, ESCRATCH = -1, -2, -3, -4
    assert lib.pn2s_volume_mesh_work_bytes(1) == EINVAL and lib.pn2s_volume_mesh_work_bytes(513) == ERANGE
    need = lib.pn2s_volume_mesh_work_bytes(201)
    assert 5 * 201 ** 3 <= need <= 5 * 201 ** 3 + 8 * (201 ** 3 // 256 + 1) + 64  # an int32 and a byte per voxel, 8 bytes per workgroup
    p = 4096  # never dereferenced: every call below is refused before a launch
    count = lambda vol=p, f16=1, res=9, s=0.01, lv=0.0, work=p, nbytes=1 << 20: lib.pn2s_volume_mesh_count(vol, f16, res, s, lv, work, nbytes, None)
    assert count(res=1) == EINVAL and count(f16=2) == EINVAL and count(s=0.0) == EINVAL and count(s=-1.0) == EINVAL
    assert count(s=float("inf")) == EINVAL and count(s=float("nan")) == EINVAL and count(lv=float("nan")) == EINVAL
    assert count(vol=None) == ENULL and count(work=None) == ENULL
    assert count(res=513, nbytes=1 << 40) == ERANGE
    assert count(nbytes=lib.pn2s_volume_mesh_work_bytes(9) - 1) == ESCRATCH
    assert count(work=p + 4) == EINVAL
    emit = lambda nv=1, nf=1, verts=p, faces=p, **kw: lib.pn2s_volume_mesh_emit(
        kw.get("vol", p), 1, kw.get("res", 9), kw.get("s", 0.01), 0.0, p, kw.get("nbytes", 1 << 20), nv, nf, verts, faces, None)
    assert emit(res=1) == EINVAL and emit(s=0.0) == EINVAL and emit(nv=-1) == EINVAL and emit(nbytes=16) == ESCRATCH
    assert emit(verts=None) == ENULL and emit(faces=None) == ENULL and emit(vol=None) == ENULL
    assert emit(nv=0, nf=0, verts=None, faces=None) == 0  # nothing to write: a no-op


# ---- the --extract_obj_mesh switch -----------------------------------------------------------------------------------------------
def test_config_default_and_flag(tmp_path, monkeypatch):
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    from configs.config import get_config
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    assert get_config(p.parse_args(["--config", "objopt_test_HO3D.yml"]), save=False)["opt"]["extract_mesh"] is False
    assert get_config(p.parse_args(["--config", "objopt_test_HO3D.yml", "--extract_obj_mesh"]), save=False)["opt"]["extract_mesh"] is True


def _tracker(save_folder=None):
    """ObjTrackModel_Optimization without its optimiser (the end-of-sequence entry and compute_loss do not use it): CPU tensors,
    the torch route."""
    from models.track_network import ObjTrackModel_Optimization
    m = ObjTrackModel_Optimization.__new__(ObjTrackModel_Optimization)
    torch.nn.Module.__init__(m)
    m.device, m.sym, m.extract_mesh, m.extract_mesh_route, m.save_folder = torch.device("cpu"), -1, True, "torch", save_folder
    return m


def _sequence():
    """A two-frame synthetic sequence that carries only its volume, 'tracked' perfectly."""
    from datasets.synthetic import SyntheticObjectSequences
    seq = SyntheticObjectSequences({"num_points": 64, "obj_category": ["bottle"]}, 1, 2, res=41, stride=0.01)[0]
    del seq[0]["obj_model_points"]
    rets = [{"rotation": d["gt_obj_pose"]["rotation"].reshape(1, 3, 3).clone(), "translation": d["gt_obj_pose"]["translation"].reshape(1, 3, 1).clone()}
            for d in seq]
    return seq, rets


def test_extract_obj_mesh_entry_reports_chamfer_and_writes_the_ply(tmp_path):
    from models import mesh_sdf
    from models.track_network import ObjTrackModel_Optimization
    ObjTrackModel_Optimization._said_no_points = True
    seq, rets = _sequence()
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    before, _ = _tracker().compute_loss(seq, rets, flags)           # the switch off: no obj_info, as before this feature
    assert "raw_obj_chamfer(mm)" not in before and all(set(r) == {"rotation", "translation"} for r in rets)

    m = _tracker(str(tmp_path))
    m._attach_mesh(seq, rets, seq[0]["sdf_volume"], seq[0]["voxel_scale"], flags)
    info = rets[0]["obj_info"]
    assert info["recon_path"] is None and not os.listdir(tmp_path)  # no --save: nothing is written
    keys, verts, faces = C.restate(seq[0]["sdf_volume"].numpy(), seq[0]["voxel_scale"])
    assert np.array_equal(info["recon_mesh"]["faces"].numpy(), faces)
    after, _ = m.compute_loss(seq, rets, flags)
    assert list(after) == [*before, "raw_obj_chamfer(mm)", "pred_obj_chamfer(mm)"] and all(after[k] == before[k] for k in before)
    assert after["raw_obj_chamfer(mm)"] == 0.0 and 0.0 <= after["pred_obj_chamfer(mm)"] < 1e-3  # the poses are the true ones

    flags["save_flag"] = True
    shared = {}
    m._attach_mesh(seq, rets, seq[0]["sdf_volume"], seq[0]["voxel_scale"], flags, shared)
    path = rets[0]["obj_info"]["recon_path"]
    assert path == os.path.join(str(tmp_path), "synthetic_obj_000_recon.ply") and os.path.isfile(path)
    lv, lf = mesh_sdf.load_mesh(path)
    assert np.array_equal(lf, faces) and np.array_equal(lv, info["recon_mesh"]["vertices"].numpy())
    # a second sequence of the group with the same volume takes the mesh already extracted
    seq2, rets2 = _sequence()
    seq2[0]["sdf_volume"] = seq[0]["sdf_volume"]
    m._attach_mesh(seq2, rets2, seq2[0]["sdf_volume"], seq2[0]["voxel_scale"], {**flags, "save_flag": False}, shared)
    assert rets2[0]["obj_info"]["recon_mesh"] is rets[0]["obj_info"]["recon_mesh"] and len(shared) == 1


def test_model_points_and_a_mesh_still_come_first():
    """With obj_model_points in the first frame the extracted mesh is not sampled: the columns are what they were."""
    from models.track_network import ObjTrackModel_Optimization
    ObjTrackModel_Optimization._said_no_points = True
    from datasets.synthetic import model_points
    seq, rets = _sequence()
    seq[0]["obj_model_points"] = model_points(70_000)
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    want, _ = _tracker().compute_loss(seq, rets, flags)
    m = _tracker()
    m._attach_mesh(seq, rets, seq[0]["sdf_volume"], seq[0]["voxel_scale"], flags)
    got, _ = m.compute_loss(seq, rets, flags)
    assert got == want


def test_sdf2mesh_is_the_reference_name():
    from models.optimization_obj import gf_optimize_obj
    assert callable(gf_optimize_obj.sdf2mesh)
