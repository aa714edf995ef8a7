"""GPU: the mesh -> signed-distance kernels (hotrack_amd/csrc/mesh_sdf.hip) against the float64 oracle and the closed forms of
tests/_mesh_cases.py at its tolerances; the volume entry against the point entry; determinism; degenerate and permuted faces;
the face-index check; and one tracked sequence whose volume the tracker builds from the capsule's mesh."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mesh_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu
FP16_ULP_AT_CLAMP = 2.0 ** -14  # spacing of binary16 in [0.0625, 0.125): the largest ulp of a volume clamped to +-0.1


def _gpu(name):
    v, f = MC.mesh(name)
    return torch.from_numpy(v.copy()).cuda(), torch.from_numpy(f.copy()).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("name", MC.MESHES)
def test_mesh_signed_distance_matches_oracle(name):
    from hotrack_amd import sdf
    v, f = _gpu(name)
    pts = torch.from_numpy(MC.grid()).cuda()
    d, w = sdf.mesh_signed_distance(pts, v, f, return_winding=True)
    d_ref, w_ref = MC.oracle(name)
    MC.check_against_oracle(d.cpu().numpy(), d_ref, w.cpu().numpy(), w_ref, label=f"kernel, {name}")
    assert torch.equal(_bits(d), _bits(sdf.mesh_signed_distance(pts, v, f)))  # with and without the winding output
    if name == "box":
        err = float(np.abs(d.cpu().numpy() - MC.box_sdf(MC.grid())).max())
        print(f"kernel, box vs its closed form: {err:.3e} m")
        assert err <= MC.MAG_TOL


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("res,stride", [(25, 0.0167), (33, 0.0125)])
def test_mesh_sdf_volume_matches_oracle(res, stride, dtype):
    from hotrack_amd import sdf
    v, f = _gpu("torus24")
    vol = sdf.mesh_sdf_volume(v, f, res, stride, 0.1, dtype)
    assert vol.shape == (res, res, res) and vol.dtype == dtype
    d_ref, _ = MC.oracle("torus24", res, stride)
    far = np.abs(d_ref) >= MC.SIGN_MIN
    assert (~far).mean() <= MC.SIGN_SKIP_MAX
    got = vol.cpu().numpy().reshape(-1)
    want = np.clip(d_ref, -0.1, 0.1)
    # the entry takes the clamp as an fp32: no value lies beyond fp32(0.1), which is 1.5e-9 above 0.1 (fp16(0.1) is below it)
    assert np.isfinite(got).all() and float(np.abs(got).max()) <= float(np.float32(0.1))
    assert ((got < 0) == (want < 0))[far].all()
    if dtype == torch.float32:
        err = float(np.abs(np.abs(got.astype(np.float64)) - np.abs(want)).max())
        print(f"volume {res}^3 fp32: max | |d| - |oracle| | = {err:.3e} m")
        assert err <= MC.MAG_TOL
    else:
        want16 = want.astype(np.float16)
        ulps = np.abs(got.view(np.int16).astype(np.int32) - want16.view(np.int16).astype(np.int32))[far]  # equal signs: ordered bits
        print(f"volume {res}^3 fp16: at most {int(ulps.max())} ulp from the rounded oracle")
        assert int(ulps.max()) <= 1
    # the volume entry is the point entry on the generated grid, bit for bit, before clamping and rounding
    pts = torch.from_numpy(MC.grid(res, stride)).cuda()
    d = sdf.mesh_signed_distance(pts, v, f)
    assert torch.equal(_bits(vol.reshape(-1)), _bits(d.clamp(-0.1, 0.1).to(dtype)))
    # and two runs are bitwise equal
    assert torch.equal(_bits(vol), _bits(sdf.mesh_sdf_volume(v, f, res, stride, 0.1, dtype)))


def test_unclamped_volume_equals_point_entry_bitwise():
    from hotrack_amd import sdf
    v, f = _gpu("torus48")
    vol = sdf.mesh_sdf_volume(v, f, 25, 0.0167, 10.0, torch.float32)  # a clamp nothing reaches: the values before rounding
    pts = torch.from_numpy(MC.grid()).cuda()
    d, w = sdf.mesh_signed_distance(pts, v, f, return_winding=True)
    assert torch.equal(_bits(vol.reshape(-1)), _bits(d))
    d2, w2 = sdf.mesh_signed_distance(pts, v, f, return_winding=True)
    assert torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(w), _bits(w2))


def test_degenerate_and_permuted_faces():
    from hotrack_amd import sdf
    v, f = MC.mesh("torus48")
    pts = torch.from_numpy(MC.grid()).cuda()
    d, w = sdf.mesh_signed_distance(pts, *_gpu("torus48"), return_winding=True)
    v2, f2 = MC.with_degenerate_faces(v, f)
    d2, w2 = sdf.mesh_signed_distance(pts, torch.from_numpy(v2).cuda(), torch.from_numpy(f2).cuda(), return_winding=True)
    assert torch.isfinite(d2).all() and torch.isfinite(w2).all()
    # the collinear face splits an edge at a midpoint rounded to fp32: the distance to a half of the edge is the distance to the
    # edge from other operands, so it is held to the geometry bound, the sign exactly
    assert float((d.abs() - d2.abs()).abs().max()) <= MC.MAG_TOL and torch.equal(d < 0, d2 < 0)
    assert float((w - w2).abs().max()) <= 1e-5
    # the repeated-vertex faces are made of edges and vertices the mesh already has: bit for bit the same distances
    d2r, w2r = sdf.mesh_signed_distance(pts, torch.from_numpy(v2).cuda(), torch.from_numpy(f2[:-1].copy()).cuda(), return_winding=True)
    assert torch.equal(_bits(d), _bits(d2r)) and torch.equal(_bits(w), _bits(w2r))
    perm = np.arange(len(f))
    perm[:512] = np.random.default_rng(0).permutation(512)  # within the first LDS chunk
    d3, w3 = sdf.mesh_signed_distance(pts, torch.from_numpy(v.copy()).cuda(), torch.from_numpy(f[perm].copy()).cuda(), return_winding=True)
    assert torch.equal(_bits(d), _bits(d3))
    assert float((w - w3).abs().max()) <= 1e-5
    # degenerate faces alone: distances to segments and points, exactly zero winding, no NaN
    only = torch.from_numpy(f2[len(f):].copy()).cuda()
    d4, w4 = sdf.mesh_signed_distance(pts, torch.from_numpy(v2).cuda(), only, return_winding=True)
    assert torch.isfinite(d4).all() and bool((w4 == 0).all()) and bool((d4 >= 0).all())
    i, j = int(f[0, 0]), int(f[0, 1])
    seg = np.sqrt(MC._segment_dist2(tuple(MC.grid().astype(np.float64)[:, k] for k in range(3)), tuple(v[i].astype(np.float64)),
                                    tuple(v[j].astype(np.float64))))
    assert float(np.abs(d4.cpu().numpy() - seg).max()) <= MC.MAG_TOL


def test_out_of_range_face_index_raises():
    from hotrack_amd import sdf
    v, f = _gpu("box")
    pts = torch.from_numpy(MC.grid()[:300]).cuda()
    for bad in (8, -1, 1 << 30):
        g = f.clone()
        g[5, 2] = bad
        with pytest.raises(ValueError, match="face index"):
            sdf.mesh_signed_distance(pts, v, g)
        with pytest.raises(ValueError, match="face index"):
            sdf.mesh_sdf_volume(v, g, 5, 0.05)
    assert torch.isfinite(sdf.mesh_signed_distance(pts, v, f)).all()  # the flag is reset by the next call


def test_binding_validates_its_arguments():
    from hotrack_amd import sdf
    v, f = _gpu("box")
    pts = torch.zeros(4, 3, device="cuda")
    with pytest.raises(RuntimeError):
        sdf.mesh_signed_distance(pts.cpu(), v, f)
    with pytest.raises(TypeError):
        sdf.mesh_signed_distance(pts, v.double(), f)
    with pytest.raises(TypeError):
        sdf.mesh_signed_distance(pts, v, f.long())
    with pytest.raises(ValueError):
        sdf.mesh_signed_distance(pts, v.t(), f)
    with pytest.raises(ValueError):
        sdf.mesh_signed_distance(pts, v[:, [2, 1, 0]].t().contiguous().t(), f)  # not contiguous
    with pytest.raises(TypeError):
        sdf.mesh_sdf_volume(v, f, 5, 0.05, dtype=torch.bfloat16)
    with pytest.raises(Exception):
        sdf.mesh_sdf_volume(v, f, 4, 0.05)
    assert sdf.mesh_signed_distance(pts[:0], v, f).shape == (0,)


def test_tracker_builds_its_volume_from_the_mesh():
    """One sequence of SyntheticObjectSequences(obj_as_mesh=True) at the dataset's default 201^3: the tracker builds the volume
    from capsule_mesh and meets the thresholds tests/test_track_obj.py applies to the analytic volume; the chamfer columns come
    from points sampled on the mesh; the built volume is the analytic one to within the tessellation's sagitta + 1 fp16 ulp."""
    from datasets.synthetic import SyntheticObjectSequences, _capsule_sdf, capsule_mesh, capsule_volume
    from models import mesh_sdf
    from models.track_network import ObjTrackModel_Optimization
    cfg = {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False},
           "num_points": 1024, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}}
    ds = SyntheticObjectSequences(cfg, 1, 3, obj_as_mesh=True)
    seq = ds[0]
    assert "sdf_volume" not in seq[0] and "obj_mesh" in seq[0]
    del seq[0]["obj_model_points"]  # the chamfer columns must come from the mesh
    model = ObjTrackModel_Optimization(cfg)
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}
    with torch.no_grad():
        rets = model(seq, flags)
        loss, _ = model.compute_loss(seq, rets, flags)
    print({k: round(v, 6) for k, v in loss.items()})
    assert loss["obj_pred_t_diff"] < 5e-3 and loss["obj_pred_axis_diff"] < 3.0
    assert np.isfinite(loss["raw_obj_chamfer(mm)"]) and np.isfinite(loss["pred_obj_chamfer(mm)"])
    assert loss["raw_obj_chamfer(mm)"] == 0.0  # the same sampled cloud on both sides
    vol = model.optimizer.sdf_volume
    assert vol.shape == (201, 201, 201) and vol.dtype == torch.float16
    v, f = capsule_mesh()
    sag = MC.sagitta(v, f, _capsule_sdf)
    diff = float((vol.float().cpu() - torch.from_numpy(capsule_volume()).float()).abs().max())
    print(f"mesh-built volume vs capsule_volume: {diff:.3e} (sagitta {sag:.3e} + fp16 ulp {FP16_ULP_AT_CLAMP:.3e})")
    assert diff <= sag + FP16_ULP_AT_CLAMP
    # a second sequence of the same object does not rebuild
    n = len(mesh_sdf._volumes)
    with torch.no_grad():
        model(ds[0], flags)
    assert len(mesh_sdf._volumes) == n


def test_tracker_without_volume_or_mesh_names_the_keys():
    from datasets.synthetic import SyntheticObjectSequences
    from models.track_network import ObjTrackModel_Optimization
    cfg = {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False},
           "num_points": 64, "obj_category": ["bottle"]}
    seq = SyntheticObjectSequences(cfg, 1, 1, obj_as_mesh=True)[0]
    del seq[0]["obj_mesh"]
    with pytest.raises(RuntimeError, match="obj_mesh_path"):
        ObjTrackModel_Optimization(cfg)(seq, {"track_flag": True, "test_flag": True})
