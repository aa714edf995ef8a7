"""CPU: the mesh -> signed-distance path without a GPU -- the float64 oracle against the box's closed form, the torch route
(network/models/mesh_sdf.py) against the oracle at the tolerances of tests/_mesh_cases.py, the mesh readers, surface sampling,
degenerate faces, and a small volume on the CPU."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mesh_cases as MC  # noqa: E402
from models import mesh_sdf  # noqa: E402


def _t(name):
    v, f = MC.mesh(name)
    return torch.from_numpy(v.copy()), torch.from_numpy(f.copy())


def test_oracle_equals_the_box_closed_form():
    d, w = MC.oracle("box")
    err = float(np.abs(d - MC.box_sdf(MC.grid())).max())
    print(f"float64 oracle vs the box closed form: {err:.3e}")
    assert err <= 1e-12
    assert np.abs(w - (d < 0)).max() <= 1e-9  # a closed, outward-oriented mesh: 0 outside, 1 inside


def test_oracle_is_within_the_sagitta_of_the_torus():
    for name in ("torus24", "torus48"):
        v, f = MC.mesh(name)
        sag = MC.sagitta(v, f, MC.torus_sdf)
        err = float(np.abs(MC.oracle(name)[0] - MC.torus_sdf(MC.grid())).max())
        print(f"{name}: sagitta {sag:.3e} m, oracle vs analytic torus {err:.3e} m")
        assert err <= sag


@pytest.mark.parametrize("name", MC.MESHES)
def test_torch_route_matches_oracle(name):
    v, f = _t(name)
    d, w = mesh_sdf.signed_distance_torch(torch.from_numpy(MC.grid()), v, f, return_winding=True)
    d_ref, w_ref = MC.oracle(name)
    MC.check_against_oracle(d.numpy(), d_ref, w.numpy(), w_ref, label=f"torch route, {name}")
    if name == "box":
        assert float(np.abs(d.numpy() - MC.box_sdf(MC.grid())).max()) <= MC.MAG_TOL


def test_degenerate_faces_change_nothing_torch():
    v, f = MC.mesh("box")
    v2, f2 = MC.with_degenerate_faces(v, f)
    pts = torch.from_numpy(MC.grid())
    d, w = mesh_sdf.signed_distance_torch(pts, torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), return_winding=True)
    d2, w2 = mesh_sdf.signed_distance_torch(pts, torch.from_numpy(v2), torch.from_numpy(f2), return_winding=True)
    assert torch.isfinite(d2).all() and torch.isfinite(w2).all()
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32))
    assert float((w - w2).abs().max()) <= 1e-5  # (zeros are added, but torch's row sums change their association with the length)
    # a mesh of degenerate faces only: distances to its segments and points, no solid angle, no NaN
    only = torch.from_numpy(f2[len(f):])
    d3, w3 = mesh_sdf.signed_distance_torch(pts, torch.from_numpy(v2), only, return_winding=True)
    assert torch.isfinite(d3).all() and bool((w3 == 0).all()) and bool((d3 >= 0).all())


def test_out_of_range_face_index_raises_torch():
    v, f = _t("box")
    f[3, 1] = 8
    with pytest.raises(ValueError, match="face index"):
        mesh_sdf.signed_distance_torch(torch.zeros(4, 3), v, f)


def test_mesh_to_volume_cpu_matches_oracle_in_fp16():
    v, f = _t("torus24")
    vol = mesh_sdf.mesh_to_volume(v, f, 25, 0.0167, clamp=0.1, dtype=torch.float16)
    assert vol.shape == (25, 25, 25) and vol.dtype == torch.float16
    d_ref, _ = MC.oracle("torus24")
    want = np.clip(d_ref, -0.1, 0.1).astype(np.float16).reshape(25, 25, 25)
    far = (np.abs(d_ref) >= MC.SIGN_MIN).reshape(25, 25, 25)
    ulps = np.abs(vol.numpy().view(np.int16).astype(np.int32) - want.view(np.int16).astype(np.int32))  # same sign: ordered bits
    assert ((vol.numpy() < 0) == (want < 0))[far].all()
    assert int(ulps[far].max()) <= 1
    assert (~far).mean() <= MC.SIGN_SKIP_MAX
    with pytest.raises(ValueError):
        mesh_sdf.mesh_to_volume(v, f, 24, 0.0167)


def test_open_mesh_warns(capsys):
    v, f = _t("box")
    mesh_sdf.mesh_to_volume(v * 8.0, f, 5, 0.05)  # the box reaches past the +-0.1 m volume: the corner voxel is inside it
    assert "WARNING: winding number" in capsys.readouterr().out


# ---- files ------------------------------------------------------------------------------------------------------------------
def _quad_box():
    v, _ = MC.mesh("box")
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, quads


def test_load_mesh_obj_with_slashes_negative_indices_and_quads(tmp_path):
    v, quads = _quad_box()
    lines = ["# a box", "o box"] + [f"v {x!r} {y!r} {z!r}" for x, y, z in v.astype(np.float64).tolist()] + ["vn 0 0 1", "vt 0 0"]
    forms = [lambda i: f"{i + 1}", lambda i: f"{i + 1}/1", lambda i: f"{i + 1}//1", lambda i: f"{i + 1}/1/1", lambda i: f"{i - 8}",
             lambda i: f"{i - 8}/1/1"]
    lines += ["f " + " ".join(form(i) for i in q) for q, form in zip(quads, forms)]
    path = tmp_path / "box.obj"
    path.write_text("\n".join(lines) + "\n")
    lv, lf = mesh_sdf.load_mesh(path)
    ref_v, ref_f = MC.mesh("box")
    assert lv.dtype == np.float32 and lf.dtype == np.int32
    assert np.array_equal(lv, ref_v) and np.array_equal(lf, ref_f)  # fan triangulation == box_mesh's split


@pytest.mark.parametrize("binary", [False, True])
def test_load_mesh_ply(tmp_path, binary):
    v, quads = _quad_box()
    header = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment a box", f"element vertex {len(v)}",
              "property float x", "property float y", "property float z", "property uchar red", "property double quality",
              f"element face {len(quads)}", "property list uchar int vertex_indices", "property float area", "end_header"]
    path = tmp_path / "box.ply"
    if binary:
        body = b"".join(struct.pack("<fffBd", *row, 7, 0.5) for row in v.tolist())
        body += b"".join(struct.pack("<B4if", 4, *q, 1.0) for q in quads)
        path.write_bytes(("\n".join(header) + "\n").encode() + body)
    else:
        rows = [f"{x!r} {y!r} {z!r} 7 0.5" for x, y, z in v.astype(np.float64).tolist()] + ["4 " + " ".join(map(str, q)) + " 1.0" for q in quads]
        path.write_text("\n".join(header + rows) + "\n")
    lv, lf = mesh_sdf.load_mesh(path)
    ref_v, ref_f = MC.mesh("box")
    assert np.array_equal(lv, ref_v) and np.array_equal(lf, ref_f)


def test_load_mesh_rejects_bad_indices(tmp_path):
    path = tmp_path / "bad.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="face index"):
        mesh_sdf.load_mesh(path)


# ---- surface samples ----------------------------------------------------------------------------------------------------------
def test_sample_surface():
    v, f = MC.mesh("box")
    a = mesh_sdf.sample_surface(v, f, 4096, seed=3)
    assert a.shape == (4096, 3) and a.dtype == torch.float32
    assert torch.equal(a, mesh_sdf.sample_surface(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), 4096, seed=3))
    assert not torch.equal(a, mesh_sdf.sample_surface(v, f, 4096, seed=4))
    d, _ = MC.oracle_uncached(a.numpy(), v, f)
    assert float(np.abs(d).max()) <= 1e-6
    # per-face counts against the areas: binomial, 5 standard deviations (a 12-face box: 6e-6 chance of a false alarm overall)
    vv = v.astype(np.float64)
    tri = vv[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=-1)
    p = area / area.sum()
    # the face a sample lies on: the one whose plane and bounding box contain it (ties on shared edges have measure zero)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    q = a.numpy().astype(np.float64)
    on_plane = np.abs(((q[:, None] - tri[None, :, 0]) * n[None]).sum(-1)) < 1e-6                        # (S,F)
    bary_ok = np.zeros_like(on_plane)
    for k in range(len(f)):
        T = np.stack([tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]], 1)                                  # (3,2)
        uv = np.linalg.lstsq(T, (q - tri[k, 0]).T, rcond=None)[0].T
        bary_ok[:, k] = (uv[:, 0] >= 0) & (uv[:, 1] >= 0) & (uv.sum(-1) <= 1)
    owner = (on_plane & bary_ok)
    assert (owner.sum(1) >= 1).all()
    counts = np.bincount(owner.argmax(1), minlength=len(f))
    sd = np.sqrt(4096 * p * (1 - p))
    assert (np.abs(counts - 4096 * p) <= 5 * sd + 1).all(), (counts, 4096 * p)


# ---- synthetic data -------------------------------------------------------------------------------------------------------------
def test_capsule_mesh_is_closed_outward_and_inscribed():
    from datasets.synthetic import _capsule_sdf, capsule_mesh
    v, f = capsule_mesh()
    assert v.dtype == np.float32 and f.dtype == np.int32 and f.shape == (4096, 3)
    assert float(np.abs(_capsule_sdf(v.astype(np.float64))).max()) < 1e-8  # vertices on the surface (fp32 rounding)
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = {(int(a), int(b)) for a, b in edges}
    assert len(fwd) == len(edges) and all((b, a) in fwd for a, b in fwd)  # every edge once in each direction: closed, consistent
    tri = v.astype(np.float64)[f]
    vol = (tri[:, 0] * np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0
    exact = np.pi * 0.04 ** 2 * 0.14 + 4.0 / 3.0 * np.pi * 0.04 ** 3
    assert 0.99 * exact < vol < exact  # outward (positive volume), inscribed (smaller)
    v2, f2 = capsule_mesh(8, 3)
    assert f2.shape == (2 * 8 * 2 * 3, 3)


def test_obj_as_mesh_moves_no_other_draw():
    from datasets.synthetic import SyntheticObjectSequences
    cfg = {"num_points": 64, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}}
    a = SyntheticObjectSequences(cfg, 1, 2, res=21, stride=0.02)[0]
    b = SyntheticObjectSequences(cfg, 1, 2, res=21, stride=0.02, obj_as_mesh=True)[0]
    assert "sdf_volume" in a[0] and "obj_mesh" not in a[0] and "obj_mesh" in b[0] and "sdf_volume" not in b[0]
    assert b[0]["obj_mesh"]["vertices"].dtype == torch.float32 and b[0]["obj_mesh"]["faces"].dtype == torch.int32
    for fa, fb in zip(a, b):
        assert torch.equal(fa["obj_points"], fb["obj_points"])
        assert torch.equal(fa["gt_obj_pose"]["rotation"], fb["gt_obj_pose"]["rotation"])
    assert torch.equal(a[0]["jittered_obj_pose"]["rotation"], b[0]["jittered_obj_pose"]["rotation"])
    assert torch.equal(a[0]["obj_model_points"], b[0]["obj_model_points"]) and a[0]["voxel_scale"] == b[0]["voxel_scale"]
