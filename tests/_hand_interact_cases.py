"""Seeded scenes and the plain reference of the hand-object interaction columns (eval_metrics.hand_interaction_metrics,
pn2x_hand_interaction_metrics), shared by tests/test_hand_interaction.py (CPU) and tests/test_gpu_hand_interaction.py.

A scene is S = 3 packed sequences with an EMPTY middle one, every live sequence with a sphere volume of its own:
  sequence 0 (a sphere of 4 cm)   frame 0: the sphere 12 cm off the hand (no vertex inside); frame 1: the sphere on the tip of
                                  finger 0's region (the whole region inside, the hand penetrates); frame 2: the sphere 30 cm away
                                  along the object's x axis, so that vertices lie outside the volume (clamped index); frame 3:
                                  grazing the palm;
  sequence 2 (a sphere of 20 cm)  frame 0: the sphere on the hand's centroid (every vertex inside); frame 1: 40 cm away (outside).
A shaped model's frames alternate between two shape codes (rest_of) inside each sequence."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from models.hand_model import SyntheticLBSHand, SyntheticManoHand, lbs_forward_from_tables, rodrigues  # noqa: E402

LENGTHS = (4, 0, 2)
RADII = (0.04, None, 0.20)
U = 2.0 ** -24  # fp32 unit roundoff (half an ulp, relative)
# Column 4: t_i = max(min sdf, 0) are exact fp32 values >= 0; a serial sum of n <= 5 of them takes n - 1 roundings of at most U
# of the partial sum (<= the total), the division one more (allowed a whole ulp = 2 U): (4 + 2) U of the value.
COL4_REL = 6 * U
# Column 6: a term sqrt(dx^2 + dy^2 + dz^2): each difference U, so each square 2 U + U, the two additions U each on non-negative
# partial sums: the radicand within 5 U; the root halves that and rounds (a whole ulp allowed): 4.5 U.  The 21 terms are summed by
# a butterfly of depth 6 (6 U on non-negative sums), the division by 21 a whole ulp: 4.5 + 6 + 2 = 12.5, stated as 13 U.
COL6_REL = 13 * U
MM = (0, 4, 5)


def hand_tables(kind, V, K, empty_finger=None):
    """(skinning tables, model or None).  kind 'plain': SyntheticLBSHand(num_verts=V) at K weights (tests/_hand_pose_cases: no
    shape space); 'shaped': the same hand with 10 shape dimensions (K = 2); 'mano': SyntheticManoHand (shape tables, pose blend
    shapes, centre_root, kp_vertex).  empty_finger: that finger's tip region is emptied."""
    if kind == "plain":
        import _hand_pose_cases as C
        model, t = None, dict(C.skinning_tables_for(V, K))
    elif kind == "shaped":
        assert K == 2
        model = SyntheticLBSHand(num_verts=V, num_betas=10)
        t = dict(model.skinning_tables())
    else:
        model = SyntheticManoHand(num_verts=V, weights_per_vertex=K)
        t = dict(model.skinning_tables())
        assert t["skin_idx"].shape[1] == K and t["centre_root"] and (t["kp_vertex"] >= 0).sum() == 5
    if empty_finger is not None:
        offs = [int(o) for o in t["finger_offsets"]]
        keep = [t["tips"][offs[i]:offs[i + 1]] for i in range(5)]
        keep[empty_finger] = keep[empty_finger][:0]
        t["tips"] = torch.cat(keep)
        t["finger_offsets"] = torch.tensor([0] + list(np.cumsum([len(k) for k in keep])), dtype=torch.long)
    return t, model


_VOLUMES = {}


def sphere_volume(res, voxel_scale, rad, dtype):
    """A sphere's exact distance at the voxel centres, the sphere centred in the volume; built once per shape (read-only)."""
    key = (res, voxel_scale, rad, dtype)
    if key not in _VOLUMES:
        ax = (torch.arange(res, dtype=torch.float64) - res // 2 + 0.5) * voxel_scale
        X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
        _VOLUMES[key] = (torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - rad).to(dtype).contiguous()
    return _VOLUMES[key]


def make_scene(tables, res, vol_dtype, seed, lengths=LENGTHS, radii=RADII, with_pred_kp=True):
    """fp32 CPU tensors: frames (eval_metrics.hand_interaction_metrics' dictionary, plus 'global_aa' the root's axis-angle),
    offsets, volumes, voxel_scale."""
    g = torch.Generator().manual_seed(4100 + seed)
    F, f64 = sum(lengths), torch.float64
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    voxel_scale = round(0.45 / res, 4)
    shaped = "shape_joints" in tables
    aa = (torch.tensor([0.25, -0.3, 0.35]) + 0.4 * torch.randn(F, 3, generator=g)).float()
    fr = {"global_aa": aa, "global_rotation": rodrigues(aa.double()).float(),
          "global_translation": (torch.tensor([-0.02, -0.09, 0.5]) + 0.03 * torch.randn(F, 3, generator=g)).float(),
          "MANO_theta": (0.25 * torch.randn(F, 45, generator=g)).float()}
    if shaped:
        fr["beta"] = (0.8 * torch.randn(2, tables["shape_joints"].shape[0], generator=g)).float()
        fr["rest_of"] = torch.arange(F) % 2
    verts, kp = reference_geometry(tables, fr)
    offs = [int(o) for o in tables["finger_offsets"]]
    finger0 = tables["tips"][offs[0]:offs[1]].long()
    Ro = rodrigues(torch.tensor([0.3, -0.5, 0.4], dtype=f64) + 0.3 * torch.randn(F, 3, generator=g).double())
    centres = torch.zeros(F, 3, dtype=f64)
    where = {0: ("off", 0.12), 1: ("tip", 0.0), 2: ("out", 0.30), 3: ("off", RADII[0] + 0.004)}
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        for i, f in enumerate(range(a, b)):
            mid = verts[f].mean(dim=0)
            if q == 0:
                what, d = where[i % 4]
                if what == "tip" and len(finger0):
                    centres[f] = verts[f][finger0].mean(dim=0)
                elif what == "out":  # along the object's own x axis: that coordinate of every vertex is about -d
                    centres[f] = mid + d * Ro[f][:, 0]
                else:
                    centres[f] = mid + d * fr["global_rotation"][f].double() @ torch.tensor([0.0, 0.0, 1.0], dtype=f64)
            else:
                centres[f] = mid + (0.0 if i % 2 == 0 else 0.40) * Ro[f][:, 0]
    fr["obj_rotation"], fr["obj_translation"] = Ro.float().contiguous(), centres.float().contiguous()
    if with_pred_kp:
        fr["pred_kp"] = (kp + 0.004 * torch.randn(F, 21, 3, generator=g).double()).float().contiguous()
    volumes = [None if r is None or n == 0 else sphere_volume(res, voxel_scale, r, vol_dtype) for r, n in zip(radii, lengths)]
    return fr, offsets, volumes, voxel_scale


def reference_geometry(tables, fr):
    """Vertices (F,V,3) and keypoints (F,21,3) in float64 from the fp32 inputs: lbs_forward_from_tables with the fp32-rounded
    root matrix."""
    f64 = torch.float64
    F = fr["MANO_theta"].shape[0]
    beta = fr["beta"].double()[fr["rest_of"].long()] if "beta" in fr else None
    pose = torch.cat([torch.zeros(F, 3, dtype=f64), fr["MANO_theta"].double()], dim=1)
    with torch.no_grad():
        return lbs_forward_from_tables(tables, pose, fr["global_translation"].double(), beta, root_R=fr["global_rotation"].double())


def rows_from_vertices(tables, verts, kp, fr, offsets, volumes, voxel_scale, contact_threshold):
    """The eight columns per frame (metres, float64) from GIVEN fp32 vertices and keypoints: the voxel by oracle.sdf_oracle.nearest
    (bit-exact on fp32 points), plain numpy reductions.  -> rows (F,8), inside counts (F,), sdf per frame (list)."""
    from oracle import sdf_oracle
    verts, kp = np.asarray(verts, dtype=np.float32), np.asarray(kp, dtype=np.float32)
    F, V = verts.shape[:2]
    offs = [int(o) for o in tables["finger_offsets"]]
    regions = [np.unique(tables["tips"][offs[i]:offs[i + 1]].numpy()) for i in range(5)]
    rows, counts, sdfs = np.zeros((F, 8)), np.zeros(F, dtype=np.int64), []
    thr = np.float32(contact_threshold)
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        for f in range(a, b):
            _, sdf, _ = sdf_oracle.nearest(verts[f:f + 1], fr["obj_rotation"][f].numpy(), fr["obj_translation"][f].numpy(),
                                           volumes[q].numpy(), voxel_scale)
            sdf = sdf[0].astype(np.float32)
            sdfs.append(sdf)
            inside = sdf < 0
            counts[f] = inside.sum()
            rows[f, 0] = (-sdf[inside]).max() if inside.any() else 0.0
            rows[f, 1] = np.float32(counts[f]) / np.float32(V)
            rows[f, 2] = float(rows[f, 0] > 0)
            mins = [sdf[r].min() for r in regions if len(r)]
            rows[f, 3] = sum(1 for m in mins if m <= thr)
            rows[f, 4] = np.mean([max(float(m), 0.0) for m in mins]) if mins else 0.0
            rows[f, 5] = sdf.min()
            if "pred_kp" in fr:
                rows[f, 6] = np.linalg.norm(kp[f].astype(np.float64) - fr["pred_kp"][f].double().numpy(), axis=-1).mean()
            rows[f, 7] = float(rows[f, 3] > 0)
    return rows, counts, sdfs


def sequence_means(rows, offsets):
    """The reduce launch restated: float32 rows added in frame order in float64, divided by the length, rounded to float32."""
    rows = np.asarray(rows, dtype=np.float32)
    seq = np.zeros((len(offsets) - 1, rows.shape[1]), dtype=np.float32)
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        for c in range(rows.shape[1]):
            acc = np.float64(0.0)
            for f in range(a, b):
                acc = acc + np.float64(rows[f, c])
            if b > a:
                seq[q, c] = np.float32(acc / np.float64(b - a))
    return seq
