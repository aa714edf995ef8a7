"""Seeded cases and plain references for the hand-pose kernels (hotrack_amd/csrc/hand_pose.hip) over the shape and dtype range
pn2x_hand_pose_opt_supported accepts.  Everything here runs on the CPU; tests/test_hand_pose_cases.py anchors the references to
tests/golden/hand_opt_sequence.npz and checks every case's preconditions, tests/test_gpu_hand_pose_shapes.py runs the kernels.

  make_case            every input of ext.hand_pose_energy / ext.hand_pose_opt from seeds (CPU tensors; to_kernel() stages them)
  reference_geometry   get_kp_from_delta's composition at [qw | pre * search] through lbs_forward_from_tables, float64
  reference_terms      evaluate()'s terms from GIVEN geometry, in the geometry's dtype, the SDF lookup as oracle/sdf_torch.py
  reference_update     the update step of optimize() in float64 -> (new state, trace row)
  assert_energies      the suite's energy rule (test_gpu_hand_pose._assert_energies) for any P and V; an excluded candidate must
                       be explained by vertices that do sit on a pixel's or a voxel's edge

A case's hand is SyntheticLBSHand(num_verts=V) -- the same skeleton and size as the fixture's hand at every V -- with its K = 2
skinning table rewritten for K = 1, 3, 4 (skinning_tables_for)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from models.hand_model import SyntheticLBSHand, lbs_forward_from_tables, rodrigues  # noqa: E402
from models.rotations import (matrix_to_unit_quaternion, quaternion_to_axis_angle, rotation_from_ortho6d,  # noqa: E402
                              unit_quaternion_to_matrix)
from oracle import sdf_torch  # noqa: E402

GEOM_TOL = 3e-7
E_TOL = 1e-5
KP_TOL, R_TOL, THETA_TOL = 2e-5, 1e-4, 4e-4
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}
THETA_SCALE = 30.0
C2, BETA = 0.1, 0.9  # gf_optimize_hand_pose.scaling_coefficient2 / beta
MAXP = 8192
TIP_KP = (8, 12, 16, 20, 4)  # get_attraction_loss: the tip keypoint of fingers 0..4 of the contact zones
S_R, S_T, S_THETA, S_SEARCH, S_PREV, S_PREV_OK = 0, 9, 12, 57, 73, 89  # the state's layout (include/pn2_ext.h)
MI355X_CUS = 256


# ---- the hand ---------------------------------------------------------------------------------------------------------------------
_TABLES = {}


def skinning_tables_for(V, K):
    """SyntheticLBSHand(num_verts=V).skinning_tables() with K weights per vertex.
    K = 1: the dominant joint with weight 1.
    K = 3, 4: odd vertices split their second weight over copies of the second joint (the vertex does not move); even vertices
    give 30% of the first weight and their second weight to K - 1 columns of which the new ones name OTHER joints, every joint
    0..20 among them (a genuinely different, still plain LBS hand -- both the kernel and the reference read this table, and an
    index read from the wrong 5-bit field moves the vertex by centimetres).
    Where V is too small for the model's own contact zones (fewer than 22 vertices) the five tip regions are dealt over the
    vertices by hand, so that every finger owns a tip vertex (the kernel does not check it)."""
    if (V, K) in _TABLES:
        return _TABLES[(V, K)]
    t = dict(SyntheticLBSHand(num_verts=V).skinning_tables())
    idx2, w2 = t["skin_idx"].long(), t["skin_w"].float()
    i = torch.arange(V)
    if K == 1:
        dom = w2.argmax(dim=1, keepdim=True)
        idx, w = idx2.gather(1, dom), torch.ones(V, 1)
    elif K == 2:
        idx, w = idx2, w2
    else:
        frac = torch.tensor({3: (0.6, 0.4), 4: (0.5, 0.3, 0.2)}[K])
        idx = idx2[:, [0, 1] + [1] * (K - 2)].clone()
        w = torch.cat([w2[:, :1], w2[:, 1:2] * frac[None]], dim=1)
        even = (i % 2) == 0
        w[even] = torch.cat([0.7 * w2[even, :1], (w2[even, 1:2] + 0.3 * w2[even, :1]) * frac[None]], dim=1)
        for k in range(2, K):
            idx[even, k] = (idx2[even, 0] + 1 + 5 * k + i[even] // 2) % 21
    t["skin_idx"], t["skin_w"] = idx.contiguous(), w.contiguous()
    offs = [int(o) for o in t["finger_offsets"]]
    if any(offs[f + 1] == offs[f] for f in range(5)):
        zones = [sorted({f % V, (f + 5) % V}) for f in range(5)]
        t["tips"] = torch.tensor([v for z in zones for v in z], dtype=torch.long)
        t["finger_offsets"] = torch.tensor([0] + list(np.cumsum([len(z) for z in zones])), dtype=torch.long)
    _TABLES[(V, K)] = t
    return t


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _pre_rows(P, seed):
    """The first P of MAXP seeded N(0, I) rows, row 0 the current estimate: cases of one seed share their prefix.  The largest
    entry of 8192 x 16 normal draws is below 5, so with search sizes of 0.005 the quaternion argument 1 - x^2 - y^2 - z^2 stays
    above 0.998."""
    pre = torch.randn(MAXP, 16, generator=torch.Generator().manual_seed(1000 + seed))
    pre[0] = 0
    return pre[:P].contiguous()


def pack_state(R, t, theta, search, prev_search=None, prev_ok=1.0):
    prev_search = search if prev_search is None else prev_search
    return torch.cat([R.reshape(9).float(), t.reshape(3).float(), theta.reshape(45).float(), search.reshape(16).float(),
                      prev_search.reshape(16).float(), torch.tensor([float(prev_ok)])]).contiguous()


def make_case(P, V, K, res, vol_dtype, h, w, seed, *, last_kp=True, vis="mixed", scene="default", obj_shift=(0.0, 0.0, 0.0),
              focal=600.0, centred=False, name=None):
    """Everything ext.hand_pose_energy / ext.hand_pose_opt take, on the CPU, from seeds.
    scene "default": the hand half a metre in front of the camera, as in the fixture; "zneg": the wrist 4 cm in front of the
    camera with the fingers pointing behind it, so a good part of the vertices has z <= 0.
    The object is a sphere of 4 cm, off-centre in its own (rotated) frame, whose surface lies 12 mm beyond the vertex of candidate
    0 nearest to the hand's centroid along the palm's normal: candidate 0 penetrates, the fingertips do not.  `obj_shift` moves
    it away.  The volume holds the sphere's exact distance at the voxel centres, in `vol_dtype`.
    The mask is background outside an ellipse around candidate 0's projection and inside a band through it.
    pred_kp is candidate 0's keypoints moved by about 9 mm plus 2 mm of noise, so that the candidates stepping that way are better
    than candidate 0 and the others are not; last_kp the same keypoints with 3 mm of noise.
    vis: "mixed" (fingertips 8 and 20 and joints 3, 10 invisible), "all", "none".
    centred: the principal point is placed so that candidate 0's centroid projects onto the image centre (with an image smaller
    than the hand's projection, vertices then fall off every edge)."""
    c = SimpleNamespace(name=name or f"P{P}-V{V}-K{K}-res{res}-{_DT[vol_dtype]}", P=P, V=V, K=K, res=res, h=h, w=w,
                        seed=seed, scene=scene, theta_scale=THETA_SCALE, weights=dict(ENERGY_WEIGHT))
    c.tables = skinning_tables_for(V, K)
    g = torch.Generator().manual_seed(seed)
    aa, t0 = ((-1.75, 0.1, 0.2), (0.01, -0.02, 0.04)) if scene == "zneg" else ((0.25, -0.3, 0.35), (-0.02, -0.09, 0.5))
    R0 = rodrigues(torch.tensor(aa, dtype=torch.float64)).float()
    theta = 0.15 * torch.randn(45, generator=g)
    c.state = pack_state(R0, torch.tensor(t0), theta, torch.full((16,), 0.005))
    c.pre = _pre_rows(P, seed)

    v0, k0 = (x[0] for x in reference_geometry(SimpleNamespace(tables=c.tables, state=c.state, pre=c.pre[:1], theta_scale=THETA_SCALE)))

    def noise(sigma):
        return sigma * torch.randn(21, 3, generator=g)

    c.pred_kp = (k0.float() + torch.tensor([0.006, -0.004, 0.005]) + noise(0.002)).contiguous()
    c.last_kp = (k0.float() + noise(0.003)).contiguous() if last_kp else None
    c.vis = torch.ones(21, dtype=torch.bool)
    if vis == "mixed":
        c.vis[[3, 8, 10, 20]] = False
    elif vis == "none":
        c.vis[:] = False

    # ---- the object ------------------------------------------------------------------------------------------------------------
    rad, c_obj = 0.04, torch.tensor([0.016, -0.012, 0.008], dtype=torch.float64)
    anchor = v0[(v0 - v0.mean(dim=0)).norm(dim=1).argmin()]
    centre = anchor + R0.double() @ torch.tensor([0.0, 0.0, rad - 0.012], dtype=torch.float64) + torch.tensor(obj_shift, dtype=torch.float64)
    Ro = rodrigues(torch.tensor([0.3, -0.5, 0.4], dtype=torch.float64))
    c.obj_r, c.obj_t = Ro.float().contiguous(), (centre - Ro @ c_obj).float().contiguous()
    c.voxel_scale = round(0.25 / res, 4) if res > 1 else 0.008
    ax = (torch.arange(res, dtype=torch.float64) - res // 2 + 0.5) * c.voxel_scale
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c.volume = (torch.sqrt((X - c_obj[0]) ** 2 + (Y - c_obj[1]) ** 2 + (Z - c_obj[2]) ** 2) - rad).to(vol_dtype).contiguous()

    # ---- the silhouette -------------------------------------------------------------------------------------------------------------
    cx, cy = w / 2.0, h / 2.0
    if centred:
        mid = v0.mean(dim=0)
        cx, cy = round(cx - float(mid[0] / mid[2]) * focal, 2), round(cy - float(mid[1] / mid[2]) * focal, 2)
    c.proj = {"fx": focal, "fy": focal, "cx": cx, "cy": cy, "w": w, "h": h}
    front = v0[v0[:, 2] > 0.01]
    if len(front) >= 3:
        px, py = front[:, 0] / front[:, 2] * focal + cx, front[:, 1] / front[:, 2] * focal + cy
        mx, my = float(px.median()), float(py.median())
        a, b = min(max(1.2 * float(px.std()), 6.0), w / 3.0), min(max(1.2 * float(py.std()), 6.0), h / 3.0)
    else:
        mx, my, a, b = w / 2.0, h / 2.0, w / 3.0, h / 3.0
    rows, cols = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    c.mask = (((cols - mx) / a) ** 2 + ((rows - my) / b) ** 2 > 1) | ((cols - mx - 0.3 * (rows - my)).abs() < 0.15 * a)
    return c


def fixture_case(frame=0):
    """The committed fixture (tests/golden/hand_opt_sequence.npz) at a frame's initial state, as a case."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "hand_opt_sequence.npz"))

    def T(key):
        return torch.from_numpy(g[key])

    res = int(g["meta"][0])
    pre = T("pre_sampled_particle").float()
    c = SimpleNamespace(name=f"fixture-f{frame}", P=pre.shape[0], V=778, K=2, res=res, scene="fixture", theta_scale=THETA_SCALE,
                        weights=dict(ENERGY_WEIGHT), tables=skinning_tables_for(778, 2), pre=pre)
    fx, fy, cx, cy, w, h = g["proj"].tolist()
    c.proj, c.h, c.w = {"fx": fx, "fy": fy, "cx": cx, "cy": cy, "w": int(w), "h": int(h)}, int(h), int(w)
    c.state = pack_state(T(f"f{frame}_init_rot"), T(f"f{frame}_init_trans"), T(f"f{frame}_init_mano"), torch.full((16,), 0.005))
    c.pred_kp = T(f"f{frame}_init_kp").reshape(21, 3)
    last = g[f"f{frame}_last_kp"]
    c.last_kp = None if last.size == 0 else torch.from_numpy(last).reshape(21, 3)
    c.vis = T(f"f{frame}_vis_mask").reshape(21).bool()
    c.obj_r, c.obj_t = T("R_obj"), T("t_obj")
    c.volume, c.voxel_scale = T("volume").reshape(res, res, res), float(g["meta"][1])
    c.mask = T("background_mask").bool()
    return c, g


def with_state(case, state, pre=None):
    c = SimpleNamespace(**vars(case))
    c.state = state.detach().cpu().float().clone()
    if pre is not None:
        c.pre, c.P = pre, pre.shape[0]
    return c


def to_kernel(case, device="cuda"):
    """The case as the keyword arguments of ext.hand_pose_energy / ext.hand_pose_opt (without `state`)."""
    from hotrack_amd import ext
    m = ext.hand_pose_model(case.tables, device)

    def d(x):
        return x.to(device).contiguous()

    return dict(model=m, rest=ext.hand_pose_rest(m), theta_scale=case.theta_scale, pre=d(case.pre), pred_kp=d(case.pred_kp),
                last_kp=None if case.last_kp is None else d(case.last_kp), vis_mask=d(case.vis.to(torch.uint8)), obj_r=d(case.obj_r),
                obj_t=d(case.obj_t), volume=d(case.volume), voxel_scale=case.voxel_scale, mask=d(case.mask.to(torch.uint8)),
                proj=case.proj, weights=case.weights)


# ---- references ------------------------------------------------------------------------------------------------------------------
def candidate_samples(state, pre, dtype=torch.float64):
    """[qw | pre * search] of optimize() in `dtype`."""
    part = pre.to(dtype) * state.to(dtype)[S_SEARCH:S_SEARCH + 16]
    qw = torch.sqrt(1 - part[:, 0] ** 2 - part[:, 1] ** 2 - part[:, 2] ** 2)
    return torch.cat([qw[:, None], part], dim=1)


def reference_geometry(case, dtype=torch.float64):
    """Vertices (P,V,3) and keypoints (P,21,3) of every candidate: get_kp_from_delta's composition (rotation through the
    quaternion's axis-angle, pose code through the first ten rows of comps) into lbs_forward_from_tables, in float64."""
    st = case.state.to(dtype)
    s = candidate_samples(case.state, case.pre, dtype)
    R = st[S_R:S_R + 9].view(1, 3, 3) @ unit_quaternion_to_matrix(s[:, :4])
    aa = quaternion_to_axis_angle(matrix_to_unit_quaternion(R))
    theta = st[S_THETA:S_THETA + 45] + (s[:, 7:] @ case.tables["comps"][:10].to(dtype)) * case.theta_scale
    with torch.no_grad():
        return lbs_forward_from_tables(case.tables, torch.cat([aa, theta], dim=1), st[S_T:S_T + 3] + s[:, 4:7])


def _saturate(v, n):
    """.float().long() and the clamp to [0, n): see pixel_indices for the values .long() does not define."""
    return torch.nan_to_num(v.float(), nan=-1.0).clamp(-1.0, float(n)).long().clamp(0, n - 1)


def pixel_indices(case, verts):
    """(row, column) of get_silhouette_loss: world2point2D in the vertices' dtype, .float(), .long() (truncation), the clamp to
    the image.  Where x / z is not finite, or beyond int64, .long() is undefined in torch; the reference takes the limit the
    device conversion takes -- it saturates, and NaN (0 / 0) lands on index 0."""
    p = case.proj
    x = verts[..., 0] / verts[..., 2] * p["fx"] + p["cx"]
    y = verts[..., 1] / verts[..., 2] * p["fy"] + p["cy"]
    return _saturate(y, case.h), _saturate(x, case.w)


def reference_terms(case, verts, kp):
    """evaluate() on given geometry, in its dtype, term by term in evaluate()'s order and torch's type promotion: the penetration
    and attraction terms are formed in the volume's dtype.  -> dict: energy (P,), base (energy without attraction), attraction
    (weighted, ungated), penetration, silhouette (the count's fraction), gate."""
    dt, W = verts.dtype, case.weights
    shim = SimpleNamespace(obj_t=case.obj_t.to(dt).reshape(1, 1, 3), obj_r=case.obj_r.to(dt), volume_size=case.res,
                           voxel_scale=case.voxel_scale, sdf_volume=case.volume)
    sdf, pen = sdf_torch.lookup(shim, verts)
    row, col = pixel_indices(case, verts)
    sil = case.mask[row, col].sum(dim=-1) / verts.shape[1]
    err = (kp - case.pred_kp.to(dt)).norm(dim=-1)
    vis = case.vis[None]
    vis_l = (err * vis).sum(dim=-1) / torch.clamp(vis.sum(dim=-1), 1)
    inv_l = (err * ~vis).sum(dim=-1) / torch.clamp((~vis).sum(dim=-1), 1)
    tmp_l = 0 if case.last_kp is None else (kp - case.last_kp.to(dt)).norm(dim=-1).mean(dim=1)
    tips, offs = case.tables["tips"], [int(o) for o in case.tables["finger_offsets"]]
    tips_sdf = sdf[:, tips]
    tips_dis = tips_sdf * (tips_sdf > 0)
    attr = torch.zeros(sdf.shape[0], dtype=sdf.dtype)
    for f in range(5):
        attr = attr + tips_dis[:, offs[f]:offs[f + 1]].min(dim=-1)[0] * ~case.vis[TIP_KP[f]]
    base = 0
    for term, key in ((sil, "sil_loss"), (pen, "penetrate_sum_loss"), (vis_l, "vis_regu_loss"), (inv_l, "invis_regu_loss"),
                      (tmp_l, "temporal_smooth")):
        base = base + term * W[key]
    gate = bool(pen[0] != 0)
    attr_w = attr * W["attraction_loss"]
    energy = base + attr_w if gate else base
    return {"energy": energy, "base": base, "attraction": attr_w, "penetration": pen, "silhouette": sil, "gate": gate,
            "pixels": (row, col)}


def reference_update(state, pre, energy, c2, beta, comps, theta_scale=THETA_SCALE):
    """One update of optimize() (weighted mean of the better candidates, re-projection onto SO(3), theta through comps, search-size
    rule and smoothing) in float64 from the float32 state, rows and energies.  -> (state (90,) float64, trace row (19,) float64)."""
    f64 = torch.float64
    st, e = state.detach().cpu().to(f64).clone(), energy.detach().cpu().to(f64)
    sample = candidate_samples(state.detach().cpu(), pre.detach().cpu(), f64)
    origin = e[0]
    better = e < origin
    weight = (origin - e) * better
    success = bool(better.any())
    new = st.clone()
    if success:
        wsum = weight.sum()
        mean_e = (e * weight).sum() / wsum
        mt = (sample * weight[:, None]).sum(dim=0) / wsum
        mt = torch.cat([mt[:4] / mt[:4].norm(), mt[4:]])
        R = st[S_R:S_R + 9].view(3, 3) @ unit_quaternion_to_matrix(mt[None, :4])[0]
        new[S_R:S_R + 9] = rotation_from_ortho6d(R.reshape(1, 9)[:, :6])[0].t().reshape(9)
        new[S_T:S_T + 3] = st[S_T:S_T + 3] + mt[4:7]
        new[S_THETA:S_THETA + 45] = st[S_THETA:S_THETA + 45] + (mt[7:] @ comps[:10].to(f64)) * theta_scale
    else:
        mean_e, mt = origin, torch.zeros(17, dtype=f64)
    s = mt[1:].abs() + 1e-3
    search = mean_e * c2 * s / s.norm() + 1e-3
    if success and bool(st[S_PREV_OK] != 0):
        search = beta * search + (1 - beta) * st[S_PREV:S_PREV + 16]
    new[S_SEARCH:S_SEARCH + 16] = search
    if success:
        new[S_PREV:S_PREV + 16] = search
    new[S_PREV_OK] = 1.0 if success else 0.0
    return new, torch.cat([torch.stack([origin, mean_e, torch.tensor(float(success), dtype=f64)]), search])


# ---- the energy rule ---------------------------------------------------------------------------------------------------------------
# Two evaluations of the same geometry differ beyond rounding only where a vertex sits on the edge of a voxel or a pixel and the
# two round it to different sides.  How near an edge counts: the object-frame coordinate is a float32 difference and three
# products of values below 1 m (a few 1e-7 m with the geometry's own 3e-7 m where the geometries differ), so 1e-6 m; a pixel
# coordinate x / z * f + c takes three float32 roundings, 1.8e-7 of |x / z * f| + |c|, so 1e-6 of |coordinate| + |c| + 1.
VOXEL_EDGE_M = 1e-6
PIXEL_EDGE_REL = 1e-6


def _steps(n):
    """Every combination of -1, 0, +1 over n axes, (3 ** n, n)."""
    return torch.cartesian_prod(*[torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)] * n).reshape(-1, n)


def energy_cap(P):
    """The suite's 2 excluded candidates per 768, scaled: ceil(P / 384), never below 2."""
    return max(2, math.ceil(P / 384))


def silhouette_count_range(case, verts):
    """(lowest, highest) background count of every candidate (..., V, 3) when each vertex within PIXEL_EDGE_REL of a pixel's edge
    may fall on either side of it."""
    p, v = case.proj, verts.double()
    coords = []
    for axis, f, c in ((0, p["fx"], p["cx"]), (1, p["fy"], p["cy"])):
        x = v[..., axis] / v[..., 2] * f + c
        d = torch.where(torch.isfinite(x), PIXEL_EDGE_REL * (x.abs() + abs(c) + 1), torch.zeros_like(x))
        coords.append((x, torch.nan_to_num(d, posinf=0.0)))
    (x, dx), (y, dy) = coords
    lo = hi = None
    for sx, sy in _steps(2).tolist():
        row = _saturate(y + sy * dy, case.h)
        col = _saturate(x + sx * dx, case.w)
        m = case.mask[row, col]
        lo, hi = (m, m) if lo is None else (lo & m, hi | m)
    return lo.sum(dim=-1), hi.sum(dim=-1)


def sdf_term_alternatives(case, verts_q):
    """(penetration values, weighted attraction values) one candidate (V, 3) can take when each vertex within VOXEL_EDGE_M of a
    voxel's face may be looked up on either side of it: only values of voxels ADJACENT to the looked-up ones, and only those the
    maximum / the per-finger minimum can actually reach.  The attraction is summed and weighted in the volume's dtype, as
    reference_terms does."""
    half, W = case.res // 2, case.weights
    o = (verts_q.double() - case.obj_t.double().reshape(1, 3)) @ case.obj_r.double()
    u = o / case.voxel_scale
    idx = torch.floor(u[:, None, :] + (VOXEL_EDGE_M / case.voxel_scale) * _steps(3)[None]).clamp(-half, half).long() + half
    s = case.volume[idx[..., 0], idx[..., 1], idx[..., 2]]  # (V, 27), the volume's dtype
    neg, pos = s.abs() * (s < 0), s * (s > 0)
    pens = torch.unique(neg[neg >= neg.min(dim=1)[0].max()]).double().tolist()
    tips, offs = case.tables["tips"], [int(x) for x in case.tables["finger_offsets"]]
    per_finger = []
    for f in range(5):
        t = pos[tips[offs[f]:offs[f + 1]]]
        per_finger.append(torch.unique(t[t <= t.max(dim=1)[0].min()]))
    combos = torch.cartesian_prod(*per_finger).reshape(-1, 5)
    assert combos.shape[0] <= 4096, f"{combos.shape[0]} attraction alternatives: the case sits on too many voxel faces"
    attr = torch.zeros(combos.shape[0], dtype=s.dtype)
    for f in range(5):
        attr = attr + combos[:, f] * ~case.vis[TIP_KP[f]]
    return pens, torch.unique(attr * W["attraction_loss"]).double().tolist()


def explained_by_discrete_steps(case, terms, verts, q, got_q):
    """Whether energy `got_q` of candidate q is the reference's (terms = reference_terms(case, verts, kp)) with vertices on a
    pixel's or a voxel's edge counted on the other side: the keypoint terms as they are, a silhouette count within
    silhouette_count_range, a penetration and an attraction out of sdf_term_alternatives, to E_TOL."""
    W, V = case.weights, verts.shape[1]
    step = W["sil_loss"] / V
    cont = float(terms["base"][q]) - float(terms["silhouette"][q]) * W["sil_loss"] - float(terms["penetration"][q]) * W["penetrate_sum_loss"]
    lo, hi = (int(x) for x in silhouette_count_range(case, verts[q]))
    pens, attrs = sdf_term_alternatives(case, verts[q])
    for pen in pens:
        for attr in (attrs if terms["gate"] else [0.0]):
            rest = got_q - cont - pen * W["penetrate_sum_loss"] - attr
            count = min(max(round(rest / step), lo), hi)
            if abs(rest - count * step) <= E_TOL:
                return True
    return False


def assert_energies(got, terms, case, verts, what):
    """The suite's energy rule (test_gpu_hand_pose._assert_energies) for any P and V, with a discrete step that binds: `got`
    against terms["energy"] (terms = reference_terms(case, verts, kp)) within E_TOL for all but at most energy_cap(P)
    candidates, and each excluded candidate explained_by_discrete_steps -- k silhouette pixels (w_sil / V each) for k vertices
    that do sit on a pixel's edge across which the mask changes, plus a penetration / attraction change between values of voxels
    adjacent to the ones its vertices look up.  A difference of any other size fails, at P = 1 too."""
    got, want = np.asarray(got, dtype=np.float64), terms["energy"].double().numpy()
    assert got.shape == want.shape == (case.P,) and np.isfinite(got).all(), f"{what}: shape {got.shape} or a non-finite energy"
    diff = np.abs(got - want)
    bad = np.nonzero(~(diff <= E_TOL))[0]
    print(f"{what}: max |dE| = {diff.max():.3e}, candidates beyond {E_TOL:g}: {len(bad)} of {case.P} {diff[bad][:8].tolist()}")
    assert len(bad) <= energy_cap(case.P), f"{what}: {len(bad)} candidates differ by more than {E_TOL:g}"
    for q in bad:
        assert explained_by_discrete_steps(case, terms, verts, int(q), float(got[q])), \
            f"{what}: candidate {q} differs by {diff[q]:.3e}, which no vertex on a pixel's or a voxel's edge explains"
    return float(diff.max()), len(bad)


# ---- the table of tests/test_gpu_hand_pose_shapes.py ---------------------------------------------------------------------------------
H, W = 480, 640
F16, F32 = torch.float16, torch.float32
_DT = {F16: "fp16", F32: "fp32"}


def second_pass_counts(cus):
    """eval_launch covers the compute units three times with workgroups of four candidates: up to 12 * cus candidates every wave
    has one, from 12 * cus + 1 the first waves take a second."""
    first = min(12 * cus, MAXP - 5)
    return [first, first + 1, first + 5]


def eval_case_specs(cus=MI355X_CUS):
    """name -> make_case arguments, the evaluation table of the GPU test.  The candidate counts around the second pass depend on
    the device's compute-unit count; every other row is the same everywhere."""
    s = {}

    def add(name, P, V, K, res, dt, seed, h=H, w=W, **kw):
        s[name] = dict(P=P, V=V, K=K, res=res, vol_dtype=dt, h=h, w=w, seed=seed, **kw)

    add("one-candidate", 1, 70, 2, 31, F16, 1)
    add("ragged-5", 5, 778, 2, 31, F32, 2)
    add("ragged-7", 7, 778, 2, 31, F32, 2)
    for extra, P in zip((0, 1, 5), second_pass_counts(cus)):
        add(f"second-pass+{extra}", P, 70, 2, 31, F16, 3)
    for dt in (F16, F32):
        add(f"workload-5120-{_DT[dt]}", 5120, 70, 2, 31, dt, 4)
        add(f"limit-8192-{_DT[dt]}", 8192, 70, 2, 31, dt, 4)
    for V in (7, 33, 64, 65, 255, 256, 257):
        add(f"verts-{V}", 64, V, 2, 31, F16, 5)
    add("lds-above-64k", 16, 1024, 4, 31, F32, 6)
    for K in (1, 3, 4):
        add(f"weights-{K}", 64, 778, K, 31, F16, 7)
    add("no-last-kp", 64, 130, 2, 31, F16, 8, last_kp=False)
    add("with-last-kp", 64, 130, 2, 31, F16, 8)
    add("all-visible", 64, 130, 2, 31, F16, 8, vis="all")
    add("none-visible", 64, 130, 2, 31, F16, 8, vis="none")
    add("off-image", 64, 130, 2, 31, F32, 9, h=60, w=100, centred=True)
    add("behind-camera", 64, 130, 2, 31, F32, 10, h=96, w=72, scene="zneg", focal=30.0)
    for dt in (F16, F32):
        add(f"res-1-{_DT[dt]}", 64, 130, 2, 1, dt, 11)
        add(f"res-101-{_DT[dt]}", 64, 130, 2, 101, dt, 12)
    add("gate-off", 64, 130, 2, 31, F16, 8, obj_shift=(0.0, 0.0, 1.0))
    return s


EVAL_CASES = tuple(eval_case_specs())  # the names do not depend on the compute-unit count
UPDATE_P = (1, 5, 63, 64, 1023, 1025, 8192)
_CASES = {}


def get_case(name, cus=MI355X_CUS):
    """A table case by name, built once (the cases are read-only)."""
    key = (name, cus)
    if key not in _CASES:
        _CASES[key] = make_case(name=name, **eval_case_specs(cus)[name])
    return _CASES[key]


def update_case(P):
    key = ("update", P)
    if key not in _CASES:
        _CASES[key] = make_case(P, 70, 2, 31, F16, H, W, seed=20, name=f"update-{P}")
    return _CASES[key]


def reference_energies(case):
    """The energies of a case in float64 end to end (for choosing rows and checking preconditions, not for comparing kernels)."""
    return reference_terms(case, *reference_geometry(case))["energy"].double()


def branch_rows(case):
    """(the best row, the worst row) of the case by its float64 energies: the material of the single-candidate update cases."""
    e = reference_energies(case)
    return int(e.argmin()), int(e.argmax())


def single_row_case(case, P, row, at):
    """P candidates that are all the current estimate (zero rows: their energies EQUAL candidate 0's) except row `row` of the
    case at index `at`."""
    pre = torch.zeros(P, 16)
    pre[at] = case.pre[row]
    return with_state(case, case.state, pre=pre)
