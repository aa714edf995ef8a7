"""Seeded synthetic hand clouds standing in for SimGrasp / HO3D / DexYCB, whose data
is not available offline.  Mirrors what the reference loaders hand to the network
(`datasets/dataset.py`: SingleFrameData for training, SequenceData for tracking tests):
dict(hand_points (N,3), jittered_hand_kp (21,3), gt_hand_kp (21,3), gt_hand_pose.palm_template (6,3)).

A frame is a hand-sized Gaussian blob clipped to a 0.15 m ball at z = 0.5 m plus 21 keypoints; the
initial keypoints are the ground truth + N(0, rand_scale^2) jitter (config hand_jitter_cfg)."""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import Dataset

PALM = [0, 1, 5, 9, 13, 17]


def make_frame(seed: int, num_points: int, jitter: float, motion: np.ndarray | None = None):
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 0.05, (num_points, 3))
    r = np.linalg.norm(pts, axis=-1, keepdims=True)
    pts = np.where(r > 0.15, pts * 0.15 / np.maximum(r, 1e-9), pts)
    off = np.array([0.0, 0.0, 0.5]) + (0 if motion is None else motion)
    gt = rng.normal(0, 0.04, (21, 3))
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return {"hand_points": f(pts + off), "gt_hand_kp": f(gt + off),
            "jittered_hand_kp": f(gt + off + rng.normal(0, jitter, (21, 3))),
            "gt_hand_pose": {"palm_template": f(gt[PALM] - gt[:1])}}


class SyntheticFrames(Dataset):
    """Independent frames (training)."""

    def __init__(self, cfg, length: int, base_seed: int = 0):
        self.n, self.len, self.seed = cfg["num_points"], length, base_seed
        self.jitter = cfg["hand_jitter_cfg"]["rand_scale"]

    def __len__(self):
        return self.len

    def __getitem__(self, i):
        return make_frame(self.seed + i, self.n, self.jitter)


class SyntheticSequences(Dataset):
    """Temporal sequences (tracking test): the hand drifts smoothly; each item is a list of frames with a
    leading batch dimension of 1, like the reference's SequenceData collate."""

    def __init__(self, cfg, num_sequences: int, frames: int):
        self.cfg, self.ns, self.nf = cfg, num_sequences, frames

    def __len__(self):
        return self.ns

    def __getitem__(self, s):
        rng = np.random.default_rng(10_000 + s)
        vel = rng.normal(0, 0.002, 3)
        base = make_frame(20_000 + s, self.cfg["num_points"], self.cfg["hand_jitter_cfg"]["rand_scale"])
        seq = []
        for t in range(self.nf):
            d = torch.from_numpy((vel * t).astype(np.float32))
            noise = make_frame(30_000 + 1000 * s + t, self.cfg["num_points"], 0.0)
            fr = {"hand_points": (noise["hand_points"] + d).unsqueeze(0), "gt_hand_kp": (base["gt_hand_kp"] + d).unsqueeze(0),
                  "jittered_hand_kp": (base["jittered_hand_kp"] + d).unsqueeze(0),
                  "gt_hand_pose": {"palm_template": base["gt_hand_pose"]["palm_template"].unsqueeze(0)},
                  "file_name": [f"synthetic_{s:03d}_{t:03d}"]}
            seq.append(fr)
        return seq


class SyntheticIKFrames(Dataset):
    """Independent frames for training IKNet (`network.type: iknet`, reference SingleFrameData items as IKNet.forward reads them,
    hand_network.py:268-271): the hand model (models/hand_model.HandModel) posed at a seeded sample and
      mano_pose (48): [global axis-angle | 45 joint axis-angles], the joints i.i.d. uniform in [-pose_range, pose_range] rad
                      (default 0.5; SyntheticHandObjectSequences' grasp poses stay within +-0.2), the global rotation uniform
                      over SO(3) (axis uniform on the sphere, angle with density (1 - cos) / pi);
      translation     (0, 0, 0.5) m + uniform [-0.1, 0.1]^3 m;
      mano_beta       (num_betas) ~ N(0, 1) when the model has a shape space;
    gt_hand_kp = the model's keypoints, jittered_hand_kp = gt + N(0, rand_scale^2) (hand_jitter_cfg), palm_template = the palm
    keypoints of the shaped rest hand.  Item i depends only on (base_seed + i)."""

    def __init__(self, cfg, length: int, base_seed: int = 0, pose_range: float = 0.5):
        self.hand = cfg.get("hand_model")
        if self.hand is None or isinstance(self.hand, str):
            from models.hand_model import named_hand_model
            self.hand = named_hand_model(self.hand or "synthetic")
        self.len, self.seed, self.pose_range = length, base_seed, pose_range
        self.jitter = cfg["hand_jitter_cfg"]["rand_scale"]

    def __len__(self):
        return self.len

    def __getitem__(self, i):
        import copy
        rng = np.random.default_rng(self.seed + i)
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        u = rng.uniform()
        ang = 0.0  # angle of a uniform rotation: inverse CDF of (x - sin x) / pi, by bisection
        lo, hi = 0.0, np.pi
        for _ in range(40):
            ang = 0.5 * (lo + hi)
            lo, hi = (ang, hi) if (ang - np.sin(ang)) / np.pi < u else (lo, ang)
        pose = np.concatenate([axis * ang, rng.uniform(-self.pose_range, self.pose_range, 45)])
        trans = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.1, 0.1, 3)
        hm = self.hand if not any(p.is_cuda for p in self.hand.buffers()) else copy.deepcopy(self.hand).cpu()
        nb = int(getattr(hm, "num_betas", 0))
        shape = {"th_betas": f(rng.standard_normal(nb))[None]} if nb else {}
        with torch.no_grad():
            _, kp = hm.forward(th_pose_coeffs=f(pose)[None], th_trans=f(trans)[None], **shape)
            _, rest = hm.forward(th_pose_coeffs=torch.zeros(1, 48), th_trans=torch.zeros(1, 3), **shape)
        gt = kp[0].float()
        pose_d = {"palm_template": rest[0, PALM].float(), "mano_pose": f(pose)}
        if nb:
            pose_d["mano_beta"] = shape["th_betas"][0]
        return {"gt_hand_kp": gt, "jittered_hand_kp": gt + f(rng.normal(0, self.jitter, (21, 3))), "gt_hand_pose": pose_d}


def get_dataloader(cfg, mode="train", shuffle=False, num_workers=0, distributed=False, length=None):
    syn = cfg["data_cfg"].get("synthetic", {})
    if not cfg.get("track") and cfg.get("network", {}).get("type") == "iknet":
        n = length or (syn.get("train_frames", 2048) if mode == "train" else max(cfg["batch_size"] * 4, 64))
        ds = SyntheticIKFrames(cfg, n, base_seed=0 if mode == "train" else 1_000_000)
        sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=shuffle) if distributed else None
        return torch.utils.data.DataLoader(ds, batch_size=cfg["batch_size"], shuffle=shuffle and sampler is None, sampler=sampler,
                                           num_workers=num_workers, drop_last=(mode == "train"))
    if (cfg.get("track") == "hand_IKNet" and (cfg.get("use_optimization") or cfg.get("use_iknet"))
            and cfg.get("hand_model") is not None):
        ds = SyntheticHandObjectSequences(cfg, syn.get("test_sequences", 2), syn.get("sequence_frames", 20) if length is None else length,
                                          hand_beta=syn.get("hand_beta"), obj_as_mesh=bool(cfg.get("obj_as_mesh", False)),
                                          obj_mesh_path=cfg.get("obj_mesh"), from_depth=bool(cfg.get("from_depth", False)))
        return torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, collate_fn=lambda b: b[0])
    if cfg.get("track") == "obj_opt":
        ds = SyntheticObjectSequences(cfg, syn.get("test_sequences", 2), syn.get("sequence_frames", 30) if length is None else length,
                                      obj_as_mesh=bool(cfg.get("obj_as_mesh", False)),
                                      obj_mesh_path=cfg.get("obj_mesh"), from_depth=bool(cfg.get("from_depth", False)),
                                      model_radius=float(cfg.get("obj_model_radius") or 0.04))
        return torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, collate_fn=lambda b: b[0])
    if cfg.get("track"):
        ds = SyntheticSequences(cfg, syn.get("test_sequences", 4),
                                syn.get("sequence_frames", cfg["data_cfg"].get("num_frames", 100)) if length is None else length)
        return torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, collate_fn=lambda b: b[0])
    n = length or (syn.get("train_frames", 2048) if mode == "train" else max(cfg["batch_size"] * 4, 64))
    ds = SyntheticFrames(cfg, n, base_seed=0 if mode == "train" else 1_000_000)
    sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=shuffle) if distributed else None
    return torch.utils.data.DataLoader(ds, batch_size=cfg["batch_size"], shuffle=shuffle and sampler is None, sampler=sampler,
                                       num_workers=num_workers, drop_last=(mode == "train"))


# ---- depth frames (models/frame_frontend.py reads them) ---------------------------------------------------------------
def render_depth_frame(hand_pts, obj_pts, K, h: int, w: int, splat: int = 0, depth_scale: float = 0.001):
    """Z-buffer point splat on the CPU: what a depth camera with intrinsics K = {fx, fy, cx, cy} (or a 3x3 matrix) and an h x w
    sensor sees of two clouds (n,3) in the camera frame (z > 0 forward; either may be None).  A point lands on the pixel nearest
    to its projection (and on the (2 splat + 1)^2 pixels round it) with its own z; the nearest z wins a pixel.
    -> depth (h,w) float32 metres, 0 where nothing landed;  seg (h,w,3) uint8, channel 0 == 255 on the hand's pixels and channel
    1 == 255 on the object's (HO3D's colours);  depth_u16 (h,w) uint16 = round(depth / depth_scale);  depth_scale."""
    if not isinstance(K, dict):
        K = np.asarray(K, dtype=np.float64)
        K = {"fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2]}
    fx, fy, cx, cy = (float(np.asarray(K[k]).reshape(-1)[0]) for k in ("fx", "fy", "cx", "cy"))
    depth = np.full((h, w), np.inf, dtype=np.float32)
    label = np.full((h, w), -1, dtype=np.int64)
    for cls, pts in enumerate((hand_pts, obj_pts)):
        if pts is None or len(pts) == 0:
            continue
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        pts = pts[pts[:, 2] > 1e-6]
        u0 = np.rint(pts[:, 0] / pts[:, 2] * fx + cx).astype(np.int64)
        v0 = np.rint(pts[:, 1] / pts[:, 2] * fy + cy).astype(np.int64)
        z = pts[:, 2].astype(np.float32)
        for dv in range(-splat, splat + 1):
            for du in range(-splat, splat + 1):
                u, v = u0 + du, v0 + dv
                ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
                flat = v[ok] * w + u[ok]
                order = np.argsort(-z[ok], kind="stable")   # far to near: the nearest point is written last
                flat, zz = flat[order], z[ok][order]
                near = zz < depth.reshape(-1)[flat]
                depth.reshape(-1)[flat[near]] = zz[near]
                label.reshape(-1)[flat[near]] = cls
    depth[~np.isfinite(depth)] = 0.0
    seg = np.zeros((h, w, 3), dtype=np.uint8)
    seg[..., 0][label == 0] = 255
    seg[..., 1][label == 1] = 255
    raw = np.clip(np.rint(depth.astype(np.float64) / depth_scale), 0, 65535).astype(np.uint16)
    return depth, seg, raw, float(depth_scale)


def _depth_entries(hand_pts, obj_pts, proj, hand_centre, obj_centre):
    """The entries a `from_depth` frame carries in place of its clouds (leading batch dimension of 1)."""
    depth, seg, _, _ = render_depth_frame(hand_pts, obj_pts, proj, int(proj["h"]), int(proj["w"]), splat=1)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return {"depth": torch.from_numpy(depth)[None], "seg": torch.from_numpy(seg)[None],
            "intrinsics": {k: float(proj[k]) for k in ("fx", "fy", "cx", "cy")},
            "hand_centre": f(hand_centre).reshape(1, 3), "obj_centre": f(obj_centre).reshape(1, 3)}


# ---- object sequences (track: obj_opt) ---------------------------------------------------------------------------------
def _capsule_sdf(p, radius: float = 0.04):
    """Signed distance to a bottle-sized capsule (radius 4 cm, 14 cm core) in the object frame, metres."""
    z = np.clip(p[..., 2], -0.07, 0.07)
    return np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2 + (p[..., 2] - z) ** 2) - radius


def capsule_volume(res: int = 201, stride: float = 0.002, model_radius: float = 0.04) -> np.ndarray:
    """(res,res,res) fp16 SDF volume on the +-0.2 m box the reference voxelises its DeepSDF decoder on
    (optimization_obj.py:133-143: 201^3, stride 0.002, clamped), indexed [ix,iy,iz].  model_radius: the radius of the capsule the
    VOLUME describes -- the clouds and depth frames always show the true one (0.04): another value hands over a wrong model
    (what opt.fuse_depth corrects)."""
    ax = (np.arange(res) - res // 2) * float(stride)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)
    return np.clip(_capsule_sdf(g, float(model_radius)), -0.1, 0.1).astype(np.float16)


def capsule_mesh(n_around: int = 64, n_cap: int = 16):
    """(verts float32 (nv,3), faces int32 (nf,3)): a closed, outward-oriented tessellation of the same capsule with every
    vertex on its surface -- n_around segments around z, n_cap latitude bands per hemispherical cap, one band for the cylinder
    (whose generators are straight); 2 n_around (2 n_cap) faces."""
    phi = np.arange(n_around) * 2 * np.pi / n_around
    theta = np.arange(1, n_cap + 1) * (np.pi / 2) / n_cap   # polar angle of a cap's rings, the last one its equator
    rings = [(0.07 + 0.04 * np.cos(th), 0.04 * np.sin(th)) for th in theta] + [(-0.07 - 0.04 * np.cos(th), 0.04 * np.sin(th)) for th in theta[::-1]]
    verts = [[0.0, 0.0, 0.11]] + [[r * np.cos(a), r * np.sin(a), z] for z, r in rings for a in phi] + [[0.0, 0.0, -0.11]]
    at = lambda ring, j: 1 + ring * n_around + j % n_around
    last, bottom = len(rings) - 1, 1 + len(rings) * n_around
    faces = []
    for j in range(n_around):
        faces.append((0, at(0, j), at(0, j + 1)))
        for k in range(last):  # from ring k down to ring k + 1
            faces += [(at(k, j), at(k + 1, j), at(k + 1, j + 1)), (at(k, j), at(k + 1, j + 1), at(k, j + 1))]
        faces.append((at(last, j), bottom, at(last, j + 1)))
    return np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int32)


def _mesh_entry():
    v, f = capsule_mesh()
    return {"vertices": torch.from_numpy(v), "faces": torch.from_numpy(f)}


def _rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def capsule_surface(rng, n, noise=0.0015):
    """n points on the capsule surface (object frame) + sensor noise."""
    z = rng.uniform(-0.11, 0.11, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    zc = np.clip(z, -0.07, 0.07)
    r = np.sqrt(np.maximum(0.04 ** 2 - (z - zc) ** 2, 0.0))
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)
    return p + rng.normal(0, noise, p.shape)


def model_points(seed: int, n: int = 2048) -> torch.Tensor:
    """(n,3) noise-free samples of the capsule surface in the object frame: the ground-truth cloud of the chamfer metrics
    (`obj_model_points`; the reference samples the object's mesh, track_network.py:398).  A generator of its own, so the
    sequences' other draws do not depend on it."""
    return torch.from_numpy(capsule_surface(np.random.default_rng(seed), n, noise=0.0).astype(np.float32))


class SyntheticObjectSequences(Dataset):
    """Sequences for `track: obj_opt` (reference SequenceData items as ObjTrackModel_Optimization.forward reads them,
    track_network.py:338-383): per frame obj_points (1,N,3) camera frame, gt_obj_pose, category / file_name / projection;
    frame 0 also carries jittered_obj_pose (obj_jitter_cfg: r degrees, t metres), -- in place of the DeepSDF latent the
    reference decodes -- the object's SDF volume, and obj_model_points (2048,3): surface samples for the chamfer metrics.
    obj_as_mesh: frame 0 carries `obj_mesh` ({'vertices', 'faces'}: capsule_mesh()) instead of `sdf_volume` and the tracker
    builds the volume (models/mesh_sdf.py); every other entry and every random draw is unchanged.  obj_mesh_path: frame 0
    carries that `obj_mesh_path` (an OBJ / PLY file, object frame, metres) instead: the clouds are tracked against its volume.
    from_depth: a frame carries, instead of obj_points, a 480 x 640 depth image and segmentation rendered from 16 n surface
    samples of a generator of its own (render_depth_frame), the intrinsics and the crop centre; the tracker builds the cloud
    (models/frame_frontend.py).  Every other entry and every other random draw is unchanged.
    model_radius: the radius of the capsule the handed-over `sdf_volume` describes (capsule_volume); the clouds, the depth frames
    and obj_model_points stay the true capsule's, and every random draw is unchanged."""

    def __init__(self, cfg, num_sequences: int, frames: int, res: int = 201, stride: float = 0.002, obj_as_mesh: bool = False,
                 obj_mesh_path=None, from_depth: bool = False, model_radius: float = 0.04):
        self.from_depth = bool(from_depth)
        self.cfg, self.ns, self.nf = cfg, num_sequences, frames
        self.res, self.stride, self.model_radius = res, stride, float(model_radius)
        self._vol = None
        self.obj_as_mesh, self.obj_mesh_path = bool(obj_as_mesh), obj_mesh_path
        self._mesh = None

    def __len__(self):
        return self.ns

    def __getitem__(self, s):
        if self.obj_mesh_path is not None:
            pass
        elif self.obj_as_mesh:
            if self._mesh is None:
                self._mesh = _mesh_entry()
        elif self._vol is None:
            self._vol = torch.from_numpy(capsule_volume(self.res, self.stride, self.model_radius))
        rng = np.random.default_rng(40_000 + s)
        n = self.cfg["num_points"]
        jit = self.cfg.get("obj_jitter_cfg", {})
        R = _rot(rng.standard_normal(3), rng.uniform(0, np.pi))
        t = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, 3)
        w_axis, w = rng.standard_normal(3), rng.normal(0, 0.01)   # per-frame rotation increment (rad) and velocity (m)
        vel = rng.normal(0, 0.002, 3)
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
        seq = []
        for k in range(self.nf):
            pts = capsule_surface(rng, n) @ R.T + t
            fr = {"obj_points": f(pts).unsqueeze(0), "category": [self.cfg["obj_category"][0]], "file_name": [f"synthetic_obj_{s:03d}/{k:04d}"],
                  "gt_obj_pose": {"rotation": f(R).reshape(1, 1, 3, 3), "translation": f(t).reshape(1, 1, 3, 1)},
                  "projection": {"w": [640], "h": [480]}}
            if self.from_depth:
                del fr["obj_points"]
                dense = capsule_surface(np.random.default_rng(90_000 + 1000 * s + k), 16 * n) @ R.T + t
                proj = dict(fx=600.0, fy=600.0, cx=320.0, cy=240.0, w=640, h=480)
                fr.update(_depth_entries(None, dense, proj, t, t))
            if k == 0:
                ang = np.deg2rad(float(jit.get("r", 5))) * rng.standard_normal()
                Rj = R @ _rot(rng.standard_normal(3), ang)
                tj = t + rng.normal(0, float(jit.get("t", 0.03)) / 3, 3)
                fr["jittered_obj_pose"] = {"rotation": f(Rj).reshape(1, 3, 3), "translation": f(tj).reshape(1, 3, 1)}
                fr["voxel_scale"] = self.stride
                fr.update({"obj_mesh_path": self.obj_mesh_path} if self.obj_mesh_path is not None else
                          {"obj_mesh": self._mesh} if self.obj_as_mesh else {"sdf_volume": self._vol})
                fr["obj_model_points"] = model_points(70_000 + s)
            seq.append(fr)
            R = R @ _rot(w_axis, w)
            t = t + vel
        return seq


class SyntheticHandObjectSequences(Dataset):
    """Sequences for `track: hand_IKNet` with `use_optimization` and a hand model (HandTrackModel's particle-optimisation
    branch, reference track_network.py:142-156, :203-211): a hand (cfg['hand_model'], models/hand_model.HandModel) grasping the
    synthetic capsule.  Per frame: hand_points sampled on the posed hand's vertices (+ sensor noise), gt / jittered keypoints,
    gt_hand_pose (palm template of the model's rest pose, rotation, translation), gt_obj_pose, projection, the silhouette's
    background mask; frame 0 also carries the object's SDF volume and obj_model_points (2048,3) (surface samples, object frame).

    hand_beta: the hand's true shape code beta* for a hand model with a shape space -- None (the zero shape: the data of a
    model without one), a (num_betas,) vector for every sequence, or a float sigma: beta* ~ N(0, sigma^2) per sequence, drawn
    from the sequence's seed.  With a shape, the palm template and every frame come from the shaped hand and gt_hand_pose
    carries `mano_beta` (1, num_betas).

    obj_as_mesh / obj_mesh_path: as in SyntheticObjectSequences -- frame 0 carries `obj_mesh` / `obj_mesh_path` instead of
    `sdf_volume`.
    from_depth: a frame carries, instead of hand_points and background_mask, a depth image and segmentation of the projection's
    size rendered from 16 n samples of the hand and of the capsule (a generator of its own; render_depth_frame), the intrinsics
    and the two crop centres (keypoint 9, the object's translation); the tracker builds the cloud and the mask
    (models/frame_frontend.py).  Every other entry and every other random draw is unchanged."""

    def __init__(self, cfg, num_sequences: int, frames: int, res: int = 151, stride: float = 0.003, hand_beta=None,
                 obj_as_mesh: bool = False, obj_mesh_path=None, from_depth: bool = False):
        self.from_depth = bool(from_depth)
        self.cfg, self.ns, self.nf, self.res, self.stride = cfg, num_sequences, frames, res, stride
        self.hand = cfg["hand_model"]
        self.hand_beta = hand_beta
        self._vol = None
        self.obj_as_mesh, self.obj_mesh_path = bool(obj_as_mesh), obj_mesh_path
        self._mesh = None

    def __len__(self):
        return self.ns

    def __getitem__(self, s):
        if self.obj_mesh_path is not None:
            pass
        elif self.obj_as_mesh:
            if self._mesh is None:
                self._mesh = _mesh_entry()
        elif self._vol is None:
            self._vol = torch.from_numpy(capsule_volume(self.res, self.stride))
        rng = np.random.default_rng(50_000 + s)
        n = self.cfg["num_points"]
        jitter = self.cfg["hand_jitter_cfg"]["rand_scale"]
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
        R_obj = _rot(rng.standard_normal(3), rng.uniform(0, np.pi))
        t_obj = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.03, 0.03, 3)
        proj = dict(fx=600.0, fy=600.0, cx=320.0, cy=240.0, w=640, h=480)
        u, v = t_obj[0] / t_obj[2] * proj["fx"] + proj["cx"], t_obj[1] / t_obj[2] * proj["fy"] + proj["cy"]
        yy, xx = np.mgrid[0:proj["h"], 0:proj["w"]]
        background = torch.from_numpy(~((xx - u) ** 2 + (yy - v) ** 2 < 110 ** 2))
        import copy
        hm = copy.deepcopy(self.hand).cpu()  # (the optimiser's instance lives on the GPU: nn.Module.cpu() moves in place)
        shape = {}
        if self.hand_beta is not None and getattr(hm, "num_betas", 0) > 0:
            hb = self.hand_beta
            beta = (np.random.default_rng(60_000 + s).normal(0, float(hb), hm.num_betas) if np.ndim(hb) == 0
                    else np.asarray(hb, np.float64).reshape(hm.num_betas))
            shape = {"th_betas": f(beta)[None]}
        with torch.no_grad():
            _, rest_kp = hm.forward(th_pose_coeffs=torch.zeros(1, 3 + hm.num_pose), th_trans=torch.zeros(1, 3), **shape)
        palm = rest_kp[:, PALM]
        seq = []
        for k in range(self.nf):
            R_ho = _rot(np.array([0.3, 0.2, 1.0]), 0.15 + 0.02 * k)
            t_ho = np.array([0.002 * k, -0.135 + 0.002 * k, 0.045])
            R = (R_obj @ R_ho).astype(np.float32)
            t = (R_obj @ t_ho + t_obj).astype(np.float32)
            theta = (0.2 * np.sin(np.arange(hm.num_pose) * 0.7 + 0.2 * k)).astype(np.float32)
            # axis-angle of R: the hand model takes the global rotation that way
            ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
            ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2 * np.sin(ang) + 1e-12)
            with torch.no_grad():
                verts, kp = hm.forward(th_pose_coeffs=torch.cat([f(ax * ang)[None], f(theta)[None]], 1), th_trans=f(t)[None], **shape)
            pick = rng.integers(0, verts.shape[1], n)
            pts = verts[0, pick].numpy() + rng.normal(0, 0.0015, (n, 3))
            fr = {"hand_points": f(pts).unsqueeze(0), "gt_hand_kp": kp.clone(), "jittered_hand_kp": kp + f(rng.normal(0, jitter, (1, 21, 3))),
                  "gt_hand_pose": {"palm_template": palm.clone(), "rotation": f(R).reshape(1, 3, 3), "translation": f(t).reshape(1, 3, 1),
                                   "mano_pose": f(theta)[None], **({"mano_beta": shape["th_betas"].clone()} if shape else {})},
                  "gt_obj_pose": {"rotation": f(R_obj).reshape(1, 3, 3), "translation": f(t_obj).reshape(1, 3, 1)},
                  "projection": {kk: [vv] for kk, vv in proj.items()}, "background_mask": background,
                  "category": [self.cfg["obj_category"][0]], "file_name": [f"synthetic_handobj_{s:03d}/{k:04d}"]}
            if self.from_depth:
                del fr["hand_points"], fr["background_mask"]
                drng = np.random.default_rng(90_000 + 1000 * s + k)
                dense_hand = verts[0, drng.integers(0, verts.shape[1], 16 * n)].numpy() + drng.normal(0, 0.0015, (16 * n, 3))
                dense_obj = capsule_surface(drng, 16 * n) @ R_obj.T + t_obj
                fr.update(_depth_entries(dense_hand, dense_obj, proj, kp[0, 9].numpy(), t_obj))
            if k == 0:
                fr["voxel_scale"] = self.stride
                fr.update({"obj_mesh_path": self.obj_mesh_path} if self.obj_mesh_path is not None else
                          {"obj_mesh": self._mesh} if self.obj_as_mesh else {"sdf_volume": self._vol})
                fr["obj_model_points"] = model_points(80_000 + s)
            seq.append(fr)
        return seq
