"""The observed surface of a tracked object: the clouds the tracker saw, taken into the object frame with the poses it found,
filtered against the model and folded into one merged cloud of fixed size with oriented normals -- the per-frame bookkeeping of
the reference's `opt.updateobjshape` route (optimization_obj.py:153-158 `load_obj`, :308-328 `optimize`, :335-343
`estimate_normal`) without its DeepSDF latent refit (:345-403, needs the decoder).  The reference estimates the normals with
open3d on the host, a device -> host -> device hop per frame; here they come from one launch of
hotrack_amd/csrc/cloud_normals.hip, and a frame's update is device work without a host synchronisation.

The surface lives in the tracker's object frame; the reference's CatCS -> InsCS normalisation is bound to its assets and is not
part of this."""
from __future__ import annotations

import torch

KEY_RANGE = 1 << 40   # random draws per point; key = draw * count + index is unique, so a selection has no ties to break


def to_object_frame(cloud: torch.Tensor, pose):
    """Camera-frame cloud (N,3) or (1,N,3) and a pose {'rotation' (1,3,3), 'translation' (1,3,1)} -> (the cloud (N,3) and the
    camera centre (3,)) in the object frame: (x - t) R, as optimization_obj.py:153-155 and :308, :317."""
    R = pose["rotation"].float().reshape(3, 3).to(cloud.device)
    t = pose["translation"].float().reshape(1, 3).to(cloud.device)
    pts = torch.matmul(cloud.float().reshape(-1, 3) - t, R).contiguous()
    cam = torch.matmul(torch.zeros_like(t) - t, R).reshape(3).contiguous()
    return pts, cam


def selection_keys(draws: torch.Tensor, usable=None) -> torch.Tensor:
    """(n,) int64 draws in [0, KEY_RANGE) -> unique int64 keys, draw * n + index; a point that is not usable gets 2^62 more,
    which puts it behind every usable one.  The `count` smallest keys are the selection."""
    n = draws.shape[0]
    keys = draws.to(torch.int64) * n + torch.arange(n, dtype=torch.int64, device=draws.device)
    if usable is not None:
        keys = torch.where(usable, keys, keys + (1 << 62))
    return keys


class ObservedSurface:
    """`points` (M,3), `normals` (M,3) in the object frame on the device, and `frames`, the number of clouds folded in.

    M: the size of the merged cloud, 3..ext.CLOUD_NORMALS_MAX_N (2048); k: neighbours per normal (open3d's default 30);
    keep_dist: a new point is kept when |SDF| of the model there is below it (the reference's 2 cm); orient: how a normal's sign
    is fixed, see ext.cloud_normals -- the default "reference" is the reference's per-component rule, which is what its refit
    is fed and is NOT a geometric orientation; "view" is the geometric one.  generator: the torch.Generator (on the clouds'
    device) the random choices are drawn from; None = the device's default generator.

    One deliberate difference from the reference: when fewer than M // frames points of a frame pass the filter, the
    reference's merged cloud silently shrinks by the missing ones (its concatenation gets shorter, :322-326).  Here M stays
    fixed: a slot whose drawn new point did not pass keeps its old point and normal."""

    def __init__(self, M: int, k: int = 30, keep_dist: float = 0.02, orient: str = "reference", generator=None):
        from hotrack_amd import ext   # (the range is the normal kernel's: ext.CLOUD_NORMALS_MAX_N / _MAX_K)
        M, k = int(M), int(k)
        if not 3 <= M <= ext.CLOUD_NORMALS_MAX_N:
            raise ValueError(f"ObservedSurface: M = {M}: a merged cloud of 3 to {ext.CLOUD_NORMALS_MAX_N} points (the normal kernel's range)")
        if not 3 <= k <= ext.CLOUD_NORMALS_MAX_K:
            raise ValueError(f"ObservedSurface: k = {k}: 3 to {ext.CLOUD_NORMALS_MAX_K} neighbours")
        if orient not in ("none", "view", "reference"):
            raise ValueError(f"ObservedSurface: orient must be 'none', 'view' or 'reference', got {orient!r}")
        if not keep_dist > 0:
            raise ValueError(f"ObservedSurface: keep_dist = {keep_dist} must be positive")
        self.M, self.k, self.keep_dist, self.orient, self.generator = M, k, float(keep_dist), orient, generator
        self.points = self.normals = None
        self.frames = 0

    def _draws(self, n: int, device) -> torch.Tensor:
        return torch.randint(0, KEY_RANGE, (n,), dtype=torch.int64, device=device, generator=self.generator)

    def start(self, cloud: torch.Tensor, pose, keys=None):
        """The first frame (load_obj, :153-158): the cloud (N,3) / (1,N,3), N >= M, and the camera centre go into the object
        frame with `pose` (the pose tracking starts from), every point gets its normal, frames = 1.  N > M: the M points with
        the smallest random keys are kept (keys: (N,) int64 draws handed in, else drawn from the generator)."""
        from hotrack_amd import ext
        pts, cam = to_object_frame(cloud, pose)
        N = pts.shape[0]
        if N < self.M:
            raise ValueError(f"ObservedSurface.start: a first cloud of {N} points cannot fill {self.M} slots")
        if N > self.M:
            draws = self._draws(N, pts.device) if keys is None else keys
            pts = pts[torch.topk(selection_keys(draws), self.M, largest=False).indices].contiguous()
        normals, _ = ext.cloud_normals(pts[None], k=self.k, viewpoint=cam[None], orient=self.orient)
        self.points, self.normals, self.frames = pts, normals[0], 1
        return self

    def add(self, cloud: torch.Tensor, pose, corner_volume, voxel_scale: float, keys=None):
        """A tracked frame (:308-328): the cloud and the camera centre go into the object frame with the pose just found; the
        points with |SDF| < keep_dist of the model (`corner_volume`: a hotrack_amd.sdf.CornerVolume or volume tensor, read
        with `voxel_scale`) are the usable ones; frames += 1 and choose = M // frames; `choose` random slots of the merged
        cloud are replaced by `choose` random usable new points and their normals, which are estimated among the chosen new
        points only (the reference calls estimate_normal on the subsample).  A slot whose drawn point is not usable keeps its
        old point: M is fixed.  choose < 3 leaves no neighbourhood to estimate from: those points get zero normals.

        keys: ((N,) draws for the new points, (M,) draws for the slots), int64 in [0, KEY_RANGE), else drawn from the generator
        in that order.  The i-th smallest new key is paired with the i-th smallest slot key.
        Device work only: no boolean indexing, nonzero or read-back; the selections are `topk` over the keys with the unusable
        points keyed out, and the filter goes into the normal kernel as its validity mask."""
        from hotrack_amd import ext, sdf
        if self.points is None:
            raise RuntimeError("ObservedSurface.add before start")
        pts, cam = to_object_frame(cloud, pose)
        N = pts.shape[0]
        usable = sdf.distance(pts, corner_volume, float(voxel_scale)).abs() < self.keep_dist
        new_draws, slot_draws = (self._draws(N, pts.device), self._draws(self.M, pts.device)) if keys is None else keys
        self.frames += 1
        choose = min(self.M // self.frames, N)
        if choose == 0:
            return self
        sel = torch.topk(selection_keys(new_draws, usable), choose, largest=False).indices
        slots = torch.topk(selection_keys(slot_draws), choose, largest=False).indices
        new_pts, new_ok = pts[sel].contiguous(), usable[sel].contiguous()
        if choose >= 3:
            new_normals = ext.cloud_normals(new_pts[None], k=self.k, viewpoint=cam[None], valid=new_ok[None], orient=self.orient)[0][0]
        else:
            new_normals = torch.zeros_like(new_pts)
        keep = new_ok[:, None]
        self.points.index_copy_(0, slots, torch.where(keep, new_pts, self.points[slots]))
        self.normals.index_copy_(0, slots, torch.where(keep, new_normals, self.normals[slots]))
        return self

    def state(self):
        """What a tracker reports for the sequence: {'points' (M,3), 'normals' (M,3), 'frames'}."""
        return {"points": self.points, "normals": self.normals, "frames": self.frames}

    def shape_update_samples(self, generator=None):
        """The training triples a shape refit draws from the surface (update_shape, :362-369): for every point p with normal n,
        an outside sample p + n mu_pos, the point itself and an inside sample p - n mu_neg, mu_pos uniform in [0, 0.1) and
        mu_neg in [0, 0.05) -> (xyz (3M,3) = [outside; on; inside], sdf_gt (3M,1) = [mu_pos; 0; -mu_neg] clamped to +-0.2).
        Plain torch on whatever device the surface is on; nothing consumes it yet -- it is the hand-over point of a later refit."""
        p, n = self.points, self.normals
        M = p.shape[0]
        mu_pos = torch.rand((M, 1), dtype=p.dtype, device=p.device, generator=generator) * 0.1
        mu_neg = torch.rand((M, 1), dtype=p.dtype, device=p.device, generator=generator) * 0.05
        xyz = torch.cat([p + n * mu_pos, p, p - n * mu_neg], dim=0)
        sdf_gt = torch.cat([mu_pos, torch.zeros_like(mu_pos), -mu_neg], dim=0).clamp(-0.2, 0.2)
        return xyz, sdf_gt


def surface_fit(points: torch.Tensor, normals: torch.Tensor, corner_volume, voxel_scale: float) -> torch.Tensor:
    """How well the model fits what was seen -> (2,) on the device, no read-back:
      [0] the mean |SDF| of the merged points, in millimetres;
      [1] the mean |n . g| over the points whose g is not zero, g the normalised central-difference gradient of the SDF at the
          point (six more lookups, at +- one voxel along each axis).  With orient "reference" n carries the reference's
          per-component signs, so this can stay below 1 on a perfect fit; "view" and "none" keep n on its line."""
    from hotrack_amd import sdf
    h = float(voxel_scale)
    M = points.shape[0]
    steps = h * torch.eye(3, dtype=points.dtype, device=points.device)
    probes = torch.cat([points[None], points[None] + steps[:, None], points[None] - steps[:, None]]).reshape(7 * M, 3)
    d = sdf.distance(probes.contiguous(), corner_volume, h).reshape(7, M)
    g = (d[1:4] - d[4:7]).t()
    norm = g.norm(dim=1)
    has = norm > 0
    agree = ((normals * g).sum(1).abs() / torch.where(has, norm, torch.ones_like(norm))) * has
    return torch.stack([d[0].abs().mean() * 1000, agree.sum() / has.sum().clamp(min=1)])
