"""Object-pose particle optimiser -- counterpart of the reference's gf_optimize_obj
(network/models/optimization_obj.py:81-301) for the part that is data-parallel hot path: the SDF-volume
evaluation of 2048 candidate poses per iteration.

Same attribute / method names as the reference (`Distance`, `evaluate`, `update_seach_size`, `optimize`,
`sdf_volume`, `volume_size`, `voxel_scale`, `pre_sampled_particle`, ...), so `track_network`-style callers work
unchanged.  Out of scope here (and raising if requested): decoding the volume from a DeepSDF latent code
(`load_obj`, :106-161 -- needs the checkpoints) and the online shape update (`update_shape`, :345-403); the
volume is handed over with `load_volume`.
"""
from __future__ import annotations

import numpy as np
import torch

from hotrack_amd import sdf as _sdf


class gf_optimize_obj:
    def __init__(self, cfg=None, device="cuda", seed=None):
        self.particle_size = 2048  # :85-91
        self.iteration = 10
        self.scaling_coefficient1 = 0.02
        self.scaling_coefficient2 = 2
        self.volume_size = 201
        self.voxel_scale = 0.002
        self.beta = 0.9
        cfg = cfg or {}
        self.update_shape_flag = bool(cfg.get("opt", {}).get("updateobjshape", False))
        if self.update_shape_flag:
            raise NotImplementedError("online DeepSDF shape update (optimization_obj.py:345-403) is out of scope")
        # opt.refine_pose (the tracker's switch): Gauss-Newton steps after the particle search, and the residual band
        self.refine_iters = int((cfg.get("opt") or {}).get("refine_iters", _sdf.REFINE_ITERS))
        self.refine_band = float((cfg.get("opt") or {}).get("refine_band", _sdf.REFINE_BAND))
        self.device = torch.device(cfg.get("device", device))
        # pre-sampled particles (:103-107): N(0, I_6), particle 0 is the current pose
        rng = np.random.default_rng(seed) if seed is not None else np.random
        pre = rng.multivariate_normal(np.zeros(6), np.eye(6), self.particle_size)
        pre[0, :] = 0
        self.pre_sampled_particle = torch.tensor(pre, dtype=torch.float32, device=self.device)
        self.sdf_volume = None
        self._work = None
        self._batch_work, self._batch_cache = None, {}  # optimize_batch: scratch; uploaded offsets / volume pointer tables

    def load_volume(self, sdf_volume: torch.Tensor, voxel_scale: float | None = None):
        """Install a (V,V,V) fp16/fp32 SDF volume (what load_obj produces at :139-149)."""
        V = sdf_volume.shape[0]
        assert sdf_volume.dim() == 3 and tuple(sdf_volume.shape) == (V, V, V)
        self.volume_size = V
        if voxel_scale is not None:
            self.voxel_scale = float(voxel_scale)
        self.sdf_volume = sdf_volume.to(self.device).contiguous()
        self._corners = _sdf.CornerVolume(self.sdf_volume)  # lookup layout (8x memory, same results), built once per object

    def sdf2mesh(self, mesh_filename=None, level: float = 0.0, route=None):
        """The triangle mesh of the loaded volume's `level` set (the reference's sdf2mesh, :399-405, which decodes its latent on
        a 128^3 grid and runs marching cubes; here the volume the tracker looks up is extracted, models/mesh_sdf.volume_to_mesh).
        Writes it to `mesh_filename` (PLY, or OBJ by extension) when one is given.  Returns (verts fp32 (nv,3), faces int32 (nf,3))."""
        if self.sdf_volume is None:
            raise RuntimeError("sdf2mesh: no SDF volume is loaded (load_volume)")
        from . import mesh_sdf
        verts, faces = mesh_sdf.volume_to_mesh(self.sdf_volume, self.voxel_scale, level, route=route)
        if mesh_filename is not None:
            mesh_sdf.save_mesh(mesh_filename, verts, faces)
        return verts, faces

    def Distance(self, V):  # noqa: N802 (reference name)
        return _sdf.distance(V.float(), self._corners, self.voxel_scale)

    def evaluate(self, pcld, r, t):
        """pcld (1,N,3), r (P,3,3), t (P,3,1) -> (energy, sdf_energy), each (P,)."""
        sdf_energy = _sdf.particle_energy(pcld.float(), r.float(), t.float(), self._corners, self.voxel_scale)
        return sdf_energy * 500, sdf_energy

    def update_seach_size(self, tsdf, mean_transform):  # reference spelling
        s = mean_transform.abs() + 1e-3
        return tsdf * self.scaling_coefficient2 * s / s.norm() + 1e-3

    def optimize(self, pcld, init_obj_pose, category=None, file_name=None, projection=None):
        """Ten particle iterations around init_obj_pose; returns {'rotation' (1,3,3), 'translation' (1,3,1)}.
        One call enqueues 11 kernels and never synchronises with the host."""
        rotation = init_obj_pose["rotation"].float().to(self.device)
        translation = init_obj_pose["translation"].float().to(self.device)
        pcld = pcld.float().to(self.device)
        need = 16 + self.pre_sampled_particle.shape[0]
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=self.device)
        R, t = _sdf.obj_optimize(pcld, rotation, translation, self.pre_sampled_particle, self._corners, self.voxel_scale,
                                 iterations=self.iteration, scaling_coefficient1=self.scaling_coefficient1,
                                 scaling_coefficient2=float(self.scaling_coefficient2), beta=self.beta, work=self._work)
        return {"rotation": R, "translation": t.reshape(1, 3, 1)}

    def refine(self, pcld, pose, route=None):
        """opt.refine_pose: `refine_iters` damped Gauss-Newton steps on the SDF volume from `pose` (what `optimize` returned) -- one
        more launch, no host synchronisation (models/pose_refine.py, hotrack_amd/csrc/sdf_refine.hip).  Returns {'rotation' (1,3,3),
        'translation' (1,3,1), 'refine_stats' (8,)}; the final cost (stats[1]) is never above the initial one (stats[0])."""
        from . import pose_refine
        R, t, stats = pose_refine.refine(pcld.float().to(self.device), pose["rotation"].float().to(self.device),
                                         pose["translation"].float().to(self.device), self._corners, self.voxel_scale,
                                         iters=self.refine_iters, band=self.refine_band, route=route)
        return {"rotation": R, "translation": t.reshape(1, 3, 1), "refine_stats": stats}

    def refine_batch(self, pclds, poses, corner_volumes, voxel_scale=None):
        """`refine` for S problems with one launch (hotrack_amd.sdf.obj_refine_batch), next to `optimize_batch` and with its
        conventions: an empty cloud or None sits out, its pose comes back unchanged (and its stats are zero).  Returns S dicts,
        each bit-equal to what `refine` returns for it."""
        S = len(poses)
        if S == 0:
            return []
        poses = [{k: p[k].float().to(self.device) for k in ("rotation", "translation")} for p in poses]
        pclds = [None if c is None else c.float().to(self.device) for c in pclds]
        R, t, stats = _sdf.obj_refine_batch(pclds, [p["rotation"] for p in poses], [p["translation"] for p in poses], list(corner_volumes),
                                            self.voxel_scale if voxel_scale is None else float(voxel_scale), iters=self.refine_iters,
                                            band=self.refine_band, cache=self._batch_cache)
        return [{"rotation": R[k:k + 1], "translation": t[k:k + 1], "refine_stats": stats[k]} for k in range(S)]

    def forget_volume_tables(self):
        """Drops optimize_batch's cached volume pointer tables, which keep their volumes alive: for a caller that has just
        replaced volumes of its group (the next call uploads one table again)."""
        for key in [k for k in self._batch_cache if k[0] == "vols"]:
            del self._batch_cache[key]

    def optimize_batch(self, pclds, init_obj_poses, corner_volumes, voxel_scale=None):
        """`optimize` for S independent problems (one frame step of S sequences) with one set of launches: the same 11
        kernels over a (particle, problem) grid (hotrack_amd.sdf.obj_optimize_batch).  pclds: S clouds, an empty one or
        None for a problem that sits this step out (its pose is returned unchanged); init_obj_poses: S pose dicts;
        corner_volumes: S hotrack_amd.sdf.CornerVolume (None where the problem sits out), all of one resolution and dtype and
        read with `voxel_scale` (default: this instance's).  Shares the instance's pre_sampled_particle and constants.
        Returns S dicts {'rotation' (1,3,3), 'translation' (1,3,1)}, each bit-equal to what `optimize` returns for it."""
        S = len(init_obj_poses)
        if S == 0:
            return []
        poses = [{k: p[k].float().to(self.device) for k in ("rotation", "translation")} for p in init_obj_poses]
        pclds = [None if c is None else c.float().to(self.device) for c in pclds]
        if len(self._batch_cache) > 64:  # (a long evaluation with ever new groups of volumes: start over)
            self._batch_cache.clear()
        need = _sdf.obj_optimize_batch_work_floats(S, self.pre_sampled_particle.shape[0])
        if self._batch_work is None or self._batch_work.numel() < need:
            self._batch_work = torch.empty(need, dtype=torch.float32, device=self.device)
        R, t = _sdf.obj_optimize_batch(pclds, [p["rotation"] for p in poses], [p["translation"] for p in poses],
                                       self.pre_sampled_particle, list(corner_volumes),
                                       self.voxel_scale if voxel_scale is None else float(voxel_scale),
                                       iterations=self.iteration, scaling_coefficient1=self.scaling_coefficient1,
                                       scaling_coefficient2=float(self.scaling_coefficient2), beta=self.beta,
                                       work=self._batch_work, cache=self._batch_cache)
        return [{"rotation": R[k:k + 1], "translation": t[k:k + 1]} for k in range(S)]
