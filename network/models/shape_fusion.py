"""Tracked depth frames fused into the object's SDF volume -- the online shape update for volumes that come from a mesh or are
handed over.  The reference's `opt.updateobjshape` refits a DeepSDF latent every tenth frame
(optimization_obj.py:308-333, :345-403), which needs its decoder; a volume needs none: every tracked depth frame is integrated as
a truncated signed distance, a weighted running average per voxel (KinectFusion's update).

  tsdf_integrate_torch   the rule of hotrack_amd/csrc/tsdf_fuse.hip in plain torch on any device: the CPU route, and the baseline
                         the kernel is timed against (scripts/bench_tsdf_fuse.py);
  VolumeFusion           a sequence's fused volume and weights: `push` a tracked frame, `flush` integrates what is pending in
                         one launch (hotrack_amd.sdf.tsdf_integrate);
  tsdf_integrate_batch_torch, VolumeFusionGroup   the same for the S sequences of a group tracked in lockstep: one launch per
                         flush for all of them (hotrack_amd.sdf.tsdf_integrate_batch)."""
from __future__ import annotations

import numpy as np
import torch


def tsdf_integrate_torch(volume, weight, voxel_scale, depth, seg, intrinsics, rotation, translation, *, trunc, obj_class=(1, 255),
                         depth_scale=None, flip_yz=False, carve_weight=1.0, max_weight=64.0):
    """hotrack_amd.sdf.tsdf_integrate's arguments and rule (the head of hotrack_amd/csrc/tsdf_fuse.hip) in torch operations, fp32,
    on the tensors' device; the same calls are refused.  Every step makes res^3 temporaries, and the products round where the
    kernel fuses them, so the results agree to rounding, not bit for bit.  In place; a voxel no frame updated keeps its bytes.
    No host synchronisation.  -> (volume, weight), the same tensors."""
    from hotrack_amd.sdf import tsdf_check
    res, F, H, W, Hs, Ws, C, f, raw = tsdf_check(volume, weight, voxel_scale, depth, seg, intrinsics, rotation, translation, trunc,
                                                 obj_class, depth_scale, carve_weight, max_weight)
    dev = volume.device
    for t in (weight, depth, seg, intrinsics, rotation, translation):
        if t.device != dev:
            raise ValueError(f"tsdf_integrate_torch: tensors on {dev} and {t.device}")
    f32 = torch.float32
    ax = (torch.arange(res, device=dev) - res // 2).to(f32) * float(voxel_scale)
    px, py, pz = (g.reshape(-1) for g in torch.meshgrid(ax, ax, ax, indexing="ij"))
    vol_flat, w_flat = volume.view(-1), weight.view(-1)
    V, Wt = vol_flat.to(f32), w_flat.clone()
    touched = torch.zeros(res ** 3, dtype=torch.bool, device=dev)
    trunc, carve, max_weight = float(trunc), float(carve_weight), float(max_weight)
    channel, value = int(obj_class[0]), int(obj_class[1])
    if raw:
        depth = depth.view(torch.int16)
    for k in range(F):
        R, t, K = rotation[k], translation[k], intrinsics[k]
        qx, qy, qz = (R[i, 0] * px + R[i, 1] * py + R[i, 2] * pz + t[i] for i in range(3))
        if flip_yz:
            qy, qz = -qy, -qz
        ok = qz > 1e-6
        zs = torch.where(ok, qz, torch.ones_like(qz))
        u, v = torch.round(qx / zs * K[0] + K[2]), torch.round(qy / zs * K[1] + K[3])
        ok &= (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)   # (a NaN fails every comparison)
        ui, vi = torch.where(ok, u, torch.zeros_like(u)).long(), torch.where(ok, v, torch.zeros_like(v)).long()
        D = depth[k].reshape(-1)[vi * W + ui]
        if raw:
            D = ((D.to(torch.int32) & 0xFFFF).double() * float(depth_scale)).to(f32)
        ok &= torch.isfinite(D) & (D > 0)
        obj = seg[k].reshape(-1)[((vi // f) * Ws + ui // f) * C + channel] == value
        d = D - qz
        upd = ok & torch.where(obj, ~(d < -trunc), d > trunc)
        s = torch.where(obj, d.clamp(max=trunc), torch.full_like(d, trunc))
        g = torch.where(obj, torch.ones_like(d), torch.full_like(d, carve))
        upd &= g != 0
        Wn = Wt + g
        V = torch.where(upd, (V * Wt + s * g) / Wn, V)
        Wt = torch.where(upd, Wn.clamp(max=max_weight), Wt)
        touched |= upd
    vol_flat.copy_(torch.where(touched, V.to(volume.dtype), vol_flat))
    w_flat.copy_(torch.where(touched, Wt, w_flat))
    return volume, weight


class VolumeFusion:
    """The fused SDF volume of one tracked sequence.

    volume: the handed-over (res,res,res) fp16 / fp32 volume -- CLONED: a dataset may share one tensor between sequences, and a
      caller's tensor is never written;  voxel_scale: its stride;  prior_weight: the weight every voxel of the handed-over model
      starts with (0 is allowed: the first observation then replaces the value);  trunc: the truncation distance in metres;
      every: frames between flushes (`due()`);  obj_class / flip_yz: as the depth front end's (models/frame_frontend.py);
      route: None (the kernel for a GPU volume, torch elsewhere), 'kernel' or 'torch'.
    `volume` and `weight` are the state; `frames` counts what has been integrated."""

    def __init__(self, volume: torch.Tensor, voxel_scale: float, prior_weight: float, trunc: float, every: int = 10, obj_class=(1, 255),
                 flip_yz: bool = False, carve_weight: float = 1.0, max_weight: float = 64.0, route=None, device=None):
        if route not in (None, "kernel", "torch"):
            raise ValueError(f"VolumeFusion: route must be None, 'kernel' or 'torch', got {route!r}")
        if int(every) < 1:
            raise ValueError(f"VolumeFusion: every must be >= 1, got {every}")
        if not 0 <= float(prior_weight) < float("inf"):
            raise ValueError(f"VolumeFusion: prior_weight must be finite and >= 0, got {prior_weight}")
        self.device = volume.device if device is None else torch.device(device)
        self.volume = volume.detach().to(self.device, copy=True).contiguous()
        self.weight = torch.full(tuple(self.volume.shape), float(prior_weight), dtype=torch.float32, device=self.device)
        self.voxel_scale, self.trunc, self.every = float(voxel_scale), float(trunc), int(every)
        self.obj_class, self.flip_yz = tuple(obj_class), bool(flip_yz)
        self.carve_weight, self.max_weight = float(carve_weight), float(max_weight)
        self.route = route
        self.frames = 0
        self._pending = []
        self._depth_scale = None

    def _dev(self, t, dtype=None):
        t = torch.as_tensor(t) if not isinstance(t, torch.Tensor) else t
        return t.to(self.device, dtype=dtype, non_blocking=True)

    def push(self, frame: dict, pose: dict) -> None:
        """Queues one tracked frame: `frame` carries depth (H,W) or (1,H,W) (fp32 metres, or uint16 counts with 'depth_scale'),
        seg (Hs,Ws,C) or (1,Hs,Ws,C) and intrinsics ({fx, fy, cx, cy} or the four values); `pose` = {'rotation' (3,3),
        'translation' (3)} in any shape with those element counts.  Tensors already on the device are kept by reference (no
        copy, no host synchronisation); anything else is uploaded."""
        intr = frame["intrinsics"]
        if isinstance(intr, dict):
            intr = [float(np.asarray(torch.as_tensor(intr[k]).cpu()).reshape(-1)[0]) for k in ("fx", "fy", "cx", "cy")]
        if not isinstance(intr, torch.Tensor):
            intr = np.asarray(intr, dtype=np.float32).reshape(4)
        depth = self._dev(frame["depth"])
        depth = depth.reshape(tuple(depth.shape[-2:]))
        if depth.dtype not in (torch.uint16, torch.int16):
            depth = depth.float()
        seg = self._dev(frame["seg"], torch.uint8)
        seg = seg.reshape(tuple(seg.shape[-3:]))
        scale = frame.get("depth_scale")
        if self._pending and (scale is None) != (self._depth_scale is None):
            raise ValueError("VolumeFusion.push: frames with and without 'depth_scale' in one flush")
        self._depth_scale = None if scale is None else float(scale)
        self._pending.append((depth, seg, self._dev(intr, torch.float32).reshape(4),
                              self._dev(pose["rotation"], torch.float32).reshape(3, 3),
                              self._dev(pose["translation"], torch.float32).reshape(3)))

    @property
    def pending(self) -> int:
        return len(self._pending)

    def due(self) -> bool:
        return len(self._pending) >= self.every

    def flush(self) -> torch.Tensor:
        """Integrates the pending frames, in the order they were pushed, with ONE launch (the torch route: one pass per frame),
        and returns the volume.  No host synchronisation."""
        if not self._pending:
            return self.volume
        depth, seg, intr, rot, trans = (torch.stack(x).contiguous() for x in zip(*self._pending))
        use_kernel = self.route == "kernel" or (self.route is None and self.volume.is_cuda)
        if use_kernel:
            from hotrack_amd.sdf import tsdf_integrate as integrate
        else:
            integrate = tsdf_integrate_torch
        integrate(self.volume, self.weight, self.voxel_scale, depth, seg, intr, rot, trans, trunc=self.trunc, obj_class=self.obj_class,
                  depth_scale=self._depth_scale, flip_yz=self.flip_yz, carve_weight=self.carve_weight, max_weight=self.max_weight)
        self.frames += len(self._pending)
        self._pending = []
        return self.volume

    def state(self) -> dict:
        return {"volume": self.volume, "weight": self.weight, "frames": self.frames, "voxel_scale": self.voxel_scale, "trunc": self.trunc}


def tsdf_integrate_batch_torch(volumes, weights, voxel_scale, depth, seg, intrinsics, rotation, translation, frame_counts, *, trunc,
                               obj_class=(1, 255), depth_scale=None, flip_yz=False, carve_weight=1.0, max_weight=64.0):
    """hotrack_amd.sdf.tsdf_integrate_batch's arguments on any device: tsdf_integrate_torch per sequence on its slice of the packed
    frames -- the CPU route, and the baseline the batched launch is timed against.  The same calls are refused, before any volume
    is written.  -> (volumes, weights), the same lists."""
    from hotrack_amd.sdf import tsdf_batch_check
    off, active = tsdf_batch_check(volumes, weights, voxel_scale, depth, seg, intrinsics, rotation, translation, frame_counts, trunc,
                                   obj_class, depth_scale, carve_weight, max_weight)
    for k in active:
        for t in (volumes[k], weights[k], seg, intrinsics, rotation, translation):
            if t.device != depth.device:
                raise ValueError(f"tsdf_integrate_batch_torch: tensors on {depth.device} and {t.device}")
    for k in active:
        a, b = off[k], off[k + 1]
        tsdf_integrate_torch(volumes[k], weights[k], voxel_scale, depth[a:b], seg[a:b], intrinsics[a:b], rotation[a:b], translation[a:b],
                             trunc=trunc, obj_class=obj_class, depth_scale=depth_scale, flip_yz=flip_yz, carve_weight=carve_weight,
                             max_weight=max_weight)
    return volumes, weights


class VolumeFusionGroup:
    """The fused volumes of S sequences tracked in lockstep: S VolumeFusion states, each owning clones as a single one does, whose
    pending frames are integrated together -- `flush(ks)` is ONE launch for the listed sequences
    (hotrack_amd.sdf.tsdf_integrate_batch), and leaves every sequence's volume and weights with the bits its own VolumeFusion
    would have after the same pushes and flushes.

    volumes: S handed-over volumes of one res and dtype (None for a sequence without frames); the other arguments are
    VolumeFusion's and shared by the group."""

    def __init__(self, volumes, voxel_scale: float, prior_weight: float, trunc: float, every: int = 10, obj_class=(1, 255),
                 flip_yz: bool = False, carve_weight: float = 1.0, max_weight: float = 64.0, route=None, device=None):
        self.states = [None if v is None else VolumeFusion(v, voxel_scale, prior_weight, trunc, every, obj_class, flip_yz, carve_weight,
                                                           max_weight, route, device) for v in volumes]
        self.route = route
        self._tables = {}  # tsdf_integrate_batch's cache: the table of a repeated (volumes, counts) is uploaded once

    def push(self, k: int, frame: dict, pose: dict) -> None:
        """VolumeFusion.push for sequence k."""
        self.states[k].push(frame, pose)

    def pending(self, k: int) -> int:
        return 0 if self.states[k] is None else self.states[k].pending

    def due(self, k: int) -> bool:
        return self.states[k] is not None and self.states[k].due()

    def state(self, k: int) -> dict:
        return self.states[k].state()

    def flush(self, ks):
        """Integrates what is pending for the sequences `ks`, each sequence's frames in the order they were pushed, with ONE
        launch (the torch route: one pass per frame and sequence), and returns their volumes, in the order of `ks`.  The pending
        frames must agree in image sizes and in having (and the value of) 'depth_scale'.  No host synchronisation."""
        ks = list(ks)
        todo = sorted(set(k for k in ks if self.pending(k)))
        if todo:
            first = self.states[todo[0]]
            sizes = lambda s: tuple((tuple(fr[0].shape), fr[0].dtype, tuple(fr[1].shape)) for fr in s._pending[:1])
            for k in todo[1:]:
                s = self.states[k]
                if sizes(s) != sizes(first) or s._depth_scale != first._depth_scale:
                    raise ValueError(f"VolumeFusionGroup.flush: sequences {todo[0]} and {k} differ in their frames (depth "
                                     f"{sizes(first)[0][0]} {sizes(first)[0][1]}, seg {sizes(first)[0][2]}, depth_scale {first._depth_scale} against "
                                     f"{sizes(s)[0][0]} {sizes(s)[0][1]}, {sizes(s)[0][2]}, {s._depth_scale}): one launch shares them")
            S = len(self.states)
            frames = [fr for k in todo for fr in self.states[k]._pending]
            depth, seg, intr, rot, trans = (torch.stack(x).contiguous() for x in zip(*frames))
            counts = [self.states[k].pending if k in todo else 0 for k in range(S)]
            vols = [self.states[k].volume if counts[k] else None for k in range(S)]
            wts = [self.states[k].weight if counts[k] else None for k in range(S)]
            kw = dict(trunc=first.trunc, obj_class=first.obj_class, depth_scale=first._depth_scale, flip_yz=first.flip_yz,
                      carve_weight=first.carve_weight, max_weight=first.max_weight)
            if self.route == "kernel" or (self.route is None and first.volume.is_cuda):
                from hotrack_amd.sdf import tsdf_integrate_batch
                tsdf_integrate_batch(vols, wts, first.voxel_scale, depth, seg, intr, rot, trans, counts, cache=self._tables, **kw)
            else:
                tsdf_integrate_batch_torch(vols, wts, first.voxel_scale, depth, seg, intr, rot, trans, counts, **kw)
            for k in todo:
                self.states[k].frames += counts[k]
                self.states[k]._pending = []
        return [self.states[k].volume for k in ks]
