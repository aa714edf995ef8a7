"""Depth frames -> the clouds the trackers read, on the device.

The reference's dataset readers (datasets/HO3D_dataset.py:66-112, :163-177, DexYCB_dataset.py:76-111) turn a depth image, a
segmentation image and the intrinsics into `hand_points` / `obj_points` in numpy on the host: back-project the valid pixels,
split them by segment, crop each segment to a ball (0.15 m round a hand keypoint, 0.25 m round the object's translation), cut
the cloud to 5 * num_points at random, farthest-point sample it to num_points and shuffle.  DepthFrontEnd does it in four launches
for a batch of frames: the two depth-frame kernels (hotrack_amd/csrc/depth_frame.hip), then the project's FPS and row-gather
operators on the (2 B, cap, 3) buffer.  Two deliberate differences: a cloud larger than cap = 5 * num_points is thinned evenly in
pixel rank instead of at random (the cut only bounds FPS's cost), and the sample stays in FPS order (no shuffle)."""
from __future__ import annotations

import numpy as np
import torch


class DepthFrontEnd:
    """npoint: points per cloud;  cap: slots FPS samples from (default 5 * npoint, at most 16384);  hand_radius / obj_radius: the
    crop balls (metres);  hand_class / obj_class: (channel, value) of the segmentation byte (HO3D: channel 0 == 255, channel 1 ==
    255);  flip_yz: negate y and z as HO3D's reader does."""

    def __init__(self, npoint: int, cap: int = None, hand_radius: float = 0.15, obj_radius: float = 0.25, hand_class=(0, 255),
                 obj_class=(1, 255), flip_yz: bool = False, device=None):
        from hotrack_amd import ext
        self.npoint = int(npoint)
        self.cap = 5 * self.npoint if cap is None else int(cap)
        if not self.npoint <= self.cap <= ext.DEPTH_FRAME_MAX_CAP:
            raise ValueError(f"DepthFrontEnd: cap = {self.cap} outside npoint = {self.npoint} .. {ext.DEPTH_FRAME_MAX_CAP} "
                             "(the register-resident FPS range)")
        self.hand_radius, self.obj_radius = float(hand_radius), float(obj_radius)
        self.hand_class, self.obj_class = tuple(hand_class), tuple(obj_class)
        self.flip_yz = bool(flip_yz)
        self.device = torch.device("cuda" if device is None else device)
        self._work = {}   # (B, H, W, cap) -> (tile counts, the (B,2,cap,3) buffer): intermediates only, results are fresh tensors

    @classmethod
    def from_cfg(cls, cfg):
        """cfg['num_points'] and the optional cfg['depth_frontend'] = {cap, hand_radius, obj_radius, hand_class, obj_class, flip_yz}."""
        return cls(cfg["num_points"], device=cfg["device"], **dict(cfg.get("depth_frontend") or {}))

    def clouds(self, frames: dict) -> dict:
        """frames: depth (B,H,W) fp32 metres (or uint16 counts with 'depth_scale'), seg (B,Hs,Ws,C) uint8, intrinsics (B,4) =
        fx, fy, cx, cy, hand_centre / obj_centre (B,3) -- tensors on the device.  -> hand_points / obj_points (B,npoint,3) in FPS
        order, background_mask (B,H,W) uint8 (1 = no segment), counts (B,2) int32: the pixels of each class before the cut to cap
        (a class with fewer than npoint distinct points repeats rows; nothing here reads counts back).  Four launches, no host
        sync, capturable."""
        from hotrack_amd import ext, pointnet2_utils as ops
        depth = frames["depth"]
        B, H, W = depth.shape
        key = (B, H, W, self.cap)
        if key not in self._work:
            self._work[key] = ext.depth_frame_workspace(B, H, W, self.cap, depth.device)[:2]
        tiles, buf = self._work[key]
        work = (tiles, buf, torch.empty((B, 2), dtype=torch.int32, device=depth.device),
                torch.empty((B, H, W), dtype=torch.uint8, device=depth.device))
        _, counts, background = ext.depth_frame_clouds(
            depth, frames["seg"], frames["intrinsics"], self.hand_class + (frames["hand_centre"], self.hand_radius),
            self.obj_class + (frames["obj_centre"], self.obj_radius), self.cap, self.flip_yz, frames.get("depth_scale"), work)
        flat = buf.view(2 * B, self.cap, 3)
        idx = ops.furthest_point_sample(flat, self.npoint)
        pts = ext.gather_rows(flat, idx).view(B, 2, self.npoint, 3)
        return {"hand_points": pts[:, 0], "obj_points": pts[:, 1], "background_mask": background, "counts": counts,
                "sample_idx": idx.view(B, 2, self.npoint)}

    def _dev(self, t, dtype=None):
        t = torch.as_tensor(t) if not isinstance(t, torch.Tensor) else t
        return t.to(self.device, dtype=dtype, non_blocking=True)

    def fill(self, data: dict) -> dict:
        """Completes one frame dict that carries `depth` (H,W) or (1,H,W), `seg` (Hs,Ws,C) or (1,Hs,Ws,C), `intrinsics` ({fx, fy,
        cx, cy} or the four values) and `hand_centre` / `obj_centre` (3 values each; one may be absent and is then the other) but
        not both clouds: sets, where absent, hand_points / obj_points (1,npoint,3), background_mask (H,W) and
        `projection` in the reference's sign convention (HO3D_dataset.py:220: fx negated where y and z are flipped), and
        depth_counts (1,2).  counts are not read back here."""
        intr = data["intrinsics"]
        if isinstance(intr, dict):
            intr = [float(np.asarray(torch.as_tensor(intr[k]).cpu()).reshape(-1)[0]) for k in ("fx", "fy", "cx", "cy")]
        if not (isinstance(intr, torch.Tensor) and intr.is_cuda):
            intr = np.asarray(intr, dtype=np.float32).reshape(4)
        depth = self._dev(data["depth"])
        depth = depth.reshape((1,) + tuple(depth.shape[-2:]))
        seg = self._dev(data["seg"], torch.uint8)
        seg = seg.reshape((1,) + tuple(seg.shape[-3:])).contiguous()
        centres = [data.get("hand_centre"), data.get("obj_centre")]
        if centres[0] is None and centres[1] is None:
            raise KeyError("DepthFrontEnd.fill: the frame carries neither 'hand_centre' nor 'obj_centre'")
        centres = [self._dev(c if c is not None else centres[1 - k], torch.float32).reshape(1, 3).contiguous() for k, c in enumerate(centres)]
        frames = {"depth": depth.contiguous() if depth.dtype in (torch.uint16, torch.int16) else depth.float().contiguous(), "seg": seg,
                  "intrinsics": self._dev(intr, torch.float32).reshape(1, 4).contiguous(), "hand_centre": centres[0],
                  "obj_centre": centres[1]}
        if data.get("depth_scale") is not None:
            frames["depth_scale"] = float(data["depth_scale"])
        out = self.clouds(frames)
        for key, value in (("hand_points", out["hand_points"]), ("obj_points", out["obj_points"]),
                           ("background_mask", out["background_mask"][0])):
            data.setdefault(key, value)   # (what the frame already carries stays)
        data["depth_counts"] = out["counts"]
        if "projection" not in data and not isinstance(intr, torch.Tensor):
            fx, fy, cx, cy = (float(v) for v in intr)
            data["projection"] = {"w": [depth.shape[-1]], "h": [depth.shape[-2]], "fx": [-fx if self.flip_yz else fx], "fy": [fy],
                                  "cx": [cx], "cy": [cy]}
        return data

