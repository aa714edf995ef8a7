"""The tracked object's SDF volume rendered to depth and normal maps, and the rendered frames compared with the observed ones
(DESIGN.md 8m): the raycast of the KinectFusion loop, the image the model predicts at the tracked pose.  The reference has no
counterpart (its vis_utils.py draws matplotlib scatter plots).

  volume_raycast_torch    the rule of hotrack_amd/csrc/sdf_raycast.hip in plain torch on any device: the CPU route, and the baseline
                          the kernel is timed against (scripts/bench_volume_raycast.py);
  raycast_compare_torch   the same for the comparison of rendered and observed frames;
  model_frame_fit         a sequence's frames at their poses against a volume: model_depth_residual(mm), model_silhouette_iou and
                          model_occluded_ratio -- columns that need no ground truth;
  save_depth_png / save_normal_png   the two maps as pictures."""
from __future__ import annotations

import numpy as np
import torch


def _sample(flat, res, lo, scale, px, py, pz):
    """Step 3 of the rule: the trilinear value at (px, py, pz), in the order of the reference's Distance, not clamped."""
    top = float(res - 1)
    zero = torch.zeros((), dtype=px.dtype, device=px.device)
    g = [torch.fmin(torch.fmax((p - lo) / scale, zero), zero + top) for p in (px, py, pz)]
    i = [x.long().clamp(max=res - 2) for x in g]
    x, y, z = (a - b.to(a.dtype) for a, b in zip(g, i))
    i000 = (i[0] * res + i[1]) * res + i[2]
    rr = res * res
    d = lambda off: flat[i000 + off]
    mx, my, mz = 1 - x, 1 - y, 1 - z
    return (((d(0) * mz + d(1) * z) * my + (d(res) * mz + d(res + 1) * z) * y) * mx
            + ((d(rr) * mz + d(rr + 1) * z) * my + (d(rr + res) * mz + d(rr + res + 1) * z) * y) * x)


def volume_raycast_torch(volume, voxel_scale, intrinsics, rotation, translation, hw, flip_yz=False, normals=True, step_scale=1.0,
                         min_step=0.5, refine=8, max_steps=None, return_steps=False):
    """hotrack_amd.sdf.volume_raycast's arguments and rule (the head of hotrack_amd/csrc/sdf_raycast.hip) in torch operations, fp32,
    on the tensors' device; the same calls are refused.  Every step of the march is some forty elementwise launches over all
    pixels of all frames, and the products round where the kernel fuses them, so the results agree to rounding, not bit for bit.
    The march stops when no ray is marching, which it asks the device every eighth step (a host synchronisation the kernel does
    not have).  return_steps: a third result, (F,H,W) int32, the march steps each ray took.
    -> (depth (F,H,W), normal (F,H,W,3) or None[, steps])."""
    from hotrack_amd.sdf import raycast_check
    res, F, H, W, max_steps = raycast_check(volume, voxel_scale, intrinsics, rotation, translation, hw, step_scale, min_step, refine,
                                            max_steps)
    dev = volume.device
    for t in (intrinsics, rotation, translation):
        if t.device != dev:
            raise ValueError(f"volume_raycast_torch: tensors on {dev} and {t.device}")
    f32 = torch.float32
    flat = volume.reshape(-1).to(f32)
    scale = torch.tensor(float(voxel_scale), dtype=f32, device=dev)
    lo = float(-(res // 2)) * scale
    hi = lo + float(res - 1) * scale
    u = torch.arange(W, device=dev, dtype=f32).reshape(1, 1, W)
    v = torch.arange(H, device=dev, dtype=f32).reshape(1, H, 1)
    K = intrinsics.reshape(F, 4, 1, 1)
    cx = ((u - K[:, 2]) / K[:, 0]).expand(F, H, W)
    cy = ((v - K[:, 3]) / K[:, 1]).expand(F, H, W)
    cz = torch.ones((), dtype=f32, device=dev)
    if flip_yz:
        cy, cz = -cy, -cz
    R = rotation.reshape(F, 3, 3, 1, 1)
    t = translation.reshape(F, 3, 1, 1)
    d = [R[:, 2, j] * cz + (R[:, 0, j] * cx + R[:, 1, j] * cy) for j in range(3)]
    o = [-(R[:, 2, j] * t[:, 2] + (R[:, 0, j] * t[:, 0] + R[:, 1, j] * t[:, 1])).expand(F, H, W) for j in range(3)]
    speed = torch.sqrt(d[2] * d[2] + (d[0] * d[0] + d[1] * d[1]))
    a = [(lo - o[j]) / d[j] for j in range(3)]
    b = [(hi - o[j]) / d[j] for j in range(3)]
    z_in = torch.fmax(torch.fmax(torch.fmin(a[0], b[0]), torch.fmin(a[1], b[1])), torch.fmin(a[2], b[2]))
    z_out = torch.fmin(torch.fmin(torch.fmax(a[0], b[0]), torch.fmax(a[1], b[1])), torch.fmax(a[2], b[2]))
    z_in = torch.fmax(z_in, torch.full_like(z_in, 1e-3))
    ray = z_out > z_in
    at = lambda zz: _sample(flat, res, lo, scale, zz * d[0] + o[0], zz * d[1] + o[1], zz * d[2] + o[2])
    z = torch.where(ray, z_in, torch.zeros_like(z_in))
    s = at(z)
    alive = ray & (s > 0)
    hit = torch.zeros_like(alive)
    za, zb, sa, sb = (torch.zeros_like(z) for _ in range(4))
    steps = torch.zeros((F, H, W), dtype=torch.int32, device=dev)
    m = float(min_step) * scale
    for it in range(max_steps):
        if it % 8 == 0 and not bool(alive.any()):
            break
        dz = torch.fmax(s * float(step_scale), m.expand_as(s)) / speed
        zn = torch.fmin(z + dz, z_out)
        sn = at(zn)
        cross = alive & (sn <= 0)
        za, sa = torch.where(cross, z, za), torch.where(cross, s, sa)
        zb, sb = torch.where(cross, zn, zb), torch.where(cross, sn, sb)
        hit = hit | cross
        steps += alive
        alive = alive & ~cross & (zn < z_out)
        z, s = torch.where(alive, zn, z), torch.where(alive, sn, s)
    for _ in range(int(refine)):
        zm = (za + zb) * 0.5
        sm = at(zm)
        neg = sm <= 0
        zb, sb = torch.where(neg, zm, zb), torch.where(neg, sm, sb)
        za, sa = torch.where(neg, za, zm), torch.where(neg, sa, sm)
    zh = za + (zb - za) * sa / (sa - sb)
    depth = torch.where(hit, zh, torch.zeros_like(zh))
    normal = None
    if normals:
        p = [zh * d[j] + o[j] for j in range(3)]
        e = 0.5 * scale
        g = []
        for j in range(3):
            plus, minus = list(p), list(p)
            plus[j], minus[j] = p[j] + e, p[j] - e
            g.append(_sample(flat, res, lo, scale, *plus) - _sample(flat, res, lo, scale, *minus))
        n2 = g[2] * g[2] + (g[0] * g[0] + g[1] * g[1])
        ok = hit & (n2 > 0)
        length = torch.sqrt(torch.where(ok, n2, torch.ones_like(n2)))
        g = [torch.where(ok, x / length, torch.zeros_like(x)) for x in g]
        n = [R[:, i, 2] * g[2] + (R[:, i, 0] * g[0] + R[:, i, 1] * g[1]) for i in range(3)]
        if flip_yz:
            n[1], n[2] = -n[1], -n[2]
        normal = torch.stack(n, dim=-1).contiguous()
    return (depth, normal, steps) if return_steps else (depth, normal)


def raycast_compare_torch(rendered, depth, seg, obj_class=(1, 255), depth_scale=None, occl_margin=None):
    """hotrack_amd.sdf.raycast_compare's arguments and rule in torch operations on the tensors' device; the same calls are refused.
    The counts are exact; the residual sum is torch's, in another order than the kernel's.  -> (F,4) float32."""
    from hotrack_amd.sdf import OCCL_MARGIN, raycast_compare_check
    occl_margin = OCCL_MARGIN if occl_margin is None else occl_margin
    F, H, W, Hs, Ws, C, f, raw = raycast_compare_check(rendered, depth, seg, obj_class, depth_scale, occl_margin)
    for t in (depth, seg):
        if t.device != rendered.device:
            raise ValueError(f"raycast_compare_torch: tensors on {rendered.device} and {t.device}")
    f32 = torch.float32
    if raw:
        D = ((depth.view(torch.int16).to(torch.int32) & 0xFFFF).double() * float(depth_scale)).to(f32)
    else:
        D = depth
    low = seg[..., int(obj_class[0])] == int(obj_class[1])
    obj = low.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2)
    valid = torch.isfinite(D) & (D > 0)
    hit = rendered > 0
    occ = ~obj & valid & hit & (D < rendered - torch.tensor(float(occl_margin), dtype=f32, device=rendered.device))
    a, b = obj & valid, hit & ~occ
    both = a & b
    resid = torch.where(both, (D - rendered).abs(), torch.zeros_like(rendered))
    cnt = lambda msk: msk.reshape(F, -1).sum(dim=1).to(f32)
    return torch.stack([cnt(both), cnt(a | b), resid.reshape(F, -1).sum(dim=1), cnt(occ)], dim=1)


def _frame_tensors(frames, device):
    """The frames' depth (F,H,W), seg (F,Hs,Ws,C), intrinsics (F,4) and depth_scale, as VolumeFusion.push reads them."""
    depth, seg, intr, scale = [], [], [], None
    for fr in frames:
        k = fr["intrinsics"]
        if isinstance(k, dict):
            k = [float(np.asarray(torch.as_tensor(k[n]).cpu()).reshape(-1)[0]) for n in ("fx", "fy", "cx", "cy")]
        if not isinstance(k, torch.Tensor):
            k = torch.from_numpy(np.asarray(k, dtype=np.float32).reshape(4))
        d = torch.as_tensor(fr["depth"]).to(device, non_blocking=True)
        d = d.reshape(tuple(d.shape[-2:]))
        if d.dtype not in (torch.uint16, torch.int16):
            d = d.float()
        s = torch.as_tensor(fr["seg"]).to(device, dtype=torch.uint8, non_blocking=True)
        depth.append(d), seg.append(s.reshape(tuple(s.shape[-3:]))), intr.append(k.to(device, dtype=torch.float32).reshape(4))
        if (fr.get("depth_scale") is None) != (frames[0].get("depth_scale") is None):
            raise ValueError("model_frame_fit: frames with and without 'depth_scale' in one sequence")
        scale = fr.get("depth_scale")
    return torch.stack(depth).contiguous(), torch.stack(seg).contiguous(), torch.stack(intr).contiguous(), scale


COLUMNS = ("model_depth_residual(mm)", "model_silhouette_iou", "model_occluded_ratio")


def fit_columns(stats):
    """(F,4) comparison rows -> the three per-sequence columns as a (3,) tensor and the number of skipped frames as a () tensor, on
    the rows' device, with no host synchronisation:
      model_depth_residual(mm)   mean over frames of 1000 * sum|D - Z| / |A n B|; a frame with an empty intersection is skipped and
                                 counted (no frame left: NaN);
      model_silhouette_iou       mean over frames of |A n B| / |A u B| (an empty union counts as 0);
      model_occluded_ratio       mean over frames of |Occ| / (|Occ| + |A n B|): of the pixels where the model is either compared
                                 with the object or hidden behind something, the hidden share (neither: 0)."""
    n_and, n_or, resid, n_occ = stats.unbind(dim=1)
    has = n_and > 0
    per = torch.where(has, 1000.0 * resid / n_and.clamp(min=1), torch.zeros_like(resid))
    residual = per.sum() / has.sum()   # (0 / 0 = NaN when every frame was skipped)
    iou = (n_and / n_or.clamp(min=1)).mean()
    occluded = (n_occ / (n_occ + n_and).clamp(min=1)).mean()
    return torch.stack([residual, iou, occluded]), (~has).sum()


def model_frame_fit(volume, voxel_scale, frames, poses, obj_class=(1, 255), flip_yz=False, step_scale=1.0, occl_margin=None, route=None,
                    normals=True):
    """How well a volume explains a sequence's depth frames at given poses, with no ground truth: every frame is rendered (one
    launch for all) and compared with the observed frame (a second).
    frames: dicts with 'depth', 'seg', 'intrinsics' (and 'depth_scale' for raw counts), as VolumeFusion.push takes them;
    poses: dicts with 'rotation' (3,3) and 'translation' (3) in any shape with those element counts, one per frame;
    route: None (the kernels for a GPU volume, torch elsewhere), 'kernel' or 'torch'.
    -> {'depth' (F,H,W), 'normal' (F,H,W,3) or None, 'stats' (F,4), 'columns' (3,) in the order of COLUMNS, 'skipped' ()}, all
    tensors on the volume's device; nothing is read back."""
    if route not in (None, "kernel", "torch"):
        raise ValueError(f"model_frame_fit: route must be None, 'kernel' or 'torch', got {route!r}")
    if len(frames) != len(poses) or not len(frames):
        raise ValueError(f"model_frame_fit: {len(frames)} frames and {len(poses)} poses: one pose per frame, at least one frame")
    dev = volume.device
    depth, seg, intr, scale = _frame_tensors(frames, dev)
    rot = torch.stack([torch.as_tensor(p["rotation"]).to(dev, dtype=torch.float32).reshape(3, 3) for p in poses]).contiguous()
    trans = torch.stack([torch.as_tensor(p["translation"]).to(dev, dtype=torch.float32).reshape(3) for p in poses]).contiguous()
    if route == "kernel" or (route is None and volume.is_cuda):
        from hotrack_amd.sdf import raycast_compare as compare, volume_raycast as cast
    else:
        cast, compare = volume_raycast_torch, raycast_compare_torch
    kw = {} if occl_margin is None else {"occl_margin": occl_margin}
    z, n = cast(volume.contiguous(), voxel_scale, intr, rot, trans, tuple(depth.shape[-2:]), flip_yz=flip_yz, normals=normals,
                step_scale=step_scale)
    stats = compare(z, depth, seg, obj_class=obj_class, depth_scale=scale, **kw)
    columns, skipped = fit_columns(stats)
    return {"depth": z, "normal": n, "stats": stats, "columns": columns, "skipped": skipped}


def _png(path, rgb):
    """An (H,W,3) uint8 image as a PNG, with the standard library alone (zlib; no image package is a dependency of this project)."""
    import struct
    import zlib
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = rgb.shape
    rows = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rgb.reshape(h, w * 3)], axis=1).tobytes()   # filter type 0 per row
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))
    return path


def save_depth_png(path, depth):
    """A depth map (H,W), 0 = no hit, as a grey PNG: near is bright, the hits' own range is stretched over 55 .. 255, no hit is black."""
    z = np.asarray(torch.as_tensor(depth).detach().float().cpu()).reshape(tuple(depth.shape[-2:]))
    hit = z > 0
    grey = np.zeros(z.shape, dtype=np.uint8)
    if hit.any():
        near, far = float(z[hit].min()), float(z[hit].max())
        grey[hit] = np.rint(255.0 - 200.0 * (z[hit] - near) / max(far - near, 1e-12)).astype(np.uint8)
    return _png(path, np.repeat(grey[..., None], 3, axis=2))


def save_normal_png(path, normal):
    """A normal map (H,W,3) as an RGB PNG, rgb = 255 (n + 1) / 2; the zero normal (no hit) is black."""
    n = np.asarray(torch.as_tensor(normal).detach().float().cpu()).reshape(tuple(normal.shape[-3:]))
    rgb = np.rint(255.0 * (np.clip(n, -1, 1) + 1) / 2).astype(np.uint8)
    rgb[(n == 0).all(axis=-1)] = 0
    return _png(path, rgb)
