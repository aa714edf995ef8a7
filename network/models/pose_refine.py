"""Gauss-Newton refinement of the tracked object pose on its SDF volume: the route switch and the torch route.

`refine` is what gf_optimize_obj.refine calls: route None / 'kernel' runs hotrack_amd.sdf.obj_refine (one launch,
hotrack_amd/csrc/sdf_refine.hip), route 'torch' runs `obj_refine_torch`, a torch composition of the same rule (stated in
include/pn2_sdf.h and at the head of sdf_refine.hip) on tensors of any device: the CPU route and the timing baseline.  The torch
route is fp32 with torch's own summation order and LAPACK's Cholesky, so it agrees with the kernel to rounding, not bit for bit;
its decisions are selections (torch.where), so it never synchronises with the host either.
"""
from __future__ import annotations

import torch

from hotrack_amd import sdf as _sdf

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, EPS, MIN_GAIN = 1e-3, 1e-7, 1e7, 1e-5, 1e-3


def _pass(cam, pose, vol, res, stride, band, bbox_min):
    """One pass of the rule -> (A (6,6), b (6,), cost (), count ())."""
    R, t = pose[:9].view(3, 3), pose[9:]
    q = (cam - t) @ R
    top = float(res - 1)
    u = (q - bbox_min) / stride
    inside = ((u > 0) & (u < top)).all(dim=1)
    c = torch.nan_to_num(u, nan=0.0).clamp(0.0, top)
    i = c.long()
    f = c - i.to(c.dtype)
    x, y, z = f.unbind(1)
    mx, my, mz = 1 - x, 1 - y, 1 - z
    i000 = (i[:, 0] * res + i[:, 1]) * res + i[:, 2]
    last, rr = vol.numel() - 1, res * res
    d = [vol[(i000 + off).clamp(max=last)] for off in (0, 1, res, 1 + res, rr, 1 + rr, res + rr, 1 + res + rr)]
    c00, c01, c10, c11 = d[0] * mz + d[1] * z, d[2] * mz + d[3] * z, d[4] * mz + d[5] * z, d[6] * mz + d[7] * z
    r0 = (c00 * my + c01 * y) * mx + (c10 * my + c11 * y) * x
    g = torch.stack([((c10 - c00) * my + (c11 - c01) * y) / stride,
                     ((c01 - c00) * mx + (c11 - c10) * x) / stride,
                     (((d[1] - d[0]) * my + (d[3] - d[2]) * y) * mx + ((d[5] - d[4]) * my + (d[7] - d[6]) * y) * x) / stride], dim=1)
    J = torch.cat([torch.linalg.cross(g, q), -(g @ R.t())], dim=1)
    a = r0.abs()
    valid = inside & (a < band)
    knee = 0.5 * band
    w = torch.where(valid, torch.where(a <= knee, torch.ones_like(a), knee / a.clamp_min(1e-30)), torch.zeros_like(a))
    r = torch.where(valid, r0, torch.zeros_like(r0))
    J = torch.where(valid[:, None], J, torch.zeros_like(J))
    v = w[:, None] * J
    count = valid.to(r.dtype).sum()
    return v.t() @ J, v.t() @ r, ((w * r) * r).sum() / count.clamp_min(1.0), count


def _exp_so3(o):
    th2 = (o * o).sum()
    small = th2 < 1e-6
    th = torch.where(small, torch.ones_like(th2), th2.sqrt())
    th2s = torch.where(small, torch.ones_like(th2), th2)
    h = torch.sin(0.5 * th)
    sa = torch.where(small, 1 - th2 / 6, torch.sin(th) / th)
    ca = torch.where(small, 0.5 - th2 / 24, 2 * h * h / th2s)
    zero = torch.zeros_like(th2)
    K = torch.stack([zero, -o[2], o[1], o[2], zero, -o[0], -o[1], o[0], zero]).view(3, 3)
    return torch.eye(3, dtype=o.dtype, device=o.device) * (1 - ca * th2) + ca * torch.outer(o, o) + sa * K


def _normalize(v):
    mag = v.norm()
    unit = torch.tensor([1.0, 0.0, 0.0], dtype=v.dtype, device=v.device)
    return torch.where(mag > 1e-8, v / mag.clamp_min(1e-30), unit)


def _apply(P, delta):
    Rn = P[:9].view(3, 3) @ _exp_so3(delta[:3])
    x = _normalize(Rn[0])
    z = _normalize(torch.linalg.cross(x, Rn[1]))
    y = torch.linalg.cross(z, x)
    return torch.cat([x, y, z, P[9:] + delta[3:]])


def obj_refine_torch(pcld, rotation, translation, volume, voxel_scale, iters=8, band=0.02, trace=False, bbox_min=_sdf.BBOX_MIN):
    """The rule of pn2s_obj_refine in torch, fp32, on the tensors' device.  volume: the LINEAR (res,res,res) volume (a CornerVolume's
    `.source` is taken).  Returns what hotrack_amd.sdf.obj_refine returns; the trace rows carry the first 16 columns and the cost and
    count of the pass ([55], [56]); A, b and delta are the kernel route's."""
    _sdf.refine_check(pcld, rotation, translation, iters, band, voxel_scale)
    vol = getattr(volume, "source", volume)
    res = vol.shape[0]
    dev = pcld.device
    vol = vol.to(dev).reshape(-1).float()
    cam = pcld.reshape(-1, 3).float()
    stride = float(torch.tensor(voxel_scale, dtype=torch.float32))
    band = float(torch.tensor(band, dtype=torch.float32))
    bbox_min = float(torch.tensor(bbox_min, dtype=torch.float32))
    cand = torch.cat([rotation.reshape(9).float(), translation.reshape(3).float()]).to(dev)
    f = lambda x: torch.tensor(float(x), dtype=torch.float32, device=dev)
    P, A_acc, b_acc = cand, torch.zeros(6, 6, device=dev), torch.zeros(6, device=dev)
    lam, c_acc, n_acc, c_0, n_0, steps = f(LAMBDA0), f(0), f(0), f(0), f(0), f(0)
    stepped = torch.zeros((), dtype=torch.bool, device=dev)
    rows = []
    eye = torch.eye(6, device=dev)
    for it in range(iters + 1):
        A, b, cost, cnt = _pass(cam, cand, vol, res, stride, band, bbox_min)
        if it == 0:
            accept = torch.ones((), dtype=torch.bool, device=dev)
            c_0, n_0 = cost, cnt
        else:
            accept = stepped & (cost <= c_acc) & (cnt >= 0.5 * n_acc)
            lam = torch.where(stepped, torch.where(accept, (lam / 3).clamp_min(LAMBDA_MIN), (lam * 10).clamp_max(LAMBDA_MAX)), lam)
            steps = steps + (stepped & accept).float()
        P = torch.where(accept, cand, P)
        A_acc, b_acc = torch.where(accept, A, A_acc), torch.where(accept, b, b_acc)
        c_acc, n_acc = torch.where(accept, cost, c_acc), torch.where(accept, cnt, n_acc)
        C, lam_solve, decided = cand, lam, stepped
        ok = torch.zeros((), dtype=torch.bool, device=dev)
        if it < iters:
            M = A_acc + lam * torch.diag(A_acc.diagonal()) + EPS * n_acc.clamp_min(1.0) * eye
            L, info = torch.linalg.cholesky_ex(torch.where(torch.isfinite(M), M, eye))
            delta = torch.cholesky_solve(-b_acc[:, None], L)[:, 0]
            ok = (info == 0) & torch.isfinite(M).all() & torch.isfinite(delta).all() & (n_acc >= 6) & (-(b_acc * delta).sum() >= MIN_GAIN * c_acc * n_acc.clamp_min(1.0))
            delta = torch.where(ok, delta, torch.zeros_like(delta))
            cand = torch.where(ok, _apply(P, delta), P)
            lam = torch.where(ok, lam, (lam * 10).clamp_max(LAMBDA_MAX))
            stepped = ok
        if trace:
            row = torch.zeros(_sdf.REFINE_TRACE_ROW, device=dev)
            row[:12], row[12], row[13], row[14], row[15] = P, lam, c_acc, n_acc, accept.float()
            row[16:28], row[55], row[56], row[57], row[58], row[59] = C, cost, cnt, lam_solve, ok.float(), decided.float()
            rows.append(row)
    stats = torch.stack([c_0, c_acc, n_0, n_acc, steps, lam, f(0), f(0)])
    out = (P[:9].view(1, 3, 3), P[9:].view(1, 3, 1), stats)
    return out + (torch.stack(rows),) if trace else out


def refine(pcld, rotation, translation, volume, voxel_scale, iters=8, band=0.02, trace=False, route=None):
    """route None: the kernel for GPU tensors, the torch route otherwise; 'kernel' / 'torch' force one."""
    if route not in (None, "kernel", "torch"):
        raise ValueError(f"refine: route must be None, 'kernel' or 'torch', got {route!r}")
    if route == "torch" or (route is None and not pcld.is_cuda):
        return obj_refine_torch(pcld, rotation, translation, volume, voxel_scale, iters, band, trace)
    return _sdf.obj_refine(pcld, rotation, translation, volume, voxel_scale, iters, band, trace)
