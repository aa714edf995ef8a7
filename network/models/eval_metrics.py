"""The reference's per-sequence evaluation of the object trackers, for all frames of a sequence at once: the symmetry-aware
rotation error, the translation error and the 5 deg 5 cm / 10 deg 10 cm accuracies of `eval_part_full`
(pose_utils/part_dof_utils.py:54-78 over pose_utils/metrics.py:6-143) and the chamfer distance of the two posed clouds
(track_network.py:91-94 after the transforms of :431-432).

Every function has two routes with the same results (tests/test_eval_metrics.py, tests/test_gpu_seq_eval.py):
  * the kernel route (hotrack_amd/csrc/seq_eval.hip): fp32 tensors on the GPU.  A fixed number of launches per sequence
    (one for the pose metrics, two for a chamfer), no host sync, capturable into a HIP graph, run-to-run bitwise equal;
  * the torch route: CPU tensors, other dtypes, any device -- the reference's expressions as batched torch operations, chunked
    over the frames so that the (frames, M, N, 3) difference tensor of the chamfer stays below ~256 MB.
The route is chosen per call; the first time the torch route runs the reason is printed (once per reason).  On the GPU with
fp32 tensors a missing HIP library is an error, not a reason to fall back."""
from __future__ import annotations

import math

import torch

_said = set()
CHUNK_FLOATS = 1 << 26  # torch route: largest difference tensor of one chunk of frames (floats)

# diag(s) for the 180-degree flips rot_diff_rad minimises over (metrics.py:61-90 box, :110-123 bottle): identity, xy, xz, yz
_FLIPS = {3: ((1., 1., 1.), (-1., -1., 1.), (-1., 1., -1.), (1., -1., -1.)), -1: ((1., 1., 1.), (-1., 1., -1.))}


def _kernel_route(route, *tensors) -> bool:
    """True: the HIP kernels run.  route: None (by the tensors), 'torch' or 'kernel' (forced: tests, benchmarks)."""
    if route == "torch":
        return False
    why = None
    for t in tensors:
        if not t.is_cuda:
            why = f"the tensors are on {t.device.type}"
        elif t.dtype != torch.float32:
            why = f"the tensors are {t.dtype}"
        if why:
            break
    if why is not None:
        if route == "kernel":
            raise RuntimeError(f"sequence evaluation: the kernel route needs fp32 GPU tensors ({why})")
        if why not in _said:
            _said.add(why)
            print(f"[Sequence evaluation] the torch route runs: {why}")
        return False
    return True


def _poses(R, t):
    return R.reshape(-1, 3, 3), t.reshape(-1, 3)


def _rot_diff_deg(R1, R2, axis: int, up_and_down_sym: bool):
    """rot_diff_degree (metrics.py:6-139) for (T,3,3) batches."""
    prod = R1 * R2
    if 0 <= axis <= 2:  # angle between the chosen columns
        cos = prod[..., axis].sum(-1).clamp(-1.0, 1.0)
        if up_and_down_sym:
            cos = cos.abs()
        rad = torch.acos(cos)
    else:  # trace(R1 diag(s) R2^T) = sum_k s_k (column k of R1 . column k of R2); the minimum angle over the flips
        signs = torch.tensor(_FLIPS.get(axis, ((1., 1., 1.),)), dtype=R1.dtype, device=R1.device)  # (K,3)
        diag = (prod.unsqueeze(-3) * signs[:, None, :]).sum(-1)  # (T,K,3): the diagonal of R1 diag(s) R2^T
        trace = diag[..., 0] + diag[..., 1] + diag[..., 2]
        rad = torch.acos(((trace - 1) / 2.0).clamp(-1.0, 1.0)).min(dim=-1)[0]
    return rad / math.pi * 180.0


def obj_pose_metrics(gt, pred, axis: int = -1, up_and_down_sym: bool = False, route=None) -> torch.Tensor:
    """gt / pred: {'rotation': (T,[1,]3,3), 'translation': (T,[1,]3[,1])} -> (T,4) = [tdiff (m), rdiff (degrees), 5deg5cm,
    10deg10cm] per frame (eval_part_full's terms before its mean over the batch)."""
    gR, gt_ = _poses(gt["rotation"], gt["translation"])
    pR, pt = _poses(pred["rotation"], pred["translation"])
    pR, pt = pR.to(gR.device), pt.to(gR.device)
    axis = int(axis)
    if _kernel_route(route, gR, gt_, pR, pt):
        from hotrack_amd import ext
        return ext.obj_pose_metrics(gR.contiguous(), gt_.contiguous(), pR.contiguous(), pt.contiguous(), axis, bool(up_and_down_sym))
    tdiff = torch.norm(gt_ - pt, p=2, dim=-1)
    rdiff = _rot_diff_deg(gR, pR, axis, bool(up_and_down_sym))
    acc5 = torch.logical_and(rdiff <= 5.0, tdiff <= 0.05).to(tdiff.dtype)
    acc10 = torch.logical_and(rdiff <= 10.0, tdiff <= 0.10).to(tdiff.dtype)
    return torch.stack([tdiff, rdiff.to(tdiff.dtype), acc5, acc10], dim=-1)


METRIC_KEYS = ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")


def eval_part_full(gt, pred, axis: int = -1, up_and_down_sym: bool = False, route=None) -> dict:
    """The reference's eval_part_full for one part: {'tdiff_0', 'rdiff_0', '5deg5cm_0', '10deg10cm_0'} as means over the
    frames (0-dim tensors on the poses' device: nothing is read back here)."""
    m = obj_pose_metrics(gt, pred, axis, up_and_down_sym, route=route).mean(dim=0)
    return {k: m[i] for i, k in enumerate(METRIC_KEYS)}


def posed_chamfer(A, B, Ra, ta, Rb, tb, route=None) -> torch.Tensor:
    """Per-frame chamfer distance of cloud A (N,3) under the poses (Ra (T,3,3), ta (T,3)) to cloud B (M,3) under (Rb, tb):
    (T,) with out[f] = mean_i min_j |Ra_f a_i + ta_f - (Rb_f b_j + tb_f)| + mean_j min_i |...| (compute_chamfer of the two
    transformed clouds, track_network.py:91-94, :431-433).  Identity poses with T = 1 give the un-posed chamfer."""
    A, B = A.reshape(-1, 3), B.reshape(-1, 3)
    Ra, ta = _poses(Ra, ta)
    Rb, tb = _poses(Rb, tb)
    T = Ra.shape[0]
    if T > 0 and (A.shape[0] == 0 or B.shape[0] == 0):
        raise ValueError(f"posed_chamfer: empty cloud (N = {A.shape[0]}, M = {B.shape[0]})")
    if _kernel_route(route, A, B, Ra, ta, Rb, tb):
        from hotrack_amd import ext
        return ext.posed_chamfer(A.contiguous(), B.contiguous(), Ra.contiguous(), ta.contiguous(), Rb.contiguous(), tb.contiguous())
    out = torch.empty(T, dtype=A.dtype, device=A.device)
    step = max(1, CHUNK_FLOATS // max(A.shape[0] * B.shape[0] * 3, 1))
    for f0 in range(0, T, step):
        f1 = min(T, f0 + step)
        pa = torch.matmul(A, Ra[f0:f1].transpose(-1, -2)) + ta[f0:f1, None, :]  # (c,N,3)
        pb = torch.matmul(B, Rb[f0:f1].transpose(-1, -2)) + tb[f0:f1, None, :]  # (c,M,3)
        dist = torch.norm(pa[:, None, :, :] - pb[:, :, None, :], dim=-1)         # (c,M,N)
        out[f0:f1] = dist.min(dim=1)[0].mean(dim=-1) + dist.min(dim=2)[0].mean(dim=-1)
    return out


def to_eval_frame(pose, eval_frame):
    """The reference's change of evaluation frame for HO3D / DexYCB (track_network.py:417-425): R <- R R_c^T, then
    t <- t - R T_c with the new R.  pose {'rotation' (T,3,3), 'translation' (T,3)}; eval_frame {'rotation', 'translation'}."""
    R, t = _poses(pose["rotation"], pose["translation"])
    Rc = eval_frame["rotation"].to(R.device, R.dtype).reshape(3, 3)
    Tc = eval_frame["translation"].to(R.device, R.dtype).reshape(3, 1)
    R2 = torch.matmul(R, Rc.t())
    return {"rotation": R2, "translation": t - torch.matmul(R2, Tc).squeeze(-1)}
