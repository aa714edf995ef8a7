"""Seeded cases and the plain float64 reference for the fused hand-loss kernels (hotrack_amd/csrc/kabsch.hip: pn2x_hand_losses,
pn2x_hand_losses_backward).  Everything here is CPU tensors and plain torch: no GPU, no extension import.
tests/test_hand_loss_cases.py anchors the reference to HandTrackNet.compute_loss and checks every case's preconditions,
tests/test_gpu_hand_losses.py runs the kernels.

  reference   the nine entries of NAMES (ext.HAND_LOSS_NAMES) and, with weights, their weighted total, in float64; differentiable
              with respect to pred_hf through the first three entries (the rest are metrics, formed without a graph as in
              HandTrackNet.compute_loss)
  fits        the four per-cloud rigid fits and the scaled keypoints the entries are formed from
  make_case   every input of ext.HandLosses from (B, per_cloud_palm, seed); get_case caches the table of the GPU tests

Inputs follow tests/test_gpu_train.py::test_fused_hand_losses_match_the_torch_composition: unit-quaternion Rc, scale 0.2,
gt_hf = 0.4 randn, pred = gt + 0.05 randn, init = gt + 0.08 randn -- with the predicted keypoints then turned by a per-cloud
rotation of 5 to 30 degrees, and the palm template drawn on its own (0.08 randn), not copied from cloud 0, whose ground-truth fit
would otherwise be the identity (angle 0).  A cloud is kept only if, in float64,

  (a) every difference under an L1 sign -- pred_s - gt_s, R - R_gt, t - t_gt -- exceeds L1_MIN = 1e-4 in magnitude: float32
      evaluation errors are ~1e-7, so no gradient sign is ambiguous;
  (b) angle(R_gt) and angle(R^T R_gt) lie in [5, 175] degrees: acos is well conditioned (|d acos / dc| <= 1 / sin 5 deg);
  (c) both fits are well posed: the smallest sum of two singular values of the cross-covariance w (the third signed by
      det w) is at least GAP_MIN = 0.01.  The rotation moves by ~|dw| / that sum; the kernel canonicalises the ground truth
      in float32 (errors ~1e-8 per coordinate of 0.08-sized points, |dw| ~ 5e-9), which then stays near 1e-6 and leaves the
      5e-6 bound on the saved fits to the solver (test_hand_loss_cases.py measures that share for every case).

Rejected clouds are redrawn from the same generator; too few survivors after MAX_ROUNDS raises."""
import math
from types import SimpleNamespace

import torch

NAMES = ("hand_pred_kp_loss", "hand_pred_r_loss", "hand_pred_t_loss", "hand_pred_kp_diff", "hand_init_kp_diff",
         "hand_init_r_diff", "hand_init_t_diff", "hand_pred_r_diff", "hand_pred_t_diff")
ANGLE_ENTRIES = (5, 7)           # of the nine; with weights on them the total is an angle entry too
PALM = (0, 1, 5, 9, 13, 17)      # hand_utils.handkp2palmkp
SCALE = 0.2
L1_MIN = 1e-4
ANGLE_MIN, ANGLE_MAX = 5.0, 175.0
GAP_MIN = 1e-2
MAX_ROUNDS = 20
# every entry weighted (the trainer's three loss weights, and the metrics too: out[9] is a plain dot product)
WEIGHTS = (10.0, 1.0, 1.0, 0.5, 0.25, 0.01, 2.0, 0.02, 3.0)

f64 = torch.float64


def quat_to_rot(q):
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)


def axis_angle_to_rot(axis, angle):
    """Rodrigues: axis (B,3) any length, angle (B,) radians."""
    a = axis / axis.norm(dim=1, keepdim=True)
    z = torch.zeros_like(angle)
    K = torch.stack([z, -a[:, 2], a[:, 1], a[:, 2], z, -a[:, 0], -a[:, 1], a[:, 0], z], 1).view(-1, 3, 3)
    s, c = torch.sin(angle)[:, None, None], torch.cos(angle)[:, None, None]
    return torch.eye(3, dtype=axis.dtype) + s * K + (1 - c) * (K @ K)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def kabsch64(x, y):
    """y ~= R x + t for x (1|B, num, 3), y (B, num, 3): the SVD form with the determinant fix-up, as _kabsch_ref of
    tests/test_gpu_fused.py and hand_utils.solve_rot_and_trans, kept in float64 and differentiable.  -> R (B,3,3), t (B,3,1), w"""
    x = x.to(f64).expand(y.shape[0], -1, -1)
    y = y.to(f64)
    cx, cy = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
    w = (x - cx).transpose(1, 2) @ (y - cy)
    u, _, vh = torch.linalg.svd(w)
    v = vh.transpose(1, 2)
    d = torch.det(v @ u.transpose(1, 2))
    fix = torch.eye(3, dtype=f64).repeat(y.shape[0], 1, 1)
    fix[:, 2, 2] = d
    R = v @ fix @ u.transpose(1, 2)
    t = cy - cx @ R.transpose(1, 2)
    return R, t.transpose(1, 2), w


def angle_deg(R):
    """Per-cloud rotation angle in degrees (hand_network._rot_angle_deg without its mean)."""
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    return torch.acos(torch.clamp((tr - 1) / 2, min=-1, max=1)) * (180 / math.pi)


def gap(w):
    """Smallest sum of two singular values of w, the third signed by det w: what the rotation's sensitivity divides by."""
    s = torch.linalg.svdvals(w)
    return s[:, 1] + torch.sign(torch.det(w)) * s[:, 2]


def fits(case, pred_hf=None, gt_s=None):
    """The intermediate quantities of the loss dictionary in float64.  pred_hf (B,3,21) replaces the case's (a leaf that requires
    grad: R and t are then differentiable); gt_s replaces the canonicalised ground truth (the float32 share of precondition c)."""
    s = float(torch.tensor(SCALE, dtype=torch.float32))  # the kernel's float scale, exactly
    Rc, tc = case.Rc.to(f64), case.tc.to(f64)
    if gt_s is None:
        gt_hf = Rc.transpose(1, 2) @ (case.gt_kp.to(f64).transpose(1, 2) - tc) / s   # hand_utils.canonicalize
        gt_s = gt_hf * s
    p = case.pred_hf.to(f64) if pred_hf is None else pred_hf
    pred_s, init_s = p * s, case.init_hf.to(f64) * s
    palm = case.palm.to(f64)
    idx = torch.tensor(PALM)
    R_gt, t_gt, w_gt = kabsch64(palm, gt_s.transpose(1, 2)[:, idx])
    R, t, w = kabsch64(palm, pred_s.transpose(1, 2)[:, idx])
    return SimpleNamespace(s=s, gt_s=gt_s, pred_s=pred_s, init_s=init_s, R=R, t=t, R_gt=R_gt, t_gt=t_gt, w=w, w_gt=w_gt)


def reference(case, pred_hf=None, weights=None):
    """(9,) float64 values in NAMES order (and the weighted total when weights (9,) are given): the expressions of
    HandTrackNet.compute_loss.  Differentiable with respect to pred_hf through entries 0..2."""
    f = fits(case, pred_hf)
    vals = [(f.pred_s - f.gt_s).abs().mean(), (f.R - f.R_gt).abs().mean(), (f.t - f.t_gt).abs().mean()]
    with torch.no_grad():  # the metrics: nothing differentiates them
        vals += [(case.pred_kp.to(f64) - case.gt_kp.to(f64)).norm(dim=2).mean(), (f.init_s - f.gt_s).norm(dim=1).mean(),
                 angle_deg(f.R_gt).mean(), f.t_gt.norm(dim=1).mean(), angle_deg(f.R.transpose(1, 2) @ f.R_gt).mean(),
                 (f.t - f.t_gt).norm(dim=1).mean()]
    vals = torch.stack(vals)
    if weights is None:
        return vals
    return vals, (vals * torch.as_tensor(weights, dtype=f64)).sum()


def fits_of_saved(case):
    """What the kernel's `saved` columns [63:75) and [75:87) hold, in float64: (R | t) and (R_gt | t_gt) per cloud, (B, 12) each."""
    f = fits(case)
    B = f.R.shape[0]
    return torch.cat([f.R.reshape(B, 9), f.t.reshape(B, 3)], 1), torch.cat([f.R_gt.reshape(B, 9), f.t_gt.reshape(B, 3)], 1)


# ---- preconditions -----------------------------------------------------------------------------------------------------------------
def preconditions(case):
    """Per cloud: (smallest |difference| under an L1 sign, angle(R_gt), angle(R^T R_gt), smallest fit gap), float64."""
    f = fits(case)
    B = f.R.shape[0]
    l1 = torch.cat([(f.pred_s - f.gt_s).reshape(B, -1), (f.R - f.R_gt).reshape(B, -1), (f.t - f.t_gt).reshape(B, -1)], 1).abs().amin(1)
    return l1, angle_deg(f.R_gt), angle_deg(f.R.transpose(1, 2) @ f.R_gt), torch.minimum(gap(f.w), gap(f.w_gt))


def valid(case):
    l1, a_gt, a_rel, g = preconditions(case)
    ok = (l1 > L1_MIN) & (g >= GAP_MIN)
    for a in (a_gt, a_rel):
        ok &= (a >= ANGLE_MIN) & (a <= ANGLE_MAX)
    return ok


# ---- cases -------------------------------------------------------------------------------------------------------------------------
_FIELDS = ("Rc", "tc", "gt_kp", "pred_hf", "init_hf", "pred_kp")


def _draw(g, n, palm):
    """n candidate clouds, float32 as the kernel receives them."""
    r = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace()
    c.Rc = quat_to_rot(r(n, 4))
    c.tc = r(n, 3, 1) * 0.1 + torch.tensor([0.0, 0.0, 0.5]).view(1, 3, 1)
    gt_hf = r(n, 3, 21) * 0.4
    c.gt_kp = (SCALE * (c.Rc @ gt_hf) + c.tc).transpose(1, 2).contiguous()
    turn = axis_angle_to_rot(r(n, 3), torch.deg2rad(5 + 25 * torch.rand(n, generator=g)))
    c.pred_hf = (turn @ (gt_hf + 0.05 * r(n, 3, 21))).contiguous()
    c.init_hf = gt_hf + 0.08 * r(n, 3, 21)
    c.pred_kp = (SCALE * (c.Rc @ c.pred_hf) + c.tc).transpose(1, 2).contiguous()
    c.palm = r(n, 6, 3) * 0.4 * SCALE if palm is None else palm
    return c


def make_case(B, per_cloud_palm, seed):
    """Inputs of ext.HandLosses (float32, CPU) for B clouds that all meet the preconditions: Rc (B,3,3), tc (B,3,1), gt_kp
    (B,21,3), pred_hf / init_hf (B,3,21), pred_kp (B,21,3), palm (B,6,3) with rows that differ per cloud or (1,6,3), scale;
    theta_min / theta_max: the smallest and largest of the angles it contains, in degrees."""
    g = torch.Generator().manual_seed(seed)
    shared = None if per_cloud_palm else torch.randn(1, 6, 3, generator=g) * 0.4 * SCALE
    kept = {k: [] for k in _FIELDS + ("palm",)}
    have = 0
    for _ in range(MAX_ROUNDS):
        cand = _draw(g, 2 * B + 8, shared)
        ok = valid(cand)
        for k in _FIELDS:
            kept[k].append(getattr(cand, k)[ok])
        if per_cloud_palm:
            kept["palm"].append(cand.palm[ok])
        have += int(ok.sum())
        if have >= B:
            break
    else:
        raise RuntimeError(f"make_case({B}, {per_cloud_palm}, {seed}): {have} clouds met the preconditions after {MAX_ROUNDS} rounds")
    case = SimpleNamespace(B=B, per_cloud_palm=per_cloud_palm, seed=seed, scale=SCALE, _ref={})
    for k in _FIELDS:
        setattr(case, k, torch.cat(kept[k])[:B].contiguous())
    case.palm = torch.cat(kept["palm"])[:B].contiguous() if per_cloud_palm else shared
    l1, a_gt, a_rel, gp = preconditions(case)
    assert bool(valid(case).all())
    angles = torch.cat([a_gt, a_rel])
    case.theta_min, case.theta_max = float(angles.min()), float(angles.max())
    case.l1_min, case.gap_min = float(l1.min()), float(gp.min())
    return case


# ---- the table of tests/test_gpu_hand_losses.py -------------------------------------------------------------------------------------
SWEEP_B = (1, 2, 127, 128, 129, 256, 300)   # one pass, a full pass, a pass and one cloud, two full passes, two and a partial one
GRAD_B = (1, 129, 300)
IDENTICAL_B = 130
GPU_CASES = tuple((B, pc) for B in SWEEP_B + (IDENTICAL_B,) for pc in (False, True))
_CASES = {}


def seed_of(B, per_cloud_palm):
    return 4000 + 2 * B + int(per_cloud_palm)


def get_case(B, per_cloud_palm):
    key = (B, bool(per_cloud_palm))
    if key not in _CASES:
        _CASES[key] = make_case(B, bool(per_cloud_palm), seed_of(*key))
    return _CASES[key]


def ref_values(case, weights=None):
    """reference(case) as detached float64, computed once per (case, weights) and left unchanged."""
    key = None if weights is None else tuple(weights)
    if key not in case._ref:
        with torch.no_grad():
            case._ref[key] = reference(case, weights=weights)
    return case._ref[key]


def ref_grad(case, g3=None, g_total=None, weights=None):
    """d(sum_i g3[i] out[i] + g_total total) / d pred_hf by autograd through reference -> (B,3,21) float64."""
    p = case.pred_hf.to(f64).requires_grad_(True)
    if weights is None:
        vals, total = reference(case, p), None
    else:
        vals, total = reference(case, p, weights)
    loss = 0.0
    if g3 is not None:
        loss = loss + (vals[:3] * torch.as_tensor(g3, dtype=f64)).sum()
    if g_total is not None:
        loss = loss + g_total * total
    (grad,) = torch.autograd.grad(loss, p)
    return grad


def identical_case():
    """pred_hf = init_hf = the canonicalised ground truth (rounded to float32), pred_kp = gt_kp: outside the preconditions."""
    base = get_case(IDENTICAL_B, False)
    c = SimpleNamespace(**{k: v for k, v in vars(base).items() if k != "_ref"}, _ref={})
    gt_hf = (fits(base).gt_s / fits(base).s).float().contiguous()
    c.pred_hf, c.init_hf, c.pred_kp = gt_hf, gt_hf.clone(), base.gt_kp.clone()
    return c


def angle_bound_deg(case, ref_value):
    """The bound on an angle entry (see tests/test_gpu_hand_losses.py): a cloud's cosine carries at most ~2^-20 absolute float32
    error, its angle 2^-20 / sin(theta) radians with theta the least favourable angle of the case, plus 2e-5 |ref| for the mean."""
    worst_sin = min(math.sin(math.radians(case.theta_min)), math.sin(math.radians(case.theta_max)))
    return math.degrees(2.0 ** -20 / worst_sin) + 2e-5 * abs(ref_value)
