"""Seeded cases and float64 references for the rigid-fit kernels (hotrack_amd/csrc/kabsch.hip: kabsch_solve, kabsch_backward_one)
across fit conditioning.  CPU tensors, plain torch and numpy: no GPU, no extension import.  tests/test_kabsch_cases.py certifies
the references and the cases, tests/test_gpu_kabsch_fp64.py runs the kernels.

  fit64       the float64 SVD fit with the determinant fix-up (mirrors _hand_loss_cases.kabsch64), differentiable in y
  fit64_horn  an independent float64 route (numpy.linalg.eigh of Horn's 4x4 matrix); it only certifies fit64
  separation  (s2 + sign(det w) s3) / s1 of the cross-covariance w: what the rotation's sensitivity divides by
  restate     the closed-form backward of kabsch.hip's header comment in float64, fed a float32-rounded R: the yardstick the
              backward kernel is held to (it, too, is handed R in float32, and its error scales with 1 / separation)

Every case is a SimpleNamespace(name, x (1|B, num, 3), y (B, num, 3)) of float32 tensors: the inputs are rounded to float32
before any reference sees them.  A group is a list of such cases ("rungs")."""
import math
from types import SimpleNamespace

import numpy as np
import torch

f64 = torch.float64
POINT = 0.05                     # the operating scale: palm points lie ~0.05 m from their centroid
FITS = 32                        # fits per rung
LADDER_E = (1.0, 0.3, 0.1, 0.03, 1e-2, 3e-3, 1e-3, 5e-4, 3e-4, 2e-4, 1e-4, 3e-5)
EXACT_FROM = 2e-4                # every rung from here upward must be certified (fit64 == fit64_horn to CERTIFY) for all its fits
CERTIFY = 1e-8
# the rungs whose float64 references disagree beyond CERTIFY: excluded from the exact comparison, held to the properties of
# a fit without a unique optimum instead (test_kabsch_cases.py asserts that this list is what the references give)
INEXACT = ("ladder e=0.0001", "ladder e=3e-05", "mirror e=0.0001", "mirror e=3e-05")
R_TOL = 2e-6                     # test_kabsch_matches_svd's bound on R and on t
T_TOL = 2e-6
SHAPE_B = (1, 63, 64, 65, 130)   # around the 64-thread workgroup
SHAPE_NUM = (1, 2, 3, 4, 6, 21, 64)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def _cov(x, y):
    x = x.to(f64).expand(y.shape[0], -1, -1)
    y = y.to(f64)
    cx, cy = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
    return x, y, cx, cy, (x - cx).transpose(1, 2) @ (y - cy)


def fit64(x, y):
    """y ~= R x + t for x (1|B, num, 3), y (B, num, 3) -> R (B,3,3), t (B,3,1) in float64, differentiable in y."""
    x, y, cx, cy, w = _cov(x, y)
    u, _, vh = torch.linalg.svd(w)
    v = vh.transpose(1, 2)
    fix = torch.eye(3, dtype=f64).repeat(y.shape[0], 1, 1)
    fix[:, 2, 2] = torch.det(v @ u.transpose(1, 2))
    R = v @ fix @ u.transpose(1, 2)
    return R, (cy - cx @ R.transpose(1, 2)).transpose(1, 2)


def fit64_horn(x, y):
    """The same fit by Horn's unit quaternion: the eigenvector of the largest eigenvalue of the 4x4 matrix, numpy.linalg.eigh."""
    x, y, cx, cy, w = _cov(x, y)
    S = w.numpy()
    N = np.empty((S.shape[0], 4, 4))
    N[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    N[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    N[:, 2, 2] = -S[:, 0, 0] + S[:, 1, 1] - S[:, 2, 2]
    N[:, 3, 3] = -S[:, 0, 0] - S[:, 1, 1] + S[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
    N[:, 2, 3] = N[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    q = torch.from_numpy(np.linalg.eigh(N)[1][:, :, 3].copy())
    a, b, c, d = q.unbind(1)
    R = torch.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c),
                     2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b),
                     2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], 1).view(-1, 3, 3)
    return R, (cy - cx @ R.transpose(1, 2)).transpose(1, 2)


def separation(x, y):
    """(s2 + sign(det w) s3) / s1 per fit, float64; 0 for a vanishing cross-covariance."""
    w = _cov(x, y)[4]
    s = torch.linalg.svdvals(w)
    return (s[:, 1] + torch.sign(torch.det(w)) * s[:, 2]) / s[:, 0].clamp_min(1e-300)


def residual(x, y, R, t):
    """sum_i |R x_i + t - y_i|^2 per fit and the scatter of y it is measured against, float64."""
    x, y = x.to(f64).expand(y.shape[0], -1, -1), y.to(f64)
    r = ((x @ R.to(f64).transpose(1, 2) + t.to(f64).transpose(1, 2) - y) ** 2).sum((1, 2))
    return r, ((y - y.mean(1, keepdim=True)) ** 2).sum((1, 2))


def autograd64(x, y, cR, ct):
    """d(sum cR R + sum ct t) / dy by autograd through fit64 -> (B, num, 3) float64; cR / ct may be None."""
    y64 = y.to(f64).requires_grad_(True)
    R, t = fit64(x, y64)
    loss = (R * 0).sum()
    if cR is not None:
        loss = loss + (R * cR.to(f64)).sum()
    if ct is not None:
        loss = loss + (t * ct.to(f64)).sum()
    return torch.autograd.grad(loss, y64)[0]


def restate(x, y, R, cR, ct):
    """The closed form of kabsch.hip's header comment in float64, for the R it is GIVEN:
    dL/dw = 2 R^T hat(u), u = K^-1 axial((B - B^T) / 2), K = tr(Sym) I - Sym, Sym = sym(R w), B = R G^T, G = dL/dR - dL/dt cx^T,
    dL/dy_i = (x_i - cx)^T dL/dw + dL/dt^T / num."""
    x, y, cx, cy, w = _cov(x, y)
    B, num = y.shape[0], y.shape[1]
    R = R.to(f64)
    gR = torch.zeros(B, 3, 3, dtype=f64) if cR is None else cR.to(f64)
    gt = torch.zeros(B, 3, 1, dtype=f64) if ct is None else ct.to(f64)
    G = gR - gt @ cx
    sym = R @ w
    sym = 0.5 * (sym + sym.transpose(1, 2))
    K = sym.diagonal(dim1=1, dim2=2).sum(1)[:, None, None] * torch.eye(3, dtype=f64) - sym
    Bm = R @ G.transpose(1, 2)
    p = 0.5 * torch.stack([Bm[:, 2, 1] - Bm[:, 1, 2], Bm[:, 0, 2] - Bm[:, 2, 0], Bm[:, 1, 0] - Bm[:, 0, 1]], 1)
    u = torch.linalg.solve(K, p[:, :, None])[:, :, 0]
    z = torch.zeros(B, dtype=f64)
    hat = torch.stack([z, -u[:, 2], u[:, 1], u[:, 2], z, -u[:, 0], -u[:, 1], u[:, 0], z], 1).view(B, 3, 3)
    dW = 2.0 * R.transpose(1, 2) @ hat
    return (x - cx) @ dW + gt.transpose(1, 2) / num


def grad_bound(x, y, cR, ct):
    """(reference gradient, bound, restatement distance): the kernel is held to 4 times the distance of restate -- fed fit64's
    R rounded to float32 -- from float64 autograd, with the floor 2e-5 max(1, |grad|max) of
    test_kabsch_fit_gradient_matches_svd_autograd."""
    ref = autograd64(x, y, cR, ct)
    R32 = fit64(x, y)[0].float()
    dist = float((restate(x, y, R32, cR, ct) - ref).abs().max())
    return ref, max(4.0 * dist, 2e-5 * max(1.0, float(ref.abs().max()))), dist


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def rotations(g, n):
    q = torch.randn(n, 4, generator=g, dtype=f64)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).view(n, 3, 3)


def axis_angle(axis, angle):
    """Rodrigues in float64; exactly 2 a a^T - I at angle pi (no sin(pi) residue)."""
    a = torch.as_tensor(axis, dtype=f64)
    a = a / a.norm()
    if angle == math.pi:
        return 2.0 * torch.outer(a, a) - torch.eye(3, dtype=f64)
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=f64)
    return torch.eye(3, dtype=f64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _case(name, x, y, **kw):
    return SimpleNamespace(name=name, x=x.float().contiguous(), y=y.float().contiguous(), **kw)


def _moved(g, x, noise, t_scale=1.0):
    """R x + t + noise for x (B, num, 3) float64 with a rotation and a translation of its own per fit."""
    B, num = x.shape[0], x.shape[1]
    R = rotations(g, B)
    t = t_scale * torch.randn(B, 1, 3, generator=g, dtype=f64)
    return x @ R.transpose(1, 2) + t + noise * torch.randn(B, num, 3, generator=g, dtype=f64)


def _select(name, x, y, d, fits, e, det_sign):
    """The first `fits` candidates, as float32, whose separation lies within a factor of 3 of d and, from EXACT_FROM upward, whose
    two float64 references agree to CERTIFY / 4 (their own error is ~4e-15 / separation: at 1e-7 some draws are not certified;
    the margin of 4 is for another LAPACK build)."""
    x, y = x.float(), y.float()
    sep = separation(x, y)
    ok = (sep >= d / 3) & (sep <= 3 * d) & (torch.det(_cov(x, y)[4]) * det_sign > 0)
    if e >= EXACT_FROM:
        (R, t), (Rh, th) = fit64(x, y), fit64_horn(x, y)
        ok &= ((R - Rh).abs().amax((1, 2)) <= CERTIFY / 4) & ((t - th).abs().amax((1, 2)) <= CERTIFY / 4)
    keep = torch.nonzero(ok)[:fits, 0]
    if keep.numel() < fits:
        raise RuntimeError(f"{name}: {keep.numel()} of {fits} fits realise the separation {d:g}")
    return _case(name, x[keep], y[keep], e=e, target=d)


def ladder_rung(e, seed=None, fits=FITS):
    """6 points at 0.05 m squeezed by e along two axes of a frame of their own, noise 1e-3 e 0.05: an elongated set whose
    separation scatters around 2 e^2 (0.5 at e = 1); candidates are drawn in bulk and selected by _select."""
    g = torch.Generator().manual_seed(1000 + LADDER_E.index(e) if seed is None else seed)
    n = 16 * fits
    x = POINT * torch.randn(n, 6, 3, generator=g, dtype=f64) * torch.tensor([1.0, e, e], dtype=f64)
    x = x @ rotations(g, n).transpose(1, 2)
    return _select(f"ladder e={e:g}", x, _moved(g, x, 1e-3 * e * POINT), min(2 * e * e, 0.5), fits, e, 1.0)


def mirror_rung(e, seed=None, fits=FITS):
    """A generic set whose target is its mirror image, moved and perturbed: the best ROTATION onto it has separation
    (s2 - s3) / s1.  The scatter of x is given the eigenvalues (1, 0.6, 0.6 - d) POINT^2 with d = min(2 e^2, 0.5), the ladder's
    separation at the same e.  float32 rounding of the inputs alone moves the separation by ~1e-7, so candidates are drawn in
    bulk and selected on the rounded inputs by _select."""
    d = min(2 * e * e, 0.5)
    g = torch.Generator().manual_seed(2000 + LADDER_E.index(e) if seed is None else seed)
    n = (64 if d > 1e-7 else 512) * fits
    p = torch.randn(n, 6, 3, generator=g, dtype=f64)
    p = p - p.mean(1, keepdim=True)
    ev, evec = torch.linalg.eigh(p.transpose(1, 2) @ p)
    p = p @ evec / ev.sqrt()[:, None, :]                                   # scatter = I exactly
    x = POINT * (p * torch.tensor([1.0, 0.6, 0.6 - d], dtype=f64).sqrt()) @ rotations(g, n).transpose(1, 2)
    mirrored = x @ (torch.eye(3, dtype=f64) - 2.0 * evec_mirror(g, n))
    y = _moved(g, mirrored, 0.01 * min(d, 1e-2) * POINT, t_scale=0.1)
    return _select(f"mirror e={e:g}", x, y, d, fits, e, -1.0)


def evec_mirror(g, n):
    """n a a^T for n random unit vectors a: I - 2 a a^T mirrors through the plane across a."""
    a = torch.randn(n, 3, generator=g, dtype=f64)
    a = a / a.norm(dim=1, keepdim=True)
    return a[:, :, None] * a[:, None, :]


ANGLES = (("0", 0.0), ("1e-4 rad", 1e-4), ("90", math.pi / 2), ("179", math.radians(179.0)), ("179.99", math.radians(179.99)),
          ("180", math.pi))
AXES = ((0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (0.3, -0.8, 0.52))


def angle_cases():
    """A generic shared set turned by exactly 0 (y = x + t, no noise), 1e-4 rad, 90, 179, 179.99 and exactly 180 degrees (no noise:
    the quaternion's scalar part is 0) about three axes, one of them a coordinate axis.  One fit per (axis, angle) in one batch;
    case.labels names them, case.noiseless marks the fits without noise."""
    g = torch.Generator().manual_seed(3000)
    x = POINT * torch.randn(1, 6, 3, generator=g, dtype=f64)
    ys, labels, noiseless = [], [], []
    for axis in AXES:
        for label, ang in ANGLES:
            t = torch.randn(1, 3, generator=g, dtype=f64)
            noise = 0.0 if label in ("0", "180") else 1e-3 * POINT
            ys.append(x[0] @ axis_angle(axis, ang).t() + t + noise * torch.randn(6, 3, generator=g, dtype=f64))
            labels.append(f"{label} about {axis}")
            noiseless.append(noise == 0.0)
    return _case("angles", x, torch.stack(ys), labels=labels, noiseless=torch.tensor(noiseless),
                 half_turn=torch.tensor([lb.startswith("180 ") for lb in labels]))


def offset_cases():
    """0.05 m points whose centroid lies 0, 1 and 100 m from the origin (t = cy - R cx: an error in R reaches t times |cx|)."""
    out = []
    for k, off in enumerate((0.0, 1.0, 100.0)):
        g = torch.Generator().manual_seed(3100 + k)
        c = torch.randn(8, 1, 3, generator=g, dtype=f64)
        x = POINT * torch.randn(8, 6, 3, generator=g, dtype=f64) + off * c / c.norm(dim=2, keepdim=True)
        x = x.float().to(f64)                                            # the moved set is what float32 holds of it
        out.append(_case(f"offset {off:g} m", x, _moved(g, x, 1e-3 * POINT, t_scale=0.3)))
    return out


def scale_cases():
    """Centred points of extent 1e-4, 1 and 1e3 m (the cross-covariance spans 28 decades), moved by about 1 m."""
    out = []
    for k, s in enumerate((1e-4, 1.0, 1e3)):
        g = torch.Generator().manual_seed(3200 + k)
        x = s * torch.randn(8, 6, 3, generator=g, dtype=f64)
        x = x - x.mean(1, keepdim=True)
        out.append(_case(f"scale {s:g}", x, _moved(g, x, 1e-3 * s)))      # t ~ 1 m at every scale: float32 holds it to 2e-6
    return out


def planar_case():
    """A palm in a plane (the third singular value of w is noise): well posed, separation ~ s2 / s1."""
    g = torch.Generator().manual_seed(3300)
    x = POINT * torch.randn(FITS, 6, 3, generator=g, dtype=f64) * torch.tensor([1.0, 1.0, 0.0], dtype=f64)
    x = x @ rotations(g, FITS).transpose(1, 2)
    return _case("planar", x, _moved(g, x, 1e-3 * POINT))


def shape_case(B, num, shared):
    g = torch.Generator().manual_seed(5000 + 100 * B + 2 * num + int(shared))
    x = POINT * torch.randn(1 if shared else B, num, 3, generator=g, dtype=f64)
    return _case(f"B={B} num={num} {'shared' if shared else 'per fit'}", x, _moved(g, x.expand(B, -1, -1), 0.04 * POINT),
                 B=B, num=num, shared=shared, unique=num >= 3)


def isolation_case():
    """65 generic fits of which fit 7 is exactly collinear and fit 64 coincident, and the same batch without those two."""
    g = torch.Generator().manual_seed(3400)
    x = POINT * torch.randn(65, 6, 3, generator=g, dtype=f64)
    x[7] = torch.tensor([-1, -0.5, -0.25, 0.25, 0.5, 1], dtype=f64).view(6, 1) * torch.tensor([[2.0 ** -5, 2.0 ** -7, -2.0 ** -6]], dtype=f64)  # exact in float32
    x[64] = 0.1
    x = x.float().to(f64)
    y = _moved(g, x, 0.0)
    y[:, :, :] += 1e-3 * POINT * torch.randn(65, 6, 3, generator=g, dtype=f64) * (x.std(1, keepdim=True).sum(2, keepdim=True) > 0)
    y[7] = x[7] @ rotations(g, 1)[0].t() + 0.3                            # no noise: the image of a line is a line
    y[64] = -0.2
    keep = torch.tensor([i for i in range(65) if i not in (7, 64)])
    return _case("isolation", x, y, keep=keep, degenerate=(7, 64))


# ---- the tables, built once ---------------------------------------------------------------------------------------------------------
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ladder():
    return _once("ladder", lambda: [ladder_rung(e) for e in LADDER_E])


def mirror_ladder():
    return _once("mirror", lambda: [mirror_rung(e) for e in LADDER_E])


def angles():
    return _once("angles", angle_cases)


def offsets_and_scales():
    return _once("offsets", lambda: offset_cases() + scale_cases())


def planar():
    return _once("planar", planar_case)


def shapes():
    return _once("shapes", lambda: [shape_case(B, num, sh) for B in SHAPE_B for num in SHAPE_NUM for sh in (True, False)])


def isolation():
    return _once("isolation", isolation_case)


def exact_cases():
    """Every case the GPU test compares exactly with fit64."""
    return ([c for c in ladder() + mirror_ladder() if c.name not in INEXACT] + [angles()] + offsets_and_scales() + [planar()]
            + [c for c in shapes() if c.unique])


def reference(case):
    """fit64 of a case as detached float64 (R, t), computed once and left unchanged."""
    if not hasattr(case, "_ref"):
        with torch.no_grad():
            case._ref = fit64(case.x, case.y)
    return case._ref


def t_bound(case):
    """T_TOL max(1, |cx|) per fit: t = cy - R cx carries R's error times the template centroid's distance from the origin."""
    cx = case.x.to(f64).mean(1).norm(dim=1).expand(case.y.shape[0])
    return T_TOL * cx.clamp_min(1.0)


def thin_hand_inputs(rung):
    """The inputs of ext.HandLosses and ext.hand_seq_metrics (mode 0) whose two palm fits per cloud are fits of a ladder rung:
    the palm template is the rung's thin set, the predicted palm keypoints are its targets, the ground-truth palm keypoints the
    same template under another motion.  Rc = I, tc = 0 and scale = 1 make the kernels' float32 canonicalisation exact
    ((g * 1 + 0 + 0) / 1 * 1), so the fits see exactly these float32 points.  The relative turn is 20 to 60 degrees and the
    ground-truth turn 30 to 150 degrees: inside the angle columns' [1, 179] degree class."""
    from _hand_loss_cases import PALM, axis_angle_to_rot
    g = torch.Generator().manual_seed(3500 + LADDER_E.index(rung.e))
    B = rung.y.shape[0]
    palm = rung.x.to(f64)
    axis = torch.randn(B, 3, generator=g, dtype=f64)
    Rg = axis_angle_to_rot(axis, torch.deg2rad(30 + 120 * torch.rand(B, generator=g, dtype=f64)))
    Rrel = axis_angle_to_rot(torch.randn(B, 3, generator=g, dtype=f64), torch.deg2rad(20 + 40 * torch.rand(B, generator=g, dtype=f64)))
    noise = lambda: 1e-3 * rung.e * POINT * torch.randn(B, 6, 3, generator=g, dtype=f64)
    tg = 0.3 * torch.randn(B, 1, 3, generator=g, dtype=f64)
    y_gt = palm @ Rg.transpose(1, 2) + tg + noise()
    y_pred = palm @ (Rrel @ Rg).transpose(1, 2) + tg + 0.01 * torch.randn(B, 1, 3, generator=g, dtype=f64) + noise()
    gt_kp = 0.08 * torch.randn(B, 21, 3, generator=g, dtype=f64) + tg
    pred = gt_kp + 0.01 * torch.randn(B, 21, 3, generator=g, dtype=f64)
    idx = torch.tensor(PALM)
    gt_kp[:, idx], pred[:, idx] = y_gt, y_pred
    c = SimpleNamespace(B=B, palm=rung.x.clone(), gt_kp=gt_kp.float().contiguous(), pred_kp=pred.float().contiguous(),
                        pred_hf=pred.float().transpose(1, 2).contiguous(), Rc=torch.eye(3).repeat(B, 1, 1), tc=torch.zeros(B, 3, 1))
    c.init_hf = (c.pred_hf + 0.01 * torch.randn(B, 3, 21, generator=g)).contiguous()
    c.y_gt, c.y_pred = c.gt_kp[:, idx].contiguous(), c.pred_kp[:, idx].contiguous()
    return c
