"""CPU: the reference and cases of tests/_hand_loss_cases.py, before tests/test_gpu_hand_losses.py rests on them.
reference is anchored to HandTrackNet.compute_loss's torch composition in float64 (values and the gradient of the weighted
total); every (B, palm form) the GPU tests use is checked to meet the generator's preconditions, and the float32 share of the
saved-fit bound is measured; the reference's gradient is checked against central differences."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
import _hand_loss_cases as C  # noqa: E402
from _netinit import make_cfg  # noqa: E402

f64 = torch.float64


@pytest.fixture(scope="module")
def model():
    from models.hand_network import HandTrackNet
    m = HandTrackNet(make_cfg("cpu"))
    m.use_fused_losses = False
    return m


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("per_cloud_palm", [False, True])
def test_reference_is_compute_loss(model, B, per_cloud_palm):
    """HandTrackNet.compute_loss (torch composition, float64 on the CPU) against reference: the nine values, and the gradient
    of the trainer's weighted total with respect to pred_kp_handframe."""
    case = C.make_case(B, per_cloud_palm, seed=11 + B)
    p = case.pred_hf.to(f64).requires_grad_(True)
    canon = {"scale": torch.tensor([C.SCALE], dtype=torch.float32).to(f64), "rotation": case.Rc.to(f64), "translation": case.tc.to(f64)}
    data = {"gt_hand_kp": case.gt_kp, "gt_hand_pose": {"palm_template": case.palm}}
    ret = {"canon_pose": canon, "pred_kp_handframe": p, "init_kp_handframe": case.init_hf.to(f64), "pred_kp": case.pred_kp.to(f64)}
    flags = {"track_flag": False, "test_flag": False, "save_flag": False, "IKNet_flag": False}
    loss, _ = model.compute_loss(data, ret, flags)
    assert getattr(loss, "fused_values", None) is None and set(loss) == set(C.NAMES)
    assert all(v.dtype == f64 for v in loss.values())
    weights = {"hand_pred_kp_loss": 10.0, "hand_pred_r_loss": 1.0, "hand_pred_t_loss": 1.0}
    (want_grad,) = torch.autograd.grad(sum(loss[k] * w for k, w in weights.items()), p)
    wvec = [weights.get(k, 0.0) for k in C.NAMES]
    vals, total = C.ref_values(case, wvec)
    want = {k: float(v.detach()) for k, v in loss.items()}
    for i, k in enumerate(C.NAMES):
        assert abs(float(vals[i]) - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, float(vals[i]), want[k])
    assert abs(float(total) - sum(want[k] * w for k, w in weights.items())) <= 1e-12
    got_grad = C.ref_grad(case, g_total=1.0, weights=wvec)
    assert float(want_grad.abs().max()) > 1e-4
    assert float((got_grad - want_grad).abs().max()) <= 1e-10 * float(want_grad.abs().max())
    # the same gradient through the first three entries alone
    assert float((C.ref_grad(case, g3=wvec[:3]) - want_grad).abs().max()) <= 1e-10 * float(want_grad.abs().max())


def test_the_table_is_the_one_asked_for():
    assert C.SWEEP_B == (1, 2, 127, 128, 129, 256, 300) and C.GRAD_B == (1, 129, 300) and C.IDENTICAL_B == 130
    assert set(C.GRAD_B) <= set(C.SWEEP_B)
    assert len({C.seed_of(*k) for k in C.GPU_CASES}) == len(C.GPU_CASES)


@pytest.mark.parametrize("B,per_cloud_palm", C.GPU_CASES)
def test_preconditions_hold_for_every_gpu_case(B, per_cloud_palm):
    case = C.get_case(B, per_cloud_palm)
    f32 = torch.float32
    assert case.palm.shape == ((B if per_cloud_palm else 1), 6, 3) and case.pred_hf.shape == (B, 3, 21) == case.init_hf.shape
    assert case.gt_kp.shape == (B, 21, 3) == case.pred_kp.shape and case.Rc.shape == (B, 3, 3) and case.tc.shape == (B, 3, 1)
    assert all(getattr(case, k).dtype == f32 and getattr(case, k).is_contiguous() for k in C._FIELDS + ("palm",))
    if per_cloud_palm and B > 1:  # rows that differ per cloud
        assert float((case.palm[1:] - case.palm[:-1]).abs().amax(dim=(1, 2)).min()) > 1e-3
    l1, a_gt, a_rel, gap = C.preconditions(case)
    print(f"B={B} per_cloud_palm={per_cloud_palm}: min |L1 argument| {float(l1.min()):.2e}, angle(R_gt) in [{float(a_gt.min()):.1f}, "
          f"{float(a_gt.max()):.1f}], angle(R^T R_gt) in [{float(a_rel.min()):.1f}, {float(a_rel.max()):.1f}], min gap {float(gap.min()):.2e}")
    assert float(l1.min()) > C.L1_MIN
    for a in (a_gt, a_rel):
        assert C.ANGLE_MIN <= float(a.min()) and float(a.max()) <= C.ANGLE_MAX
    assert float(gap.min()) >= C.GAP_MIN
    assert case.theta_min == float(torch.cat([a_gt, a_rel]).min()) and case.theta_max == float(torch.cat([a_gt, a_rel]).max())
    assert torch.equal(C.make_case(B, per_cloud_palm, C.seed_of(B, per_cloud_palm)).pred_hf, case.pred_hf)  # deterministic
    # precondition (c) at work: canonicalising the ground truth in float32, as the kernel does, moves the float64 fit by at
    # most half of the 5e-6 the GPU test allows the saved fits -- the other half is the solver's
    s32 = torch.tensor(C.SCALE, dtype=f32)
    gt_s32 = (case.Rc.transpose(1, 2) @ (case.gt_kp.transpose(1, 2) - case.tc) / s32) * s32
    a, b = C.fits(case), C.fits(case, gt_s=gt_s32.to(f64))
    moved = max(float((a.R_gt - b.R_gt).abs().max()), float((a.t_gt - b.t_gt).abs().max()))
    print(f"    float32 canonicalisation moves the ground-truth fit by {moved:.2e}")
    assert moved <= 2.5e-6
    # a float32 evaluation of the signs under the L1 terms agrees with float64 (what (a) is for)
    assert torch.equal(torch.sign(case.pred_hf * s32 - gt_s32), torch.sign(a.pred_s - a.gt_s).float())


def test_identical_case_is_identical():
    c = C.identical_case()
    f = C.fits(c)
    assert c.pred_hf.shape == (C.IDENTICAL_B, 3, 21) and torch.equal(c.pred_hf, c.init_hf) and torch.equal(c.pred_kp, c.gt_kp)
    assert float((f.pred_s - f.gt_s).abs().max()) <= 1e-7  # float32 rounding of the canonicalised ground truth
    vals = C.ref_values(c)
    assert bool(torch.isfinite(vals).all()) and float(vals[:5].max()) <= 1e-6 and float(vals[7]) <= 0.01 and float(vals[8]) <= 1e-6


def test_reference_gradient_matches_central_differences():
    """Autograd through reference (SVD, determinant fix-up) against central differences of the float64 value, on palm and
    non-palm coordinates, for the weighted total and for the rotation term alone."""
    for per_cloud_palm in (False, True):
        case = C.get_case(2, per_cloud_palm)
        wvec = list(C.WEIGHTS)
        for g3, g_total in (((0.0, 1.0, 0.0), None), (None, 1.0), ((0.3, -2.0, 0.7), 0.5)):
            grad = C.ref_grad(case, g3=g3, g_total=g_total, weights=wvec)

            def value(p):
                with torch.no_grad():
                    vals, total = C.reference(case, p, wvec)
                    # the total's metric entries do not depend on p as far as the gradient is concerned: leave them out
                    v = 0.0 if g_total is None else g_total * float((vals[:3] * torch.tensor(wvec[:3], dtype=f64)).sum())
                    return v + (0.0 if g3 is None else float((vals[:3] * torch.tensor(g3, dtype=f64)).sum()))

            h = 1e-6
            for b, c, k in ((0, 0, 0), (1, 2, 5), (0, 1, 17), (1, 0, 13), (0, 2, 3), (1, 1, 20), (0, 0, 10)):  # palm: 0 5 17 13
                p = case.pred_hf.to(f64)
                up, dn = p.clone(), p.clone()
                up[b, c, k] += h
                dn[b, c, k] -= h
                fd = (value(up) - value(dn)) / (2 * h)
                assert abs(fd - float(grad[b, c, k])) <= 1e-6 * max(1.0, float(grad.abs().max())), (per_cloud_palm, g3, g_total, b, c, k, fd, float(grad[b, c, k]))
        assert float(grad[:, :, list(C.PALM)].abs().min()) > 0 and float(grad.abs().max()) > 1e-3
