"""GPU: the rigid-fit kernels (hotrack_amd/csrc/kabsch.hip: kabsch_solve, kabsch_backward_one) against float64 across fit
conditioning -- between the generic fits and the exactly degenerate ones the suite already had, where the fast path (Newton root +
adjugate column) hands over to the Jacobi sweep.  Cases and references: tests/_kabsch_cases.py, certified on the CPU by
tests/test_kabsch_cases.py.

Forward (ext.kabsch, and the same solver inside ext.hand_frame, ext.HandLosses, ext.hand_seq_metrics mode 0).  Against fit64 of
the same float32 inputs: |R - ref| <= 2e-6 and |t - ref| <= 2e-6 max(1, |cx|) (test_kabsch_matches_svd's bound; t = cy - R cx
carries R's error times |cx|), always |R R^T - I| < 1e-5, |det R - 1| < 1e-5, finite.  Rungs the two float64 references do not
certify (_kabsch_cases.INEXACT, all below e = 2e-4) and fits of 1 or 2 points are held to a proper rotation and the optimum's
residual, as test_kabsch_degenerate_and_ill_separated_fits does.  hand_frame: R, t bit-equal to ext.kabsch, xyz1 / xyz2 at
2e-6 max(1, |ref|) (test_gpu_hand_frame.py); HandLosses' saved fits 5e-6 (test_gpu_hand_losses.py); hand_seq_metrics columns 5
and 7: 5e-3 degrees for angles in [1, 179] degrees (test_gpu_hand_seq_eval.py).

With the hand-over threshold the kernel had before these tests (best > 1e-12 lambda^6) a CPU build of kabsch_solve gave, per
ladder rung, worst |R - ref| and fits beyond 2e-6 of 32:  e=3e-3 3.2e-7 (0) | 1e-3 3.0e-5 (9) | 5e-4 3.8e-4 (17) |
3e-4 2.2e-4 (13) | 2e-4 2.1e-4 (6); mirrored: 1e-3 2.0e-5 (11) | 5e-4 4.1e-4 (31) | 3e-4 1.2e-4 (4).  With 1e-7: <= 1.7e-9 on
every fit the fast path keeps, <= 1.3e-8 on every certified rung.

Backward (ext.kabsch_backward, ext.KabschFit).  Against float64 autograd through fit64.  The kernel is handed R in float32 and
the gradient scales with 1 / separation, so the bound is measured, not fixed: 4 times the distance from autograd of the
closed form restated in float64 and fed fit64's R rounded to float32 (_kabsch_cases.restate), floor 2e-5 max(1, |grad|max)
(test_kabsch_fit_gradient_matches_svd_autograd).  Restatement distances measured with the seeds of this file (both gradients
given), worst over the fits of a rung, and |grad|max:
    ladder  e=1 6.9e-07 (24) | 0.3 2.2e-06 (49)  | 0.1 1.5e-05 (1.5e2) | 0.03 1.9e-04 (4.0e2) | 0.01 1.6e-03 (1.7e3)
    mirror  e=1 2.2e-06 (84) | 0.3 2.0e-05 (1.6e2) | 0.1 1.5e-03 (1.5e3) | 0.03 1.8e-01 (2.5e4) | 0.01 1.4e+01 (1.9e5)
    planar 1.4e-06 (63) | angles 4.9e-07 (16) | shapes <= 1.0e-04 (B=130 num=3 per fit, |grad|max 4.3e2: three points near a line)
    with grad_t alone: <= 5.1e-07 on the ladder, <= 1.8e-09 on the mirrored ladder (|grad|max ~ 1: the floor 2e-5 decides)
The floor decides on the ladder (2e-5 * 1.7e3 = 3.5e-2 against 4 * 1.6e-3 at e = 0.01); 4 times the measured distance decides
on the mirrored ladder from e = 0.03 down, where (s2 - s3) / s1 shrinks while |grad| grows as its inverse.

Isolation and repeatability: bit equality."""
import pytest
import torch

import _kabsch_cases as C

pytestmark = pytest.mark.gpu
f64 = torch.float64


def _run(case):
    from hotrack_amd import ext
    R, t = ext.kabsch(case.x.cuda(), case.y.cuda())
    return R.cpu(), t.cpu()


def _proper(R, t, what):
    R = R.double()
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all()), what
    orth = float((R @ R.transpose(1, 2) - torch.eye(3, dtype=f64)).abs().max())
    det = float((torch.det(R) - 1).abs().max())
    assert orth < 1e-5 and det < 1e-5, (what, orth, det)


def _forward_failures(case, R, t):
    """[] or one line naming the case's worst errors and how many fits exceed the bounds."""
    _proper(R, t, case.name)
    if case.name in C.INEXACT or not getattr(case, "unique", True):
        Rr, tr = C.reference(case)
        got, scat = C.residual(case.x, case.y, R, t)
        ref, _ = C.residual(case.x, case.y, Rr, tr)
        bad = got > ref + 1e-6 * scat + 1e-12         # the allowance of test_kabsch_degenerate_and_ill_separated_fits
        return [f"{case.name}: residual above the optimum's on {int(bad.sum())} fits"] if bool(bad.any()) else []
    Rr, tr = C.reference(case)
    eR = (R.double() - Rr).abs().amax((1, 2))
    et = (t.double() - tr).abs().amax((1, 2))
    nR, nt = int((eR > C.R_TOL).sum()), int((et > C.t_bound(case)).sum())
    line = f"{case.name}: worst |R - ref| {float(eR.max()):.2e} ({nR} of {eR.numel()} fits beyond {C.R_TOL:g}), worst |t - ref| {float(et.max()):.2e} ({nt} beyond)"
    print(line)
    return [line] if nR or nt else []


@pytest.mark.parametrize("group", ["ladder", "mirror", "angles", "offsets and scales", "planar"])
def test_forward_matches_fp64_across_conditioning(group):
    cases = {"ladder": C.ladder, "mirror": C.mirror_ladder, "angles": lambda: [C.angles()], "offsets and scales": C.offsets_and_scales,
             "planar": lambda: [C.planar()]}[group]()
    failures = []
    for case in cases:
        failures += _forward_failures(case, *_run(case))
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("B", C.SHAPE_B)
def test_forward_shapes(B):
    failures = []
    for case in C.shapes():
        if case.B == B:
            R, t = _run(case)
            assert R.shape == (B, 3, 3) and t.shape == (B, 3, 1)
            failures += _forward_failures(case, R, t)
    assert not failures, "\n" + "\n".join(failures)


# ---- the other consumers of kabsch_solve ---------------------------------------------------------------------------------------------
def _frame_inputs(case, seed, J=21, N=300):
    """Keypoints whose rows palm_idx are the case's targets, and a cloud around them."""
    g = torch.Generator().manual_seed(seed)
    B, num = case.y.shape[0], case.y.shape[1]
    palm_idx = torch.randperm(J, generator=g)[:num]
    centre = case.y.mean(1, keepdim=True)
    kp = centre + 0.08 * torch.randn(B, J, 3, generator=g)
    kp[:, palm_idx] = case.y
    pts = centre + 0.1 * torch.randn(B, N, 3, generator=g)
    return kp.contiguous(), palm_idx.int(), pts.contiguous()


@pytest.mark.parametrize("group", ["ladder", "angles"])
def test_hand_frame_is_the_same_fit_and_canonicalises_with_it(group):
    from hotrack_amd import ext
    scale = 0.2
    s = float(torch.tensor(scale, dtype=torch.float32))
    for k, case in enumerate(C.ladder() if group == "ladder" else [C.angles()]):
        kp, palm_idx, pts = _frame_inputs(case, 4000 + k)
        R, t, xyz2, xyz1 = ext.hand_frame(case.x.cuda(), kp.cuda(), palm_idx.cuda(), pts.cuda(), scale)
        R2, t2 = ext.kabsch(case.x.cuda(), case.y.cuda())
        assert torch.equal(R, R2) and torch.equal(t, t2), case.name
        for name, got, src in (("xyz2", xyz2, pts), ("xyz1", xyz1, kp)):
            ref = (src.double() - t.cpu().double().transpose(1, 2)) @ R.cpu().double() / s
            err, bound = float((got.cpu().double() - ref).abs().max()), 2e-6 * max(1.0, float(ref.abs().max()))
            assert err <= bound, (case.name, name, err, bound)


@pytest.mark.parametrize("e", [1.0, 1e-2, 1e-3])
def test_hand_losses_and_seq_metrics_fit_a_thin_palm(e):
    from hotrack_amd import ext
    from _hand_loss_cases import angle_deg
    rung = C.ladder()[C.LADDER_E.index(e)]
    h = C.thin_hand_inputs(rung)
    B = h.B
    (R, t), (Rg, tg) = C.fit64(h.palm, h.y_pred), C.fit64(h.palm, h.y_gt)
    pred_hf = h.pred_hf.cuda().requires_grad_(True)
    out = ext.HandLosses.apply(pred_hf, h.init_hf.cuda(), h.gt_kp.cuda(), h.pred_kp.cuda(), h.Rc.cuda(), h.tc.cuda(), 1.0, h.palm.cuda())
    saved = out.grad_fn.saved_tensors[2].cpu().double()
    assert torch.equal(saved[:, :63].float(), h.gt_kp.transpose(1, 2).reshape(B, 63))          # scale 1, Rc = I, tc = 0: exact
    for name, got, ref in (("(R | t)", saved[:, 63:75], torch.cat([R.reshape(B, 9), t.reshape(B, 3)], 1)),
                           ("(R_gt | t_gt)", saved[:, 75:87], torch.cat([Rg.reshape(B, 9), tg.reshape(B, 3)], 1))):
        err = (got - ref).abs().amax(1)
        print(f"e={e:g} saved {name}: worst |diff| {float(err.max()):.2e}, {int((err > 5e-6).sum())} of {B} beyond 5e-6")
        assert float(err.max()) <= 5e-6, (name, float(err.max()), int((err > 5e-6).sum()))
    rows, _, mask = ext.hand_seq_metrics(h.pred_hf.cuda(), h.init_hf.cuda(), h.gt_kp.cuda(), h.pred_kp.cuda(), h.Rc.cuda(),
                                         h.tc.view(B, 3).contiguous().cuda(), torch.ones(B).cuda(), list(range(B + 1)), palm=h.palm.cuda())
    assert mask & 0xa0 == 0xa0
    rows = rows.cpu().double()
    for col, ref in ((5, angle_deg(Rg)), (7, angle_deg(R.transpose(1, 2) @ Rg))):
        assert 1.0 <= float(ref.min()) and float(ref.max()) <= 179.0
        err = (rows[:, col] - ref).abs()
        print(f"e={e:g} column {col}: worst |diff| {float(err.max()):.2e} degrees")
        assert float(err.max()) <= 5e-3, (col, float(err.max()), int((err > 5e-3).sum()))


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def _backward_cases():
    return C.ladder()[:5] + C.mirror_ladder()[:5] + [C.planar(), C.angles()] + [c for c in C.shapes() if c.unique]


def _backward_failures(case, k):
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(6000 + k)
    B = case.y.shape[0]
    cR, ct = torch.randn(B, 3, 3, generator=g), torch.randn(B, 3, 1, generator=g)
    rows = torch.ones(B, dtype=torch.bool)
    if hasattr(case, "half_turn"):
        rows = ~case.half_turn                       # exactly 180 degrees with zero noise is not compared
    x, y = case.x.cuda(), case.y.cuda()
    R, _ = ext.kabsch(x, y)
    out = []
    for what, gr, gt in (("both", cR, ct), ("grad_R", cR, None), ("grad_t", None, ct)):
        ref, bound, dist = C.grad_bound(case.x[rows] if case.x.shape[0] == B else case.x, case.y[rows],
                                        None if gr is None else gr[rows], None if gt is None else gt[rows])
        dy = ext.kabsch_backward(x, y, R, None if gr is None else gr.cuda(), None if gt is None else gt.cuda()).cpu()
        assert bool(torch.isfinite(dy).all()), (case.name, what)
        err = float((dy[rows].double() - ref).abs().max())
        line = f"{case.name} {what}: |dy - autograd| {err:.2e} of {bound:.2e} (restatement {dist:.2e}, |grad|max {float(ref.abs().max()):.2e})"
        print(line)
        if err > bound:
            out.append(line)
        if what == "both":                           # the autograd Function is the same two launches
            yg = y.clone().requires_grad_(True)
            Rf, tf = ext.KabschFit.apply(x, yg)
            ((Rf * cR.cuda()).sum() + (tf * ct.cuda()).sum()).backward()
            assert torch.equal(Rf.detach(), R) and torch.equal(yg.grad.cpu(), dy), case.name
        elif what == "grad_R":                       # the other gradient arrives as None
            yg = y.clone().requires_grad_(True)
            (ext.KabschFit.apply(x, yg)[0] * cR.cuda()).sum().backward()
            assert torch.equal(yg.grad.cpu(), dy), case.name
    zero = ext.kabsch_backward(x, y, R, None, None)
    assert float(zero.abs().max()) == 0.0, case.name
    return out


@pytest.mark.parametrize("group", ["ladder", "mirror", "planar and angles", "shapes"])
def test_backward_matches_fp64_autograd(group):
    cases = _backward_cases()
    pick = {"ladder": lambda c: c.name.startswith("ladder"), "mirror": lambda c: c.name.startswith("mirror"),
            "planar and angles": lambda c: c.name in ("planar", "angles"), "shapes": lambda c: c.name.startswith("B=")}[group]
    failures = []
    for k, case in enumerate(cases):
        if pick(case):
            failures += _backward_failures(case, k)
    assert not failures, "\n" + "\n".join(failures)


# ---- isolation and repeatability -------------------------------------------------------------------------------------------------------
def test_degenerate_fits_leave_the_rest_of_the_batch_alone():
    """Fit 7 is exactly collinear and fit 64 coincident (across the 64-thread boundary).  Every other fit's R, t and dy are, bit for
    bit, those of the batch without the two.  The degenerate fits get a finite proper rotation, and for dy what include/pn2_ext.h
    promises of a singular K: the translation term grad_t / num alone, zeros without grad_t -- never Inf or NaN."""
    from hotrack_amd import ext
    c = C.isolation()
    g = torch.Generator().manual_seed(6100)
    cR, ct = torch.randn(65, 3, 3, generator=g), torch.randn(65, 3, 1, generator=g)
    keep, deg = c.keep, torch.tensor(c.degenerate)
    x, y = c.x.cuda(), c.y.cuda()
    R, t = ext.kabsch(x, y)
    dy = ext.kabsch_backward(x, y, R, cR.cuda(), ct.cuda())
    dy_R = ext.kabsch_backward(x, y, R, cR.cuda(), None)
    xk, yk = c.x[keep].contiguous().cuda(), c.y[keep].contiguous().cuda()
    Rk, tk = ext.kabsch(xk, yk)
    dyk = ext.kabsch_backward(xk, yk, Rk, cR[keep].contiguous().cuda(), ct[keep].contiguous().cuda())
    assert torch.equal(R.cpu()[keep], Rk.cpu()) and torch.equal(t.cpu()[keep], tk.cpu()) and torch.equal(dy.cpu()[keep], dyk.cpu())
    ref, bound, _ = C.grad_bound(c.x[keep], c.y[keep], cR[keep], ct[keep])          # and they are right
    assert float((dyk.cpu().double() - ref).abs().max()) <= bound
    _proper(R.cpu()[deg], t.cpu()[deg], "degenerate fits")
    want = (ct[deg].transpose(1, 2) / 6.0).expand(-1, 6, -1)
    assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(dy_R).all())
    assert float((dy.cpu()[deg] - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float(dy_R.cpu()[deg].abs().max()) == 0.0


def test_two_runs_are_bitwise_equal():
    from hotrack_amd import ext
    rungs = C.ladder()
    x, y = torch.cat([r.x for r in rungs]).cuda(), torch.cat([r.y for r in rungs]).cuda()
    g = torch.Generator().manual_seed(6200)
    cR, ct = torch.randn(y.shape[0], 3, 3, generator=g).cuda(), torch.randn(y.shape[0], 3, 1, generator=g).cuda()
    runs = []
    for _ in range(2):
        R, t = ext.kabsch(x, y)
        runs.append((R, t, ext.kabsch_backward(x, y, R, cR, ct)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    for k, r in enumerate(rungs):                    # and a fit does not depend on its place in the batch
        Rr, tr = ext.kabsch(r.x.cuda(), r.y.cuda())
        assert torch.equal(Rr, runs[0][0][k * C.FITS:(k + 1) * C.FITS]) and torch.equal(tr, runs[0][1][k * C.FITS:(k + 1) * C.FITS])
