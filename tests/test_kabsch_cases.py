"""CPU: the cases and float64 references of tests/_kabsch_cases.py, before tests/test_gpu_kabsch_fp64.py holds a kernel to them.

  - every rung of both ladders realises the separation it claims (within a factor of 3 of min(2 e^2, 0.5), on the float32 inputs);
  - fit64 (SVD) and fit64_horn (eigh of Horn's matrix) agree to 1e-8 on every case the GPU test compares exactly; the rungs where
    they do not are exactly INEXACT, all of them below e = 2e-4; every rung from 2e-4 upward keeps all 32 fits;
  - the restatement of the backward's closed form equals float64 autograd when it is given the float64 R: the distances the GPU
    test measures with a float32 R are that rounding's and nothing else's;
  - the constructed angle, offset, planar, shape and isolation cases are what their names say."""
import math

import pytest
import torch

import _kabsch_cases as C


def _disagreement(case):
    (R, t), (Rh, th) = C.fit64(case.x, case.y), C.fit64_horn(case.x, case.y)
    return torch.maximum((R - Rh).abs().amax((1, 2)), (t - th).abs().amax((1, 2)))


@pytest.mark.parametrize("group", ["ladder", "mirror"])
def test_every_rung_realises_its_separation(group):
    rungs = C.ladder() if group == "ladder" else C.mirror_ladder()
    assert [r.e for r in rungs] == list(C.LADDER_E)
    for r in rungs:
        assert r.x.dtype == torch.float32 and r.y.dtype == torch.float32 and r.x.shape == (C.FITS, 6, 3) and r.y.shape == (C.FITS, 6, 3)
        sep = C.separation(r.x, r.y)
        assert r.target == min(2 * r.e * r.e, 0.5)
        assert float(sep.min()) >= r.target / 3 and float(sep.max()) <= 3 * r.target, (r.name, float(sep.min()), float(sep.max()))
        w = C._cov(r.x, r.y)[4]
        assert bool((torch.det(w) * (1 if group == "ladder" else -1) > 0).all()), r.name   # the mirrored targets need the det fix-up
        spread = (r.x - r.x.mean(1, keepdim=True)).norm(dim=2).amax(1)
        assert 0.01 < float(spread.min()) and float(spread.max()) < 0.3, r.name              # the operating scale


def test_the_two_references_agree_wherever_the_gpu_test_compares_exactly():
    worst = 0.0
    for case in C.exact_cases():
        d = float(_disagreement(case).max())
        worst = max(worst, d)
        assert d <= C.CERTIFY, (case.name, d)
    print(f"worst |fit64 - fit64_horn| over the exact cases: {worst:.2e}")


def test_uncertified_rungs_are_the_listed_ones_and_lie_below_the_exact_range():
    found = []
    for r in C.ladder() + C.mirror_ladder():
        d = _disagreement(r)
        if float(d.max()) > C.CERTIFY:
            found.append(r.name)
            assert r.e < C.EXACT_FROM, (r.name, float(d.max()))
        else:
            assert int((d <= C.CERTIFY).sum()) == C.FITS
    assert tuple(found) == C.INEXACT
    assert all(r.name not in C.INEXACT for r in C.ladder() + C.mirror_ladder() if r.e >= C.EXACT_FROM)


def test_restatement_with_the_float64_rotation_is_autograd():
    """restate(R64) against autograd through the SVD: rounding only, growing as 1 / separation."""
    g = torch.Generator().manual_seed(11)
    for case in C.ladder()[:5] + C.mirror_ladder()[:5] + [C.planar(), C.angles(), C.shape_case(65, 3, True), C.shape_case(2, 64, False)]:
        B = case.y.shape[0]
        cR, ct = torch.randn(B, 3, 3, generator=g), torch.randn(B, 3, 1, generator=g)
        for gr, gt in ((cR, ct), (cR, None), (None, ct)):
            ref = C.autograd64(case.x, case.y, gr, gt)
            got = C.restate(case.x, case.y, C.fit64(case.x, case.y)[0], gr, gt)
            sep = float(C.separation(case.x, case.y).min())
            assert float((got - ref).abs().max()) <= 1e-10 / sep * max(1.0, float(ref.abs().max())), case.name
        assert float(C.autograd64(case.x, case.y, None, None).abs().max()) == 0.0
        ref, bound, dist = C.grad_bound(case.x, case.y, cR, ct)
        assert bound >= 2e-5 * max(1.0, float(ref.abs().max())) and bound >= 4 * dist


def test_angle_cases_are_the_angles_they_name():
    c = C.angles()
    R, _ = C.reference(c)
    ang = torch.acos(((R.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1))
    assert len(c.labels) == len(C.AXES) * len(C.ANGLES) == c.y.shape[0] and c.x.shape[0] == 1
    for i, lb in enumerate(c.labels):
        want = dict(C.ANGLES)[lb.split(" about ")[0]]
        assert abs(float(ang[i]) - want) < 5e-3, (lb, float(ang[i]))   # the noise of 1e-3 of the extent turns the fit by ~1e-3 rad
    # exactly 0 and exactly 180 degrees carry no noise beyond float32 rounding of y: the fit is the constructed rotation to ~1e-6
    q0 = torch.sqrt((1 + R.diagonal(dim1=1, dim2=2).sum(1)).clamp_min(0)) / 2
    assert float(q0[c.half_turn].max()) < 1e-5 and int(c.half_turn.sum()) == 3 and int(c.noiseless.sum()) == 6
    assert any(sorted(a) == [0.0, 0.0, 1.0] for a in C.AXES)


def test_offset_scale_planar_shape_and_isolation_cases():
    offs = C.offsets_and_scales()
    assert [c.name for c in offs] == ["offset 0 m", "offset 1 m", "offset 100 m", "scale 0.0001", "scale 1", "scale 1000"]
    for c, want in zip(offs[:3], (0.0, 1.0, 100.0)):
        cx = c.x.double().mean(1).norm(dim=1)
        assert float((cx - want).abs().max()) < 0.1
        assert float(C.t_bound(c).max()) <= C.T_TOL * max(1.0, want + 0.1) and float(C.t_bound(c).min()) >= C.T_TOL
    for c, s in zip(offs[3:], (1e-4, 1.0, 1e3)):
        ext = (c.x - c.x.mean(1, keepdim=True)).norm(dim=2).amax(1)
        assert 0.5 * s < float(ext.min()) and float(ext.max()) < 5 * s
    p = C.planar()
    assert float(torch.linalg.svdvals(p.x.double() - p.x.double().mean(1, keepdim=True))[:, 2].max()) < 1e-8
    assert float(C.separation(p.x, p.y).min()) > 1e-2
    sh = C.shapes()
    assert {(c.B, c.num, c.shared) for c in sh} == {(B, n, s) for B in C.SHAPE_B for n in C.SHAPE_NUM for s in (True, False)}
    for c in sh:
        assert c.x.shape == (1 if c.shared else c.B, c.num, 3) and c.y.shape == (c.B, c.num, 3) and c.unique == (c.num >= 3)
        if c.unique:
            assert float(C.separation(c.x, c.y).min()) > 1e-4, c.name   # (three random points can lie close to a line)
    iso = C.isolation()
    assert iso.y.shape == (65, 6, 3) and iso.keep.numel() == 63 and iso.degenerate == (7, 64)
    xc = iso.x.double() - iso.x.double().mean(1, keepdim=True)
    sv = torch.linalg.svdvals(xc)
    assert float(sv[7, 1]) < 1e-8 * float(sv[7, 0]) and float(sv[64, 0]) == 0.0
    assert float(sv[iso.keep][:, 2].min()) > 1e-3
    assert math.isfinite(float(iso.y.abs().max()))


def test_thin_hand_inputs_carry_the_rungs_fits():
    from _hand_loss_cases import PALM, angle_deg
    for rung in (C.ladder()[0], C.ladder()[4], C.ladder()[6]):
        h = C.thin_hand_inputs(rung)
        idx = torch.tensor(PALM)
        assert torch.equal(h.pred_hf.transpose(1, 2)[:, idx], h.y_pred) and torch.equal(h.gt_kp[:, idx], h.y_gt)
        assert torch.equal(h.palm, rung.x)
        (R, _), (Rg, _) = C.fit64(h.palm, h.y_pred), C.fit64(h.palm, h.y_gt)
        for a in (angle_deg(Rg), angle_deg(R.transpose(1, 2) @ Rg)):
            assert 1.0 <= float(a.min()) and float(a.max()) <= 179.0
        for y in (h.y_pred, h.y_gt):
            sep = C.separation(h.palm, y)
            assert float(sep.min()) >= rung.target / 10 and float(sep.max()) <= 10 * rung.target
            assert float(_disagreement_xy(h.palm, y).max()) <= C.CERTIFY


def _disagreement_xy(x, y):
    (R, t), (Rh, th) = C.fit64(x, y), C.fit64_horn(x, y)
    return torch.maximum((R - Rh).abs().amax((1, 2)), (t - th).abs().amax((1, 2)))
