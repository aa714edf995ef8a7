"""GPU: ext.HandLosses (hotrack_amd/csrc/kabsch.hip: hand_loss_fwd_kernel, hand_loss_bwd_kernel) against the float64 reference
of tests/_hand_loss_cases.py (anchored to HandTrackNet.compute_loss by tests/test_hand_loss_cases.py): across the forward's
passes of 128 clouds (a full pass, a pass and one cloud, two full passes, two and a partial one), with the shared (1,6,3) and
the per-cloud (B,6,3) palm template, with and without the in-kernel weighted total, the per-cloud fits it saves for the
backward, every way of driving the backward, identical prediction and ground truth, and replay from a captured graph.

Bounds.  The seven entries that are no angles: |a - ref| <= 2e-5 max(1, |ref|), the bound of
test_gpu_train.py::test_fused_hand_losses_match_the_torch_composition.  The angle entries (hand_init_r_diff, hand_pred_r_diff
and the weighted total, which sums them with weights <= 0.02): the kernel forms a cloud's cosine (tr - 1) / 2 in float32 from
nine products of float32-rounded matrix entries, halved: at most about 2^-20 absolute error.  acos turns an error dc of the
cosine into dc / sin(theta) radians, and the generator keeps every angle within [5, 175] degrees, so a cloud's angle is off by at
most 2^-20 / sin(theta*) radians with theta* the least favourable angle the case contains; in degrees, plus 2e-5 |ref| for the
float32 mean over the clouds: _hand_loss_cases.angle_bound_deg.  At theta* = 5 degrees that is 6.3e-4 degrees + 2e-5 |ref|.
The saved fits: 5e-6 absolute, what test_kabsch_degenerate_and_ill_separated_fits allows well-posed fits (the generator's
precondition (c) makes them so).  The gradient: max |a - ref| <= 2e-5 max |ref| + 1e-7, as in the existing test."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_loss_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
ANGLE = set(C.ANGLE_ENTRIES)


def _inputs(case, weights):
    d = lambda t: t.cuda()
    p = d(case.pred_hf).requires_grad_(True)
    w = None if weights is None else torch.tensor(weights, dtype=torch.float32, device="cuda")
    return p, (d(case.init_hf), d(case.gt_kp), d(case.pred_kp), d(case.Rc), d(case.tc).reshape(-1, 3), case.scale, d(case.palm), w)


def _apply(ext, case, weights):
    """-> (pred_hf leaf, out (9,), total | None)"""
    p, rest = _inputs(case, weights)
    res = ext.HandLosses.apply(p, *rest)
    out, total = res if weights is not None else (res, None)
    assert out.shape == (9,) and out.dtype == torch.float32
    return p, out, total


def _check_values(case, out, total, weights, what):
    ref = C.ref_values(case, weights)
    ref_vals, ref_total = ref if weights is not None else (ref, None)
    got = out.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), (what, got)
    for i, name in enumerate(C.NAMES):
        a, r = float(got[i]), float(ref_vals[i])
        bound = C.angle_bound_deg(case, r) if i in ANGLE else 2e-5 * max(1.0, abs(r))
        print(f"{what} {name}: {a:.7g} vs {r:.7g}, |diff| {abs(a - r):.2e} of {bound:.2e}")
        assert abs(a - r) <= bound, (what, name, a, r, abs(a - r), bound)
    if weights is not None:
        a, r = float(total.detach()), float(ref_total)
        bound = C.angle_bound_deg(case, r)
        print(f"{what} weighted total: {a:.7g} vs {r:.7g}, |diff| {abs(a - r):.2e} of {bound:.2e}")
        assert abs(a - r) <= bound, (what, "total", a, r, abs(a - r), bound)


@pytest.mark.parametrize("with_weights", [False, True])
@pytest.mark.parametrize("per_cloud_palm", [False, True])
@pytest.mark.parametrize("B", C.SWEEP_B)
def test_values_and_saved_fits_match_fp64(B, per_cloud_palm, with_weights):
    from hotrack_amd import ext
    assert tuple(ext.HAND_LOSS_NAMES) == C.NAMES
    case = C.get_case(B, per_cloud_palm)
    weights = C.WEIGHTS if with_weights else None
    what = f"B={B} palm={'B' if per_cloud_palm else 1} weights={with_weights}:"
    p, out, total = _apply(ext, case, weights)
    _check_values(case, out, total, weights, what)
    # the per-cloud fits the forward saves for the backward, EVERY cloud: a pass that writes another cloud's fit shows at b >= 128
    saved = out.grad_fn.saved_tensors[2]
    assert saved.shape == (B, 87)
    saved = saved.cpu().double()
    fit_pred, fit_gt = C.fits_of_saved(case)
    for name, got, ref in (("(R | t)", saved[:, 63:75], fit_pred), ("(R_gt | t_gt)", saved[:, 75:87], fit_gt)):
        err = (got - ref).abs().amax(1)
        print(f"{what} saved {name}: worst |diff| {float(err.max()):.2e} at cloud {int(err.argmax())}")
        assert float(err.max()) <= 5e-6, (what, name, float(err.max()), int(err.argmax()))
    gt_s = C.fits(case).gt_s.reshape(B, 63)  # [0:63): the scaled canonical ground truth, channel-major
    assert float((saved[:, :63] - gt_s).abs().max()) <= 2e-6


@pytest.mark.parametrize("mode", ["grad3", "total", "both"])
@pytest.mark.parametrize("per_cloud_palm", [False, True])
@pytest.mark.parametrize("B", C.GRAD_B)
def test_gradient_matches_autograd_through_fp64(B, per_cloud_palm, mode):
    """The three ways of driving the backward: a gradient on the first three outputs only, on the weighted total only, and on
    both at once (g_i = grad[i] + grad_total w[i])."""
    from hotrack_amd import ext
    case = C.get_case(B, per_cloud_palm)
    g3 = (0.7, -1.3, 2.1)
    g_total = 0.6
    p, out, total = _apply(ext, case, C.WEIGHTS)
    dev3 = torch.tensor(g3, device="cuda")
    if mode == "grad3":
        loss, ref = (out[:3] * dev3).sum(), C.ref_grad(case, g3=g3)
    elif mode == "total":
        loss, ref = g_total * total, C.ref_grad(case, g_total=g_total, weights=C.WEIGHTS)
    else:
        loss, ref = (out[:3] * dev3).sum() + g_total * total, C.ref_grad(case, g3=g3, g_total=g_total, weights=C.WEIGHTS)
    (got,) = torch.autograd.grad(loss, p)
    assert got.shape == (B, 3, 21)
    err = (got.cpu().double() - ref).abs()
    bound = 2e-5 * float(ref.abs().max()) + 1e-7
    print(f"B={B} palm={'B' if per_cloud_palm else 1} {mode}: max |d_pred_hf - ref| {float(err.max()):.2e} of {bound:.2e} "
          f"(cloud {int(err.amax(dim=(1, 2)).argmax())}), max |ref| {float(ref.abs().max()):.3e}")
    assert float(err.max()) <= bound, (float(err.max()), bound, int(err.amax(dim=(1, 2)).argmax()))
    # per cloud as well: the largest gradient of the batch must not hide a wrong cloud with a small one
    per_cloud = ref.abs().amax(dim=(1, 2))
    worst = (err.amax(dim=(1, 2)) / (2e-5 * per_cloud + 1e-7))
    assert float(worst.max()) <= 1.0, (float(worst.max()), int(worst.argmax()))


@pytest.mark.parametrize("per_cloud_palm", [False, True])
def test_the_metric_entries_carry_no_gradient(per_cloud_palm):
    from hotrack_amd import ext
    case = C.get_case(129, per_cloud_palm)
    for weights in (None, C.WEIGHTS):
        p, out, total = _apply(ext, case, weights)
        (g,) = torch.autograd.grad(out[3:].sum(), p, allow_unused=True)
        assert g is None or float(g.abs().max()) == 0.0


def test_identical_prediction_and_ground_truth():
    """pred_hf = the canonicalised ground truth: every L1 argument and both relative poses are at float32 round-off, outside
    the generator's preconditions.  hand_pred_r_diff: the cosine error bound 2^-20 at theta = 0, acos(1 - 2^-20) = 0.079 deg."""
    from hotrack_amd import ext
    case = C.identical_case()
    p, out, total = _apply(ext, case, C.WEIGHTS)
    got = out.detach().cpu().double()
    print("identical:", {n: float(v) for n, v in zip(C.NAMES, got)}, float(total.detach()))
    assert bool(torch.isfinite(got).all()) and math.isfinite(float(total.detach()))
    for i in (0, 1, 2, 3, 4):
        assert float(got[i]) <= 1e-6, (C.NAMES[i], float(got[i]))
    assert 0.0 <= float(got[7]) <= math.degrees(math.acos(1 - 2.0 ** -20)), float(got[7])
    assert float(got[8]) <= 1e-6
    ref = C.ref_values(case)
    assert abs(float(got[5]) - float(ref[5])) <= C.angle_bound_deg(case, float(ref[5]))  # the ground-truth fit is an ordinary one
    (g,) = torch.autograd.grad(total, p)
    assert bool(torch.isfinite(g).all())


def test_replay_from_a_captured_graph():
    """Forward and backward captured at B = 300 and replayed twice.  The forward ends in LDS float atomics, so its values are held
    to the tolerances, not to bit equality; d_pred_hf depends on the forward only through `saved`, which one thread per fit
    writes, and the backward has no atomics: bit-equal between replays and to the eager run."""
    from hotrack_amd import ext
    case = C.get_case(300, True)
    weights = C.WEIGHTS
    p, rest = _inputs(case, weights)
    out_e, total_e = ext.HandLosses.apply(p, *rest)
    (d_e,) = torch.autograd.grad(total_e, p)
    out_e, total_e, d_e = out_e.detach().clone(), total_e.detach().clone(), d_e.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o, t = ext.HandLosses.apply(p, *rest)
        torch.autograd.grad(t, p)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out_g, total_g = ext.HandLosses.apply(p, *rest)
            (d_g,) = torch.autograd.grad(total_g, p)
    torch.cuda.current_stream().wait_stream(side)
    runs = []
    for _ in range(2):
        out_g.detach().zero_()
        d_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        runs.append((out_g.detach().clone(), total_g.detach().clone(), d_g.clone()))
    for i, (o, t, d) in enumerate(runs):
        _check_values(case, o, t, weights, f"replay {i}:")
        assert torch.equal(d, d_e), f"replay {i}: d_pred_hf differs from the eager run"
    assert torch.equal(runs[0][2], runs[1][2])
    assert float(runs[0][2].abs().max()) > 0
    _check_values(case, out_e, total_e, weights, "eager:")
