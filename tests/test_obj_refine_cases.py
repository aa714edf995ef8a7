"""CPU: the Gauss-Newton pose refinement's rule, checked on its numpy restatements (tests/_obj_refine_cases.py) and on the torch route
(network/models/pose_refine.py): the Jacobian against finite differences, convergence on an exact volume, the unobservable
direction of the capsule, the monotone cost, and the share of sensitive points and decisions the GPU test allows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

import _obj_refine_cases as rc  # noqa: E402
from _obj_refine_cases import F32, F64  # noqa: E402

CASE = {c["name"]: c for c in rc.CASES}


def _residuals64(a, case, pose):
    return rc.points(a["cam"], pose, a["vol"], a["res"], a["stride"], case["band"], F64)


def test_jacobian_equals_central_differences():
    """d r / d delta by central differences of the float64 residual, at points strictly inside their cells (so that the step stays in
    the cell, where the interpolant is a polynomial): step 1e-6, the interpolant is trilinear, so the difference's truncation error is
    O(h^2) of third derivatives that a trilinear form bounds by |d| / stride^3 h^2 ~ 1e-7 relative; 1e-5 absolute on |J| <= ~1."""
    case = CASE["n1024_box_f32"]
    a = build = rc.build(case)
    P = _residuals64(a, case, a["pose"])
    inner = P["valid"] & np.all((P["f"] > 0.05) & (P["f"] < 0.95), axis=1)
    assert inner.sum() > 300
    h = 1e-6
    pose = a["pose"].astype(F64)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = _residuals64(build, case, rc.apply_step(pose, d, F64))["r0"]
        rm = _residuals64(build, case, rc.apply_step(pose, -d, F64))["r0"]
        fd = (rp - rm) / (2 * h)
        err = np.abs(fd - P["J"][:, k])[inner].max()
        assert err < 1e-5, (k, err)


def test_residual_is_distance_without_the_clamp():
    """Inside the band (which lies inside the reference's +-0.05 clamp) and off the border, the residual is Distance()'s value."""
    case = CASE["n1500_wraps"]
    a = rc.build(case)
    P = _residuals64(a, case, a["pose"])
    d = rc.distance64(P["q"], a["vol"].astype(F64), a["res"], a["stride"])
    assert P["valid"].sum() > 1000 and np.array_equal(d[P["valid"]], P["r0"][P["valid"]])


@pytest.mark.parametrize("name", ["n1024_box", "n1024_box_f32", "res17_sphere"])
def test_converges_back_on_an_exact_volume(name):
    """From the case's perturbation (0.02 rad, 4 mm) the float64 restatement comes back to the pose that made the cloud, up to what
    1.5 mm of sensor noise on n points and the trilinear interpolation of a stride-wide grid leave: well inside the perturbation."""
    case = CASE[name]
    a = rc.build(case)
    pose, stats, _ = rc.trace_of(case)
    r0, t0 = rc.pose_error(a["pose"], a["true"])
    r1, t1 = rc.pose_error(pose, a["true"])
    print(name, "start", r0, t0, "end", r1, t1, "cost", stats[0], stats[1], "steps", stats[4])
    assert stats[4] >= 1 and stats[1] < stats[0]
    assert t1 < 0.5 * t0
    if case["shape"] != "sphere":       # (a sphere does not observe rotation)
        assert r1 < 0.5 * r0


def test_capsule_axis_rotation_stays_at_the_dampings_scale():
    """Rotation about the capsule's axis (object z, delta[2]) is unobservable.  The damped matrix is A + lambda diag A + eps n I with A
    positive semi-definite, so its smallest eigenvalue is at least eps n and |delta| <= |b| / (eps n): every step stays finite and
    below that bound, whatever A's own conditioning."""
    case = CASE["capsule"]
    _, _, trace = rc.trace_of(case)
    for row in trace[:-1]:
        if row[58]:
            delta = row[60:66]
            assert np.all(np.isfinite(delta))
    a = rc.build(case)
    T, _ = rc.evaluate(a["cam"], a["pose"], a["vol"], a["res"], a["stride"], case["band"], F64)
    delta, ok, M = rc.solve6(T[:27], rc.LAMBDA0, rc.EPS * T[28], F64)
    assert ok and abs(delta[2]) <= np.linalg.norm(T[21:27]) / (rc.EPS * T[28])
    undamped = np.linalg.eigvalsh(M - np.eye(6) * rc.EPS * T[28])
    print("capsule: smallest eigenvalue without eps", undamped[0], "with", np.linalg.eigvalsh(M)[0], "delta", delta)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_final_cost_never_exceeds_initial(dt):
    for case in rc.CASES:
        _, stats, trace = rc.trace_of(case, dt)
        assert stats[1] <= stats[0], case["name"]
        assert np.all(np.diff(trace[:, 13]) <= 0), case["name"]


def test_special_cases_do_what_they_are_for():
    for name in ("n1", "n5", "outside_band", "on_border"):
        a = rc.build(CASE[name])
        pose, stats, _ = rc.trace_of(CASE[name], F32)
        assert np.array_equal(pose, a["pose"]) and stats[4] == 0, name
    for name in ("outside_band", "on_border"):
        assert rc.trace_of(CASE[name], F32)[1][2] == 0, name
    _, stats, trace = rc.trace_of(CASE["first_step_rejected"])
    assert trace[1, 59] == 1 and trace[1, 15] == 0, "the first step is not rejected"
    a = rc.build(CASE["nan_cell"])
    P = rc.points(a["cam"], a["pose"], a["vol"], a["res"], a["stride"], 0.02, F64)
    assert np.isnan(P["r0"]).any() and not P["valid"][np.isnan(P["r0"])].any()
    assert rc.trace_of(CASE["nan_cell"], F32)[1][4] >= 1


def test_torch_route_agrees_with_the_float32_restatement():
    """Same rule, fp32, another summation order and LAPACK's Cholesky: the poses agree to a few fp32 roundings of a step
    (|delta| <= ~0.03, conditioning ~1e3: 1e-5), wherever both take the same decisions."""
    import torch
    from models import pose_refine
    for name in ("n1024_box_f32", "n65", "capsule", "n5", "outside_band", "iters0"):
        case = CASE[name]
        a = rc.build(case)
        vol = torch.from_numpy(a["vol"].reshape(a["res"], a["res"], a["res"]))
        R, t, stats, trace = pose_refine.refine(torch.from_numpy(a["cam"]), torch.from_numpy(a["pose"][:9]).view(3, 3),
                                                torch.from_numpy(a["pose"][9:]), vol, a["stride"], iters=case["iters"], band=case["band"],
                                                trace=True, route="torch")
        pose, want, tr = rc.trace_of(case, F32)
        got = np.concatenate([R.reshape(9).numpy(), t.reshape(3).numpy()])
        # the first pass and the first step, before any decision can differ: A, b enter through the candidate of pass 1
        assert np.allclose(trace[0, [13, 14]].numpy(), tr[0, [13, 14]], rtol=1e-4, atol=1e-12), name
        if case["iters"] >= 1:
            assert np.abs(trace[1, 16:28].numpy() - tr[1, 16:28]).max() < 1e-5, (name, np.abs(trace[1, 16:28].numpy() - tr[1, 16:28]).max())
        # the end: both stop at the same minimum (decisions at rounding level may differ on the way: 1e-4 of pose, 1 % of cost)
        assert np.abs(got - pose).max() < 1e-4, (name, np.abs(got - pose).max())
        assert np.allclose(stats.numpy()[:4], want[:4], rtol=1e-2, atol=1e-9), (name, stats, want)
        assert float(stats[1]) <= float(stats[0])


# ---- what the GPU test leaves out, checked on the restatements alone -------------------------------------------------------------
def test_sensitive_shares_stay_inside_the_caps():
    """The float32 restatement against float64, teacher forced: at most 2 % of a case's points and 1 in 20 of the decisions over the
    list are sensitive (tests/test_gpu_obj_refine_fp64.py asserts the same of the kernel)."""
    tol, share = rc.measured_tolerances()
    print("tolerances (4 x measured)", tol)
    print("sensitive point shares", {k: v for k, v in share.items() if v})
    for case in rc.CASES:
        if case["n"] >= 50:               # (one point of fewer than 50 is more than 2 %)
            assert share[case["name"]] <= 0.02, (case["name"], share[case["name"]])
    decisions = sensitive = 0
    for case in rc.CASES:
        for rec in rc.teacher_forced(case, rc.trace_of(case, F32)[2]):
            if rec["gap"] is not None:
                decisions += 1
                sensitive += rec["gap"] <= tol["cost"]
    print("decisions", decisions, "sensitive", sensitive)
    assert decisions >= 20 and sensitive * 20 <= decisions
