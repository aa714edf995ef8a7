"""GPU: pn2s_obj_refine (hotrack_amd/csrc/sdf_refine.hip) against float64, teacher forced: for every pass the kernel's own traced
states are taken and A, b, cost, count, the step and the next pose recomputed in float64 (tests/_obj_refine_cases.py).  The
tolerances are 4 x the worst |float32 restatement - float64| of each quantity over the case list, recomputed on every run.

Measured on an MI355X (this file's output): see DESIGN.md 8o."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _obj_refine_cases as rc  # noqa: E402
from _obj_refine_cases import F32, F64  # noqa: E402

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in rc.CASES}
NAMES = [c["name"] for c in rc.CASES]


def _upload(case):
    from hotrack_amd import sdf
    a = rc.build(case)
    dev = torch.device("cuda", 0)
    vol = torch.from_numpy(a["vol"].reshape(a["res"], a["res"], a["res"])).to(dev)
    return a, dict(pcld=torch.from_numpy(a["cam"]).to(dev), rotation=torch.from_numpy(a["pose"][:9]).view(3, 3).to(dev),
                   translation=torch.from_numpy(a["pose"][9:]).to(dev), volume=sdf.CornerVolume(vol), voxel_scale=a["stride"],
                   iters=case["iters"], band=case["band"])


@pytest.fixture(scope="module")
def tolerances():
    tol, share = rc.measured_tolerances()
    print("tolerances (4 x |float32 restatement - float64|):", {k: float(v) for k, v in tol.items()})
    return tol


@pytest.fixture(scope="module")
def runs():
    from hotrack_amd import sdf
    out = {}
    for case in rc.CASES:
        a, args = _upload(case)
        R, t, stats, trace = sdf.obj_refine(trace=True, **args)
        out[case["name"]] = (a, args, torch.cat([R.reshape(9), t.reshape(3)]).cpu().numpy(), stats.cpu().numpy(), trace.cpu().numpy())
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_pass_agrees_with_float64(name, runs, tolerances):
    case = CASE[name]
    a, _, pose, stats, trace = runs[name]
    dev, share, recs = rc.deviations(case, trace)
    print(name, {k: float(v) for k, v in dev.items()}, "sensitive share", share)
    for q in rc.QUANTITIES:
        assert dev[q] <= tolerances[q], (name, q, dev[q], tolerances[q])
    if case["n"] >= 50:
        assert share <= 0.02
    for k, (row, rec) in enumerate(zip(trace, recs)):
        assert abs(row[56] - rec["T"][28]) <= rec["n_sensitive"], (name, k)                      # the count, sensitive points aside
        if rec["gap"] is not None and rec["gap"] > tolerances["cost"] and rec["n_sensitive"] == 0:     # a decision that is not sensitive
            want = rc.cost_of(rec["T"], F64) <= trace[k - 1, 13] and rec["T"][28] >= 0.5 * trace[k - 1, 14]
            assert bool(row[15]) == bool(want), (name, k)
    assert stats[1] <= stats[0] and np.array_equal(pose, trace[-1, :12])
    assert np.all(np.diff(trace[:, 13]) <= 0)


def test_sensitive_decisions_stay_under_one_in_twenty(runs, tolerances):
    decisions = sensitive = 0
    for name in NAMES:
        for rec in rc.teacher_forced(CASE[name], runs[name][4]):
            if rec["gap"] is not None:
                decisions += 1
                sensitive += rec["gap"] <= tolerances["cost"]
    print("decisions", decisions, "sensitive", sensitive)
    assert decisions >= 20 and sensitive * 20 <= decisions


def test_the_special_cases(runs):
    for name in ("n1", "n5", "outside_band", "on_border"):
        a, _, pose, stats, trace = runs[name]
        assert np.array_equal(pose, a["pose"]) and stats[4] == 0, name
    for name in ("outside_band", "on_border"):
        assert runs[name][3][2] == 0 and runs[name][3][3] == 0
    assert runs["iters0"][4].shape == (1, rc.TRACE_ROW) and np.array_equal(runs["iters0"][2], runs["iters0"][0]["pose"])
    tr = runs["first_step_rejected"][4]
    assert tr[1, 59] == 1 and tr[1, 15] == 0 and np.array_equal(tr[1, :12], tr[0, :12]) and tr[1, 12] > tr[0, 12]
    assert runs["nan_cell"][3][4] >= 1 and np.all(np.isfinite(runs["nan_cell"][2]))
    assert np.all(np.isfinite(runs["capsule"][4][:, 60:66]))
    assert runs["at_optimum"][3][1] <= runs["at_optimum"][3][0]


@pytest.mark.parametrize("name", ["n1500_wraps", "n64", "nan_cell"])
def test_repeatable_untraced_and_without_readback(name, runs):
    from hotrack_amd import sdf
    _, args, pose, stats, trace = runs[name]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        R, t, st = sdf.obj_refine(**args)                       # no trace: the same bits
        R2, t2, st2, tr2 = sdf.obj_refine(trace=True, **args)   # a second traced run
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for got in ((R, t, st), (R2, t2, st2)):
        assert np.array_equal(torch.cat([got[0].reshape(9), got[1].reshape(3)]).cpu().numpy(), pose)
        assert np.array_equal(got[2].cpu().numpy(), stats)
    assert np.array_equal(tr2.cpu().numpy(), trace)


def test_graph_capture_replays_the_same_bits(runs):
    from hotrack_amd import sdf
    _, args, pose, stats, _ = runs["n1024_box"]
    sdf.obj_refine(**args)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        R, t, st = sdf.obj_refine(**args)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat([R.reshape(9), t.reshape(3)]).cpu().numpy(), pose)
        assert np.array_equal(st.cpu().numpy(), stats)


def test_refused_calls_leave_the_outputs_untouched(runs):
    from hotrack_amd import sdf
    _, args, _, _, _ = runs["n65"]
    dev = args["pcld"].device
    pose = torch.full((12,), 7.0, device=dev)
    stats = torch.full((8,), 7.0, device=dev)

    def record(**kw):
        r = sdf._Refine(problems=1, n=65, res=41, vol_fmt=3, iters=8, bbox_min=-0.2, stride=0.01, band=0.02)
        r.pcld, r.volume, r.poses, r.stats = args["pcld"].data_ptr(), args["volume"].data.data_ptr(), pose.data_ptr(), stats.data_ptr()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    EINVAL, ENULL, ERANGE = -1, -2, -3   # include/pn2_hip.h
    for kw, code in ((dict(n=0), EINVAL), (dict(problems=2), EINVAL), (dict(iters=-1), EINVAL), (dict(vol_fmt=1), EINVAL),
                     (dict(band=float("nan")), EINVAL), (dict(stride=0.0), EINVAL), (dict(res=1), EINVAL), (dict(iters=65), ERANGE),
                     (dict(res=1025), ERANGE), (dict(volume=None), ENULL), (dict(stats=None), ENULL), (dict(pcld=None), ENULL)):
        assert sdf._lib.pn2s_obj_refine(ctypes.byref(record(**kw)), None) == code, kw
    assert sdf._lib.pn2s_obj_refine(None, None) == ENULL
    assert sdf._lib.pn2s_obj_refine_batch(ctypes.byref(record(cloud_off=None, vols=None)), None) == ENULL
    torch.cuda.synchronize()
    assert bool((pose == 7).all()) and bool((stats == 7).all())
    with pytest.raises(TypeError):
        sdf.obj_refine(args["pcld"], args["rotation"], args["translation"], args["volume"].source, 0.01)
    with pytest.raises(ValueError):
        sdf.obj_refine(**dict(args, iters=65))
