"""GPU: pn2s_obj_refine_batch -- every problem of a batch has the bits of the single entry, an inactive problem keeps every byte."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _obj_refine_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
CASE = {c["name"]: c for c in rc.CASES}


def _problem(name, dev):
    a = rc.build(CASE[name])
    vol = torch.from_numpy(a["vol"].reshape(a["res"], a["res"], a["res"])).to(dev)
    return dict(pcld=torch.from_numpy(a["cam"]).to(dev), R=torch.from_numpy(a["pose"][:9]).view(3, 3).to(dev),
                t=torch.from_numpy(a["pose"][9:]).to(dev), vol=vol, stride=a["stride"])


def _single(sdf, p, corner, trace):
    return sdf.obj_refine(p["pcld"], p["R"], p["t"], corner, p["stride"], trace=trace)


def test_one_problem_equals_the_single_entry():
    from hotrack_amd import sdf
    dev = torch.device("cuda", 0)
    p = _problem("n1500_wraps", dev)
    corner = sdf.CornerVolume(p["vol"])
    want = _single(sdf, p, corner, True)
    got = sdf.obj_refine_batch([p["pcld"]], [p["R"]], [p["t"]], [corner], p["stride"], trace=True)
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[1][0], want[1][0]) and torch.equal(got[2][0], want[2])
    assert torch.equal(got[3][0], want[3])


def test_three_problems_an_inactive_one_and_a_shared_volume():
    from hotrack_amd import sdf
    dev = torch.device("cuda", 0)
    # unequal clouds on fp16 41^3 volumes; problems 0 and 3 share one volume object; problem 1 is inactive with a NULL volume entry
    ps = [_problem("n1024_box", dev), None, _problem("capsule", dev), _problem("n65", dev)]
    box = sdf.CornerVolume(ps[0]["vol"])
    corners = [box, None, sdf.CornerVolume(ps[2]["vol"]), box]
    idle_R, idle_t = torch.eye(3, device=dev) * 0.5, torch.tensor([1.0, 2.0, 3.0], device=dev)
    cache = {}
    for _ in range(2):       # (the second call takes the offsets and the pointer table from the cache)
        got = sdf.obj_refine_batch([None if p is None else p["pcld"] for p in ps], [idle_R if p is None else p["R"] for p in ps],
                                   [idle_t if p is None else p["t"] for p in ps], corners, 0.01, trace=True, cache=cache)
        for k, p in enumerate(ps):
            if p is None:
                assert torch.equal(got[0][k], idle_R) and torch.equal(got[1][k].reshape(3), idle_t)
                assert not got[2][k].any() and not got[3][k].any()      # the stats and trace rows handed in (zeros) are untouched
                continue
            want = _single(sdf, p, corners[k], True)
            assert torch.equal(got[0][k], want[0][0]) and torch.equal(got[1][k], want[1][0]), k
            assert torch.equal(got[2][k], want[2]) and torch.equal(got[3][k], want[3]), k
            assert float(got[2][k][1]) <= float(got[2][k][0])


def test_the_optimiser_methods():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "network"))
    from hotrack_amd import sdf
    from models.optimization_obj import gf_optimize_obj
    dev = torch.device("cuda", 0)
    opt = gf_optimize_obj({"device": dev}, seed=1)
    ps = [_problem("n1024_box", dev), _problem("n65", dev)]
    opt.load_volume(ps[0]["vol"], 0.01)
    poses = [{"rotation": p["R"].view(1, 3, 3), "translation": p["t"].view(1, 3, 1)} for p in ps]
    single = [opt.refine(p["pcld"], pose) for p, pose in zip(ps, poses)]
    batch = opt.refine_batch([p["pcld"] for p in ps] + [None], poses + [poses[0]], [opt._corners, opt._corners, None])
    for a, b in zip(single, batch):
        assert all(torch.equal(a[k], b[k]) for k in ("rotation", "translation", "refine_stats"))
    assert torch.equal(batch[2]["rotation"], poses[0]["rotation"]) and batch[0]["translation"].shape == (1, 3, 1)
    torch_route = opt.refine(ps[0]["pcld"], poses[0], route="torch")
    assert (torch_route["translation"] - single[0]["translation"]).abs().max() < 1e-4
