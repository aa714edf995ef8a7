"""GPU: the depth-frame kernels and DepthFrontEnd.clouds against the numpy restatement of their contract (tests/_depth_cases.py),
bit for bit: clouds, counts and background mask; the FPS indices against the CPU oracle on the restatement's padded buffers; the
gathered rows; determinism, independence of the workspaces' previous contents, no host sync, and graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

import _depth_cases as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))

CASES = D.cases()
EXPECTED = {}


def _expected(case):
    if case["name"] not in EXPECTED:
        EXPECTED[case["name"]] = D.restate(case)
    return EXPECTED[case["name"]]


def _device_frames(case):
    dev = torch.device("cuda")
    return {"depth": torch.from_numpy(case["depth"]).to(dev), "seg": torch.from_numpy(case["seg"]).to(dev),
            "intrinsics": torch.from_numpy(case["intrinsics"]).to(dev), "hand_centre": torch.from_numpy(case["hand"][2]).to(dev),
            "obj_centre": torch.from_numpy(case["obj"][2]).to(dev), "depth_scale": case["depth_scale"]}


def _binding_call(case, fr, work=None):
    from hotrack_amd import ext
    return ext.depth_frame_clouds(fr["depth"], fr["seg"], fr["intrinsics"], case["hand"][:2] + (fr["hand_centre"], case["hand"][3]),
                                  case["obj"][:2] + (fr["obj_centre"], case["obj"][3]), case["cap"], case["flip_yz"],
                                  case["depth_scale"], work)


def _front_end(case):
    from models.frame_frontend import DepthFrontEnd
    return DepthFrontEnd(D.NPOINT, cap=case["cap"], hand_radius=case["hand"][3], obj_radius=case["obj"][3], hand_class=case["hand"][:2],
                         obj_class=case["obj"][:2], flip_yz=case["flip_yz"])


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernels_match_the_restatement(case):
    want = _expected(case)
    clouds, counts, background = _binding_call(case, _device_frames(case))
    assert np.array_equal(counts.cpu().numpy(), want["counts"])
    assert np.array_equal(background.cpu().numpy(), want["background"])
    assert np.array_equal(_bits(clouds), want["clouds"].view(np.uint32))


FACTOR_CASES = D.factor_cases()


@pytest.mark.parametrize("case", FACTOR_CASES, ids=[c["name"] for c in FACTOR_CASES])
def test_segment_cell_by_shift_and_by_division(case):
    """f = 1 and 4 find a pixel's segment cell with a shift, f = 3 with a division (csrc/frame_device.h); CASES has only 1 and 2."""
    want = _expected(case)
    assert (want["counts"] > 0).all()
    clouds, counts, background = _binding_call(case, _device_frames(case))
    assert np.array_equal(counts.cpu().numpy(), want["counts"])
    assert np.array_equal(background.cpu().numpy(), want["background"])
    assert np.array_equal(_bits(clouds), want["clouds"].view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_front_end_samples_and_gathers(case, oracle):
    want = _expected(case)
    B, cap = case["depth"].shape[0], case["cap"]
    out = _front_end(case).clouds(_device_frames(case))
    ref_idx = oracle.furthest_point_sample(want["clouds"].reshape(2 * B, cap, 3), D.NPOINT).reshape(B, 2, D.NPOINT)
    idx = out["sample_idx"].cpu().numpy()
    assert np.array_equal(idx, ref_idx)
    rows = np.take_along_axis(want["clouds"], ref_idx[..., None].astype(np.int64).repeat(3, -1), axis=2)
    assert out["hand_points"].shape == out["obj_points"].shape == (B, D.NPOINT, 3)
    assert np.array_equal(_bits(out["hand_points"]), rows[:, 0].view(np.uint32))
    assert np.array_equal(_bits(out["obj_points"]), rows[:, 1].view(np.uint32))
    assert np.array_equal(out["counts"].cpu().numpy(), want["counts"])
    assert np.array_equal(out["background_mask"].cpu().numpy(), want["background"])
    for b in range(B):
        for k in range(2):
            n = int(want["counts"][b, k])
            if D.NPOINT <= n <= cap:   # enough real points: the padding (at distance 0 of the first pick) is never sampled
                assert (idx[b, k] < n).all(), (case["name"], b, k, n)


@pytest.mark.parametrize("case", [CASES[2], CASES[3]], ids=[CASES[2]["name"], CASES[3]["name"]])
def test_repeatable_and_independent_of_the_workspaces(case):
    from hotrack_amd import ext
    fr = _device_frames(case)
    B, H, W = case["depth"].shape
    first = [t.clone() for t in _binding_call(case, fr)]
    again = _binding_call(case, fr)
    work = ext.depth_frame_workspace(B, H, W, case["cap"], fr["depth"].device)
    for t in work:   # NaN bytes everywhere: nothing may depend on what the buffers held
        t.view(torch.uint8).fill_(0xFF)
    into = _binding_call(case, fr, work)
    assert into[0] is work[1] and into[1] is work[2] and into[2] is work[3]
    for a, b, c in zip(first, again, into):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


def test_no_host_sync_and_graph_replay():
    case = CASES[2]
    fe, fr = _front_end(case), _device_frames(case)
    eager = fe.clouds(fr)   # (also allocates the workspaces)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        quiet = fe.clouds(fr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    keys = ("hand_points", "obj_points", "background_mask", "counts", "sample_idx")
    for k in keys:
        assert np.array_equal(_bits(eager[k]), _bits(quiet[k])), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fe.clouds(fr)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fe.clouds(fr)
    for k in keys:   # the replay writes them: poison what it must overwrite
        captured[k].view(torch.uint8).fill_(0xFF) if captured[k].is_contiguous() else captured[k].fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert np.array_equal(_bits(eager[k]), _bits(captured[k])), k
