"""CPU: the depth-frame front end's boundary without a launch -- the argument validation of pn2x_depth_frame_supported /
_work_ints / _clouds (each code and the order among them: a bad value before a limit before a NULL pointer), the slot rule against
a brute-force enumeration, the test frames' own coverage, the renderer's round trip, the binding's refusal of CPU tensors and
the --from_depth flag."""
import argparse
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _depth_cases as D
from hotrack_amd import ext
from hotrack_amd.ext import _DepthFrame as Frame, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENULL, ERANGE = -1, -2, -3
POINTERS = ("depth", "seg", "intrinsics", "clouds", "counts", "background", "work")


def test_the_library_exports_the_entries(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("pn2x_depth_frame_supported", "pn2x_depth_frame_work_ints", "pn2x_depth_frame_clouds"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(Frame) == 144
    assert _lib.pn2_abi_version() == 4


def test_the_bound_record_matches_the_header():
    """_DepthFrame against `struct pn2x_depth_frame` of pn2_ext.h field by field (name, order, kind, array length), and its size
    against the one the library asserts beside the entry."""
    c = ctypes
    src = open(os.path.join(ROOT, "include", "pn2_ext.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    body = re.search(r"struct\s+pn2x_depth_frame\s*\{(.*?)\}\s*;", src, flags=re.S).group(1)
    assert re.search(r"typedef\s+struct\s+pn2x_depth_frame\s+pn2x_depth_frame\s*;", src)
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = [d.strip() for d in stmt.split(",")]
        words = re.sub(r"\b(const|unsigned)\b", "", first.replace("*", " * ")).split()
        base = {"int": "int", "float": "float", "double": "double"}.get(words[0], "other")
        for d in (first, *more):
            kind = "pointer" if "*" in d else base
            assert kind != "other", stmt
            name, length = re.search(r"(\w+)\s*(?:\[(\d+)\])?$", d).groups()
            fields.append((name, kind, int(length or 1)))
    kinds = {c.c_void_p: "pointer", c.c_int: "int", c.c_float: "float", c.c_double: "double"}
    bound = [(n, kinds[getattr(t, "_type_", t) if hasattr(t, "_length_") else t], getattr(t, "_length_", 1)) for n, t in Frame._fields_]
    assert bound == fields
    hip = open(os.path.join(ROOT, "hotrack_amd", "csrc", "depth_frame.hip")).read()
    assert re.findall(r"static_assert\(sizeof\(pn2x_depth_frame\) == (\d+)", hip) == [str(c.sizeof(Frame))]
    sizes = [c.sizeof(t) // getattr(t, "_length_", 1) for _, t in Frame._fields_]   # no implicit padding
    assert sizes == sorted(sizes, reverse=True) and sum(c.sizeof(t) for _, t in Frame._fields_) == c.sizeof(Frame)


def test_supported():
    ok = _lib.pn2x_depth_frame_supported
    assert ok(480, 640, 480, 640, 3, 5120) == 1 and ok(480, 640, 240, 320, 1, 16384) == 1 and ok(50, 70, 50, 70, 3, 1) == 1
    assert ok(480, 640, 240, 640, 3, 5120) == 0 and ok(480, 640, 241, 320, 3, 5120) == 0    # differing / non-integer factor
    assert ok(480, 640, 480, 640, 2, 5120) == 0 and ok(480, 640, 480, 640, 4, 5120) == 0 and ok(480, 640, 480, 640, 0, 5120) == 0
    assert ok(480, 640, 480, 640, 3, 0) == 0 and ok(480, 640, 480, 640, 3, 16385) == 0
    assert ok(0, 640, 0, 640, 3, 5120) == 0 and ok(480, -1, 480, -1, 3, 5120) == 0
    assert ok(1 << 15, 1 << 14, 1 << 15, 1 << 14, 3, 5120) == 0 and ok((1 << 15) - 1, 1 << 14, (1 << 15) - 1, 1 << 14, 3, 5120) == 1


def test_work_ints():
    wi = _lib.pn2x_depth_frame_work_ints
    assert wi(1, 480, 640) == 2 * 300 and wi(8, 480, 640) == 8 * 2 * 300 and wi(3, 50, 70) == 3 * 2 * 4 and wi(1, 32, 32) == 2
    assert wi(1, 1, 1) == 2 and wi(0, 480, 640) == 0 and wi(65535, 480, 640) == 65535 * 600
    assert wi(-1, 480, 640) == EINVAL and wi(1, 0, 640) == EINVAL and wi(1, 480, -3) == EINVAL


def test_depth_frame_clouds_argument_validation():
    one = 16

    def call(h=48, w=64, hs=24, ws=32, c=3, cap=320, b=2, u16=0, flip=0, channel=(0, 1), value=(255, 255), radius=(0.15, 0.25),
             centre=(one, one), **ptr):
        r = Frame(b=b, h=h, w=w, hs=hs, ws=ws, c=c, cap=cap, depth_u16=u16, flip_yz=flip, depth_scale=0.001)
        for name in POINTERS:
            setattr(r, name, ptr.get(name, one))
        for k in range(2):
            r.channel[k], r.value[k], r.radius[k], r.centre[k] = channel[k], value[k], radius[k], centre[k]
        return _lib.pn2x_depth_frame_clouds(ctypes.byref(r), None)

    # bad values
    assert call(hs=24, ws=64) == EINVAL and call(hs=25) == EINVAL and call(ws=33) == EINVAL and call(hs=96, ws=128) == EINVAL
    assert call(c=2) == EINVAL and call(c=0) == EINVAL and call(c=4) == EINVAL
    assert call(channel=(3, 1)) == EINVAL and call(channel=(0, -1)) == EINVAL and call(c=1, channel=(0, 1)) == EINVAL
    assert call(value=(256, 255)) == EINVAL and call(value=(255, -1)) == EINVAL
    assert call(radius=(0.0, 0.25)) == EINVAL and call(radius=(0.15, -1.0)) == EINVAL and call(radius=(float("nan"), 0.25)) == EINVAL
    assert call(cap=0) == EINVAL and call(cap=-5) == EINVAL and call(b=-1) == EINVAL and call(h=0, hs=0) == EINVAL and call(w=-64) == EINVAL
    assert call(u16=2) == EINVAL and call(flip=-1) == EINVAL
    # over a limit
    assert call(cap=16385) == ERANGE and call(b=65536) == ERANGE
    assert call(h=1 << 15, w=1 << 14, hs=1 << 15, ws=1 << 14) == ERANGE
    # NULL: the record, and each of its pointers
    assert _lib.pn2x_depth_frame_clouds(None, None) == ENULL
    for name in POINTERS:
        assert call(**{name: None}) == ENULL, name
    assert call(centre=(None, one)) == ENULL and call(centre=(one, None)) == ENULL
    # the order among them
    assert call(cap=0, b=65536, depth=None) == EINVAL and call(cap=16385, c=2) == EINVAL
    assert call(cap=16385, depth=None) == ERANGE and call(b=65536, seg=None) == ERANGE
    # no frames: nothing is launched and no pointer is looked at; a bad argument is still refused
    assert call(b=0) == 0 and call(b=0, depth=None, work=None) == 0
    assert call(b=0, c=2) == EINVAL and call(b=0, cap=16385) == ERANGE


@pytest.mark.parametrize("cap", [1, 7, 320])
def test_slot_rule_against_enumeration(cap):
    for n in (0, 1, cap - 1, cap, cap + 1, 2 * cap + 3, 7 * cap):
        # brute force, in Python integers: walk the ranks, keep one whenever the running floor moves on
        kept = [(r, r * cap // n) for r in range(n) if n <= cap or (r + 1) * cap // n > r * cap // n]
        if n <= cap:
            kept = [(r, r) for r in range(n)]
        slots = [s for _, s in kept]
        assert len(kept) == min(n, cap) and slots == list(range(min(n, cap))), (n, cap)   # distinct, in order, none skipped
        got = D.slot_of_rank(n, cap)
        assert [(r, int(s)) for r, s in enumerate(got) if s >= 0] == kept, (n, cap)
        if n > cap:  # evenly spaced in rank: neighbours differ by floor(n / cap) or one more
            ranks = np.array([r for r, _ in kept])
            assert set(np.diff(ranks).tolist()) <= {n // cap, n // cap + 1}, (n, cap)
        # every slot of the buffer is covered once the padding is in: mark the points with their rank + 1
        pts = np.repeat(np.arange(1, n + 1, dtype=np.float32)[:, None], 3, axis=1)
        cloud = D.fill_cloud(pts, cap)
        want = np.zeros(cap) if n == 0 else np.array([r + 1 for r, _ in kept] + [1] * (cap - min(n, cap)), dtype=np.float32)
        assert np.array_equal(cloud[:, 0], want) and np.array_equal(cloud[:, 1], want), (n, cap)


def test_cases_cover_the_count_regimes():
    cases = D.cases()
    seen, sizes = set(), set()
    for case in cases:
        D.assert_margins(case)
        B, H, W = case["depth"].shape
        sizes.add((H, W) + case["seg"].shape[1:])
        counts = D.restate(case)["counts"]
        for n in counts.reshape(-1):
            seen.add("zero" if n == 0 else "below_npoint" if n < D.NPOINT else "below_cap" if n < D.CAP else "cap" if n == D.CAP else "above")
        if B > 1:
            assert len(set(counts.reshape(-1).tolist())) == counts.size, case["name"]   # a different count per frame and class
    assert seen == {"zero", "below_npoint", "below_cap", "cap", "above"}
    assert {(48, 64, 48, 64, 1), (60, 80, 30, 40, 3), (50, 70, 50, 70, 3)} <= sizes
    assert any(c["flip_yz"] for c in cases) and any(not c["flip_yz"] for c in cases)
    assert any(c["depth"].dtype == np.uint16 and c["depth_scale"] == 0.00012498664727900177 for c in cases)
    # a class whose first pixel is in the last tile
    case = next(c for c in cases if c["name"] == "60x80_seg30x40")
    ch, val, centre, radius = case["obj"]
    _, valid, per_class = D.classify(case["depth"][0], case["seg"][0], case["intrinsics"][0], [(ch, val, centre[0], radius)], True)
    first = np.flatnonzero((valid & per_class[0][0] & (per_class[0][1] < np.float32(radius))).reshape(-1))[0]
    assert first // D.TILE == (60 * 80 - 1) // D.TILE == 4


def test_render_depth_frame_round_trip():
    from datasets.synthetic import render_depth_frame
    rng = np.random.default_rng(0)
    K = dict(fx=150.0, fy=150.0, cx=80.0, cy=60.0)
    hand = rng.normal(0, 0.03, (400, 3)) + [-0.05, 0.0, 0.5]
    obj = rng.normal(0, 0.03, (400, 3)) + [0.06, 0.01, 0.55]
    depth, seg, raw, scale = render_depth_frame(hand, obj, K, 120, 160)
    assert depth.shape == (120, 160) and depth.dtype == np.float32 and seg.shape == (120, 160, 3) and seg.dtype == np.uint8
    assert raw.dtype == np.uint16 and np.abs(raw * scale - depth).max() <= scale / 2 + 1e-7
    assert ((seg[..., 0] == 255) | (seg[..., 1] == 255)).sum() == (depth > 0).sum() and not (seg[..., 2] != 0).any()
    for cls, pts in enumerate((hand, obj)):
        # every point's pixel holds a depth no farther than the point (the z-buffer keeps the nearest)
        u = np.rint(pts[:, 0] / pts[:, 2] * K["fx"] + K["cx"]).astype(int)
        v = np.rint(pts[:, 1] / pts[:, 2] * K["fy"] + K["cy"]).astype(int)
        assert (depth[v, u] > 0).all() and (depth[v, u] <= pts[:, 2].astype(np.float32)).all()
        # every pixel of the class back-projects to within one pixel's footprint of the point that won it
        vv, uu = np.nonzero(seg[..., cls] == 255)
        z = depth[vv, uu].astype(np.float64)
        back = np.stack([(uu - K["cx"]) * z / K["fx"], (vv - K["cy"]) * z / K["fy"], z], axis=1)
        d = np.abs(back[:, None, :] - pts[None, :, :])
        footprint = z / K["fx"]
        hit = ((d[..., 0] <= footprint[:, None]) & (d[..., 1] <= footprint[:, None]) & (d[..., 2] < 1e-6)).any(axis=1)
        assert hit.all()
    # the same frame through the contract's arithmetic: the crop round each cloud's mean keeps the class's pixels
    case = {"name": "render", "depth": depth[None], "depth_scale": None, "seg": seg[None], "cap": 2048, "flip_yz": False,
            "intrinsics": np.array([[150, 150, 80, 60]], dtype=np.float32),
            "hand": (0, 255, hand.mean(0, keepdims=True).astype(np.float32), 0.15),
            "obj": (1, 255, obj.mean(0, keepdims=True).astype(np.float32), 0.25)}
    counts = D.restate(case)["counts"][0]
    assert counts[0] == (seg[..., 0] == 255).sum() and counts[1] == (seg[..., 1] == 255).sum()


def test_binding_refuses_cpu_tensors():
    depth, seg = torch.zeros(1, 48, 64), torch.zeros(1, 48, 64, 3, dtype=torch.uint8)
    centre, intr = torch.zeros(1, 3), torch.tensor([[60.0, 60.0, 32.0, 24.0]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.depth_frame_clouds(depth, seg, intr, (0, 255, centre, 0.15), (1, 255, centre, 0.25), cap=320)


def test_parser_knows_from_depth():
    sys.path.insert(0, os.path.join(ROOT, "network"))
    try:
        from parse_args import add_args
    finally:
        sys.path.pop(0)
    p = add_args(argparse.ArgumentParser())
    assert p.parse_args([]).from_depth is None
    assert p.parse_args(["--from_depth"]).from_depth is True
