"""CPU: the frame lists of tests/_pose_metric_cases.py hold what the GPU test (tests/test_gpu_seq_eval_fp64.py) relies on: every
kind of frame in every mode, float64 values where the issue expects them, and no frame within its own tolerance of a flag's
threshold (if that fails the inputs are wrong, not the assertion).  Prints the restated-cosine figures."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pose_metric_cases as P  # noqa: E402

MODES = [tuple(int(v) for v in m) for m in np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))["modes"]]


def test_all_nine_modes():
    assert sorted(MODES) == sorted([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (-1, 0), (5, 0)])


@pytest.mark.parametrize("axis,sym", MODES)
def test_frames_and_references(axis, sym):
    fr = P.frames(axis, sym)
    ref = P.reference(fr, axis, sym)
    kind = fr["kind"]
    F = len(kind)
    assert F < 63 and F % 2 == 0 and np.gcd(F, 64) == 2   # tiled, a frame meets many lanes
    at = lambda name: kind.index(name)
    deg, td = ref["deg"], ref["td"]
    assert np.isfinite(deg).all() and (ref["lo"] <= deg).all() and (deg <= ref["hi"]).all()
    # the ladder: 10^-k radians, to what float32 rotations can hold (~1e-7 / sin)
    for k in range(8):
        a = np.degrees(10.0 ** -k)
        assert ref["lo"][at(f"rung{k}")] <= a * (1 + 1e-6) + 1e-12 and a * (1 - 1e-6) <= ref["hi"][at(f"rung{k}")] + 0.05
    assert (fr["gR"][at("identical")] == fr["pR"][at("identical")]).all()
    ident = deg[at("identical")]
    assert ident < 0.05
    # pred = gt diag(s): the identical-rotation value where the mode minimises over that flip (or the flipped column is not the
    # mode's, or |cos| is taken), 180 degrees where it does not
    for s in P.HALF_TURNS:
        d = deg[at("flip" + "".join("+" if v > 0 else "-" for v in s))]
        if 0 <= axis <= 2:
            same = s[axis] > 0 or sym
        else:
            same = s in P.FLIPS.get(axis, [])
        assert (d == ident) if same else (d > 179.9), (s, d)
    if 0 <= axis <= 2:   # parallel and antiparallel columns both occur
        cs = [s[axis] for s in P.HALF_TURNS]
        assert 1 in cs and -1 in cs
    c, _ = P.cosines_fp64(fr, axis, sym)
    assert c[at("scaled"), 0] > 1.001 and deg[at("scaled")] == 0.0 and ref["hi"][at("scaled")] == 0.0
    far = at("far")
    assert np.abs(fr["gt"][far]).min() > 900 and 1e-3 < td[far] < 2e-3
    d32 = fr["gt"][far] - fr["pt"][far]
    assert (d32.astype(np.float64) == fr["gt"][far].astype(np.float64) - fr["pt"][far].astype(np.float64)).all()   # exact in fp32
    # all four combinations per flag
    for tag, col in (("5", 0), ("10", 1)):
        got = {(a, m): ref["flags"][at(f"thr{tag}{a}{m}"), col] for a in "+-" for m in "+-"}
        assert got == {("-", "-"): 1.0, ("-", "+"): 0.0, ("+", "-"): 0.0, ("+", "+"): 0.0}
    # margins: no frame within its own tolerance of a threshold
    for thr in (5.0, 10.0):
        assert ((ref["hi"] + 64 * P.ulps(ref["hi"]) < thr) | (ref["lo"] - 64 * P.ulps(ref["lo"]) > thr)).all()
    for thr in (0.05, 0.10):
        assert (np.abs(td - thr) > 8 * P.U * td).all()
    # the restated float32 cosine sits inside the derived bound
    c32 = P.cosines_fp32(fr, axis, sym).astype(np.float64)
    c64, ab = P.cosines_fp64(fr, axis, sym)
    worst = np.max(np.abs(c32 - c64) / (P.delta(axis) * ab))
    print(f"mode ({axis},{sym}): {F} frames; |cos32 - cos64| / bound {worst:.3f}; worst interval width {np.max(ref['hi'] - ref['lo']):.3g} deg; "
          f"|deg32 - deg| max {np.max(np.abs(ref['deg32'] - deg)):.3g}")
    assert worst <= 1.0
    assert ((ref["lo"] <= ref["deg32"]) & (ref["deg32"] <= ref["hi"])).all()


def test_tiling_puts_frames_in_other_blocks_and_lanes():
    fr = P.frames(5, 0)
    F = len(fr["kind"])
    for T in P.T_SIZES:
        tiled, idx = P.tile(fr, T)
        assert tiled["gR"].shape == (T, 3, 3) and tiled["pt"].shape == (T, 3) and tiled["gR"].dtype == np.float32
    _, idx = P.tile(fr, 257)
    where = np.flatnonzero(idx == 0)
    assert len(set(where // 64)) >= 4 and len(set(where % 64)) >= 8
