"""CPU: the fp64 restatement of the object-pose particle optimiser (tests/_obj_opt_cases.py) and its case table -- that the
restatement is the reference's loop, that every case meets the conditions under which a comparison with an fp32 kernel is
decisive, and that the GPU test's tolerances (tests/test_gpu_obj_opt_fp64.py) are the measured ones."""
import os

import numpy as np
import pytest

import _obj_opt_cases as C

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = [c["name"] for c in C.CASES]


def test_restatement_reproduces_the_reference_vectors():
    """R_ref / t_ref of sdf_optimize.npz are the imported reference's own output (gf_optimize_obj.optimize); the tolerances
    are those tests/test_gpu_sdf.py applies to the kernel on the same vectors."""
    z = np.load(os.path.join(G, "sdf_optimize.npz"))
    i = 0
    while f"o{i}_vol" in z:
        _, stride = z[f"o{i}_meta"]
        tr = C.optimize64(z[f"o{i}_pcld"], z[f"o{i}_R_init"], z[f"o{i}_t_init"], z[f"o{i}_pre"], z[f"o{i}_vol"], float(stride))
        assert len(tr) == 11
        np.testing.assert_allclose(tr[-1]["rotation"], z[f"o{i}_R_ref"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(tr[-1]["translation"], z[f"o{i}_t_ref"], rtol=0, atol=2e-6)
        i += 1
    assert i >= 2


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_case_is_decisive_and_inside_the_domain(case):
    tr = C.trace_of(case)
    assert len(tr) == case["iters"] + 1
    for k, step in enumerate(tr[1:], 1):
        assert step["margin_energy"] >= C.MIN_MARGIN_ENERGY, (k, step["margin_energy"])
        assert step["margin_domain"] > C.MIN_MARGIN_DOMAIN, (k, step["margin_domain"])
        assert np.isfinite(step["sdf_energy"]).all() and step["sdf_energy"].shape == (case["p"],)
    a = C.build(case)
    assert a["cam"].shape == (case["n"], 3) and a["pre"].shape == (case["p"], 6) and not a["pre"][0].any()
    if case["p"] == 1:
        assert not any(step["success"] for step in tr[1:])      # particle 0 alone is never better than itself


def test_table_covers_what_it_must():
    assert {c["p"] for c in C.CASES} >= set(C.P_LIST)
    assert {c["n"] for c in C.CASES} >= set(C.N_LIST)
    for lo, hi in ((63, 2048), (2049, 1 << 30)):                 # every format at a mid-sized p and beyond one reduction trip
        assert {c["fmt"] for c in C.CASES if lo <= c["p"] < hi} == set(C.FORMATS), (lo, hi)
    assert {c["iters"] for c in C.CASES} >= {10} and all(c["iters"] >= 1 for c in C.CASES)   # (0 iterations: entry 0 of a trace)
    assert any((c["c1"], c["c2"], c["beta"]) != (0.02, 2.0, 0.9) for c in C.CASES)
    assert any((c["c1"], c["c2"], c["beta"]) == (0.02, 2.0, 0.9) for c in C.CASES)
    seen = set()
    for c in C.CASES:
        if c["p"] > 1 and np.any(C.build(c)["pre"][1:] != 0):    # (a), (b), (c) count with real particles only
            seen |= C.branches(step["success"] for step in C.trace_of(c)[1:])
    assert seen == {"a", "b", "c", "d"}, seen


def test_outliers_bind_both_clamps():
    """In an `outliers` case some points lie beyond the volume in the object frame: there the index clamps bind (the unclamped
    voxel coordinate leaves [0, res - 1]) and the +-0.05 value clamp binds (the volume holds +-0.1 out there)."""
    cases = [c for c in C.CASES if c["outliers"]]
    assert cases
    for c in cases:
        a = C.build(c)
        obj = (a["cam"].astype(np.float64) - a["t"]) @ a["R"].astype(np.float64)
        v = (obj + 0.2) / C.STRIDE
        out = np.any((v < 0) | (v > C.RES - 1), axis=1)
        assert 0 < out.sum() < c["n"] // 8
        d = C.distance64(obj, a["vol"].astype(np.float64), C.RES, C.STRIDE)
        assert np.all(np.abs(d[out]) == np.float64(np.float32(0.05))) and np.all(np.abs(d[~out]) < 0.049)


def test_tolerances_are_the_measured_ones():
    """Re-measure the fp32 oracle's deviation from the fp64 traces; each stays within the recorded figure (= tolerance / 4,
    above the 4-ulp floor).  The oracle's C library is built on demand: where it cannot be, this fails."""
    from oracle import sdf_oracle as S
    worst = dict(rotation=0.0, translation=0.0, search=0.0, sdf_energy=0.0)
    for case in C.CASES:
        a, ref, got = C.build(case), C.trace_of(case), []
        S.obj_optimize(a["cam"], a["R"], a["t"], a["pre"], a["vol"], C.STRIDE, iterations=case["iters"], trace=got, **C.hyper(case))
        assert [g["success"] for g in got] == [r["success"] for r in ref[1:]], case["name"]
        for g, r in zip(got, ref[1:]):
            for key in worst:
                worst[key] = max(worst[key], float(np.abs(g[key].astype(np.float64) - r[key]).max()))
    print("fp32 oracle vs fp64, largest absolute deviation:", worst)
    assert worst["rotation"] <= C.DEV_ROTATION and 4 * C.DEV_ROTATION <= C.TOL_ROTATION
    assert worst["translation"] <= C.DEV_TRANSLATION and 4 * C.DEV_TRANSLATION <= C.TOL_TRANSLATION
    assert worst["search"] <= C.DEV_SEARCH and 4 * C.DEV_SEARCH <= C.TOL_SEARCH
    assert worst["sdf_energy"] <= C.DEV_ENERGY and 4 * C.DEV_ENERGY <= C.TOL_ENERGY
    for tol, dev in ((C.TOL_ROTATION, C.DEV_ROTATION), (C.TOL_TRANSLATION, C.DEV_TRANSLATION), (C.TOL_SEARCH, C.DEV_SEARCH),
                     (C.TOL_ENERGY, C.DEV_ENERGY)):
        assert tol == 4 * dev       # no floor binds: each tolerance is exactly four times its measured deviation
