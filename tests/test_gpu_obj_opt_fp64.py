"""GPU: the object-pose particle optimiser (pn2s_obj_optimize / pn2s_obj_optimize_batch, `obj_optimize_block` in
hotrack_amd/csrc/sdf.hip) step by step against the fp64 restatement of the reference's loop (tests/_obj_opt_cases.py).

Every case of the table is run for every iteration count k from 0 to its own, and the pose and the final search size
(work[0..5], the one part of `work` include/pn2_sdf.h defines) are compared with entry k of the fp64 trace: the search size is
what makes the search-size state machine visible without depending on the scratch layout.  The table's conditions
(tests/test_obj_opt_cases.py) make `success` and the `better` mask the same in fp32 and fp64, so every comparison is one of
continuous quantities, at the tolerances measured there (C.TOL_*)."""
import numpy as np
import pytest
import torch

import _obj_opt_cases as C

pytestmark = pytest.mark.gpu
IDS = [c["name"] for c in C.CASES]
BY_NAME = {c["name"]: c for c in C.CASES}


@pytest.fixture(scope="module")
def sdf():
    from hotrack_amd import sdf as m
    return m


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _device_volume(sdf, vol, fmt):
    lin = _d(vol)
    return sdf.CornerVolume(lin) if fmt.startswith("corner") else lin


@pytest.fixture(scope="module")
def world(sdf):
    """Every case's device inputs and fp64 trace, made once.  Read-only."""
    out = {}
    for c in C.CASES:
        a = C.build(c)
        out[c["name"]] = dict(cam=_d(a["cam"]), R=_d(a["R"]), t=_d(a["t"]), pre=_d(a["pre"]), vol=_device_volume(sdf, a["vol"], c["fmt"]),
                              host=a, trace=C.trace_of(c))
    return out


def _kw(case, k):
    return dict(iterations=k, scaling_coefficient1=case["c1"], scaling_coefficient2=case["c2"], beta=case["beta"])


def _run(sdf, w, case, k, vol=None):
    """-> (R (3,3), t (3,), search (6,)) as float32 numpy, from a NaN-filled caller-owned work tensor."""
    work = torch.full((16 + case["p"],), float("nan"), device="cuda")
    R, t = sdf.obj_optimize(w["cam"], w["R"], w["t"], w["pre"], w["vol"] if vol is None else vol, C.STRIDE, work=work, **_kw(case, k))
    return R.cpu().numpy().reshape(3, 3), t.cpu().numpy().reshape(3), work[:6].cpu().numpy()


def _check_step(case, step, R, t, search, what):
    print(f"{what}: |dR| {np.abs(R - step['rotation']).max():.2e} |dt| {np.abs(t - step['translation']).max():.2e} "
          f"|dsearch| {np.abs(search - step['search']).max():.2e}")
    np.testing.assert_allclose(R, step["rotation"], rtol=0, atol=C.TOL_ROTATION, err_msg=what)
    np.testing.assert_allclose(t, step["translation"], rtol=0, atol=C.TOL_TRANSLATION, err_msg=what)
    np.testing.assert_allclose(search, step["search"], rtol=0, atol=C.TOL_SEARCH, err_msg=what)
    Rd = R.astype(np.float64)
    assert np.allclose(Rd @ Rd.T, np.eye(3), rtol=0, atol=1e-6), what


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_every_iteration_count_against_fp64(sdf, world, case):
    w = world[case["name"]]
    trace = w["trace"]
    for k in range(case["iters"] + 1):
        R, t, search = _run(sdf, w, case, k)
        _check_step(case, trace[k], R, t, search, f"{case['name']} after {k} iterations")
        if not any(step["success"] for step in trace[1:k + 1]):      # nothing has moved yet: the pose is the input, every bit
            assert np.array_equal(R.view(np.int32), w["host"]["R"].view(np.int32))
            assert np.array_equal(t.view(np.int32), w["host"]["t"].view(np.int32))


@pytest.mark.parametrize("p,n", [(1, 1), (257, 255), (2049, 257), (4100, 1000)])
def test_first_iteration_particle_energies(sdf, p, n):
    """evaluate() at the loop's own shapes: the particles of iteration 1 (rounded to float32, as particle_energy takes them)
    against the float64 energies at exactly those poses -- tells "the energy is wrong" from "the update is wrong"."""
    case = C._case("energy", p, n, 1, 100 + p + n, angle=0.02, trans=0.003, shape="capsule", outliers=3 if n > 3 else 0)
    a = C.build(case)
    rot, tr, want = C.first_particles(case)
    got = sdf.particle_energy(_d(a["cam"]), _d(rot), _d(tr), _d(a["vol"]), C.STRIDE).cpu().numpy()
    print(f"p {p} n {n}: largest |d sdf_energy| {np.abs(got - want).max():.2e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=C.TOL_ENERGY)


def test_layout_and_storage_type_change_no_bit_inside_the_loop(sdf, world):
    """p = 2049: corner layout == linear volume, and an fp16 volume == the same values stored as fp32, in every bit of the
    pose and of the search size, at every iteration count."""
    case = BY_NAME["p2049_linear16"]
    w = world[case["name"]]
    vol16 = w["host"]["vol"]
    assert vol16.dtype == np.float16
    lin16, lin32 = _d(vol16), _d(vol16.astype(np.float32))
    variants = {"linear16": lin16, "corner16": sdf.CornerVolume(lin16), "linear32": lin32, "corner32": sdf.CornerVolume(lin32)}
    for k in range(case["iters"] + 1):
        base = _run(sdf, w, case, k, vol=lin16)
        for name, vol in variants.items():
            got = _run(sdf, w, case, k, vol=vol)
            for x, y in zip(base, got):
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), (name, k)


def test_batch_of_table_problems(sdf, world):
    """Three problems of the table on one set of 2049 particles, n = 257 / 255 (inactive) / 1000, in one batched launch per
    iteration: bit for bit the three single calls, the inactive one untouched, the active ones on their fp64 traces."""
    names = ["p2049_corner16", "p2049_batch_n255", "p2049_batch_n1000"]
    cases = [BY_NAME[x] for x in names]
    ws = [world[x] for x in names]
    assert len({c["n"] for c in cases}) == 3 and all(c["p"] == 2049 and c["fmt"] == "corner16" for c in cases)
    assert all(torch.equal(w["pre"], ws[0]["pre"]) for w in ws)
    R0, t0 = torch.stack([w["R"] for w in ws]), torch.stack([w["t"] for w in ws])
    for k in (0, 1, 2):
        clouds = [ws[0]["cam"], None, ws[2]["cam"]]
        R, t = sdf.obj_optimize_batch(clouds, R0, t0, ws[0]["pre"], [ws[0]["vol"], None, ws[2]["vol"]], C.STRIDE, **_kw(cases[0], k))
        assert np.array_equal(_bits(R[1]), _bits(R0[1])) and np.array_equal(_bits(t[1].reshape(3)), _bits(t0[1]))
        for j in (0, 2):
            Rs, ts, _ = _run(sdf, ws[j], cases[j], k)
            assert np.array_equal(_bits(R[j]), Rs.view(np.int32)) and np.array_equal(_bits(t[j].reshape(3)), ts.view(np.int32)), (j, k)
            step = ws[j]["trace"][k]
            np.testing.assert_allclose(R[j].cpu().numpy(), step["rotation"], rtol=0, atol=C.TOL_ROTATION)
            np.testing.assert_allclose(t[j].cpu().numpy().reshape(3), step["translation"], rtol=0, atol=C.TOL_TRANSLATION)
    # all three active: each equals its single call
    R, t = sdf.obj_optimize_batch([w["cam"] for w in ws], R0, t0, ws[0]["pre"], [w["vol"] for w in ws], C.STRIDE, **_kw(cases[0], 2))
    for j in range(3):
        Rs, ts, _ = _run(sdf, ws[j], cases[j], 2)
        assert np.array_equal(_bits(R[j]), Rs.view(np.int32)) and np.array_equal(_bits(t[j].reshape(3)), ts.view(np.int32)), j
        np.testing.assert_allclose(R[j].cpu().numpy(), ws[j]["trace"][2]["rotation"], rtol=0, atol=C.TOL_ROTATION)
        np.testing.assert_allclose(t[j].cpu().numpy().reshape(3), ws[j]["trace"][2]["translation"], rtol=0, atol=C.TOL_TRANSLATION)


def test_repeatable_at_p4100(sdf, world):
    """The ticket decides which workgroup does the update, not what it computes: two calls, the same bits."""
    for name in ("p4100_outliers", "p4100_n1000"):
        case, w = BY_NAME[name], world[name]
        a, b = _run(sdf, w, case, case["iters"]), _run(sdf, w, case, case["iters"])
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), name
