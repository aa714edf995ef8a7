"""GPU: hand_pose_eval_kernel<F16> and hand_pose_update_kernel (hotrack_amd/csrc/hand_pose.hip) over the shape and dtype range
pn2x_hand_pose_opt_supported accepts, through ext.hand_pose_energy / ext.hand_pose_opt, against the plain references of
tests/_hand_pose_cases.py (anchored to the recorded fixture and checked case by case in tests/test_hand_pose_cases.py).

Evaluation, per case of the table (C.eval_case_specs): the geometry against float64 within GEOM_TOL (the synthetic hand has the
fixture's size at every vertex count), every element written; the energies against evaluate()'s terms formed on the geometry
the kernel wrote, within E_TOL for all but ceil(P / 384) (at least 2) candidates, each of which must be explained by vertices
that sit on a pixel's or a voxel's edge (C.assert_energies).  Around the second pass of the candidate loop, rows are bit-equal whichever pass or wave computed them.

Update: one iteration at a time against reference_update fed the energies hand_pose_energy returns at the same state, with
the suite's tolerances (trace and search sizes rtol 1e-5 / atol 1e-6, rotation R_TOL, translation KP_TOL, pose code THETA_TOL),
and three iterations in one call bit-equal to three calls of one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_pose_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

_RESULTS = {}


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _refill_with_nan(*numels):
    """Best effort at making an unwritten element visible: the binding allocates its outputs itself, so blocks of the outputs'
    sizes are filled with NaN and released just before the call.  The caching allocator usually hands them out again, and
    _evaluate reports whether it did; where it did not, the finiteness assertions alone stand.  -> the released addresses."""
    blocks = [torch.full((n,), float("nan"), device="cuda") for n in numels]
    torch.cuda.synchronize()
    return {b.data_ptr() for b in blocks}


def _evaluate(case):
    """(energy, vertices, keypoints) of the kernel on the CPU, once per case."""
    if case.name not in _RESULTS:
        from hotrack_amd import ext
        kw, state = C.to_kernel(case), case.state.cuda()
        released = _refill_with_nan(4 * case.P, case.P, case.P * case.V * 3, case.P * 63)
        energy, verts, kp = ext.hand_pose_energy(state=state, with_geometry=True, **kw)
        torch.cuda.synchronize()
        reused = [what for what, x in (("energy", energy), ("vertices", verts), ("keypoints", kp)) if x.data_ptr() in released]
        print(f"{case.name}: outputs allocated over NaN-filled memory: {', '.join(reused) or 'none'}")
        _RESULTS[case.name] = (energy.cpu(), verts.cpu(), kp.cpu())
    return _RESULTS[case.name]


@pytest.mark.parametrize("name", C.EVAL_CASES)
def test_evaluation_matches_the_references(name):
    case = C.get_case(name, _cus())
    energy, verts, kp = _evaluate(case)
    # 1. geometry
    assert verts.shape == (case.P, case.V, 3) and kp.shape == (case.P, 21, 3) and energy.shape == (case.P,)
    assert bool(torch.isfinite(verts).all()) and bool(torch.isfinite(kp).all()) and bool(torch.isfinite(energy).all())
    v64, k64 = C.reference_geometry(case)
    dv, dk = float((verts.double() - v64).abs().max()), float((kp.double() - k64).abs().max())
    print(f"{name} (P {case.P}, V {case.V}, K {case.K}, res {case.res}, {case.volume.dtype}): kernel vs float64: vertices {dv:.3e} m, "
          f"keypoints {dk:.3e} m")
    assert dv <= C.GEOM_TOL and dk <= C.GEOM_TOL
    # 2. energies, on the geometry the kernel wrote
    want = C.reference_terms(case, verts, kp)
    if name == "gate-off":  # 4. candidate 0 does not penetrate: the attraction term, a large one, is in no reference energy
        assert not want["gate"] and float(want["attraction"].min()) > 100 * C.E_TOL and torch.equal(want["energy"], want["base"])
    C.assert_energies(energy.numpy(), want, case, verts, f"{name}: kernel vs evaluate() on its geometry")


def test_candidates_do_not_depend_on_the_pass_or_wave_that_computed_them():
    cus = _cus()
    first, _, last = C.second_pass_counts(cus)
    small, large = C.get_case("second-pass+0", cus), C.get_case("second-pass+5", cus)
    assert (small.P, large.P) == (first, last) and torch.equal(small.pre, large.pre[:first])
    (e0, v0, k0), (e1, v1, k1) = _evaluate(small), _evaluate(large)

    def same(a, b):
        return torch.equal(a.view(torch.int32), b[:first].contiguous().view(torch.int32))

    rows = torch.nonzero((e0.view(torch.int32) != e1[:first].view(torch.int32)))[:8].flatten().tolist()
    print(f"{cus} compute units: {first} candidates in one pass, {last} in two; rows whose energy differs: {rows}")
    assert same(v0, v1) and same(k0, k1) and same(e0, e1)


def test_the_workload_count_is_a_prefix_of_the_limit():
    """5120 and 8192 candidates deal the rows over the waves differently (rounds = 2 and 3 on 256 compute units)."""
    cus = _cus()
    for dt in ("fp16", "fp32"):
        (e0, v0, k0), (e1, v1, k1) = _evaluate(C.get_case(f"workload-5120-{dt}", cus)), _evaluate(C.get_case(f"limit-8192-{dt}", cus))
        assert torch.equal(v0, v1[:5120]) and torch.equal(k0, k1[:5120]) and torch.equal(e0, e1[:5120])


# ---- the update ----------------------------------------------------------------------------------------------------------------
def _proper(R, what):
    R = R.double().view(3, 3)
    a, b = float((R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max()), abs(float(torch.linalg.det(R)) - 1)
    print(f"{what}: |R R^T - I| = {a:.2e}, |det R - 1| = {b:.2e}")
    assert a < 1e-5 and b < 1e-5


def _one_iteration(case, kw, state_in, what):
    """One hand_pose_opt iteration from `state_in` against reference_update on the kernel's energies at that state.
    -> (state after, trace row, reference trace row)."""
    from hotrack_amd import ext
    energy, _, _ = ext.hand_pose_energy(state=state_in.clone(), **kw)
    state = state_in.clone()
    tr = ext.hand_pose_opt(state=state, iterations=1, scaling_coefficient2=C.C2, beta=C.BETA, trace=True, **kw)
    torch.cuda.synchronize()
    want, want_tr = C.reference_update(state_in, case.pre, energy, C.C2, C.BETA, case.tables["comps"])
    got, got_tr = state.cpu().double(), tr.cpu().double()[0]

    def sl(a, n):
        return slice(a, a + n)

    d = {k: float((got[s] - want[s]).abs().max()) for k, s in (("R", sl(C.S_R, 9)), ("t", sl(C.S_T, 3)), ("theta", sl(C.S_THETA, 45)))}
    print(f"{what}: success {int(got_tr[2])}, better candidates {int((energy < energy[0]).sum())} of {case.P}, |dR| {d['R']:.2e}, "
          f"|dt| {d['t']:.2e}, |dtheta| {d['theta']:.2e}, max rel d(search) "
          f"{float(((got[sl(C.S_SEARCH, 16)] - want[sl(C.S_SEARCH, 16)]).abs() / want[sl(C.S_SEARCH, 16)]).max()):.2e}")
    assert tr.shape == (1, 19) and bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_tr).all())
    assert float(got_tr[2]) == float(want_tr[2])
    assert torch.allclose(got_tr, want_tr, rtol=1e-5, atol=1e-6)
    for a in (C.S_SEARCH, C.S_PREV):
        assert torch.allclose(got[sl(a, 16)], want[sl(a, 16)], rtol=1e-5, atol=1e-6)
    assert float(got[C.S_PREV_OK]) == float(want[C.S_PREV_OK])
    assert d["R"] <= C.R_TOL and d["t"] <= C.KP_TOL and d["theta"] <= C.THETA_TOL
    _proper(got[sl(C.S_R, 9)], what)
    return state, got_tr, want_tr


def _incoming(case, prev_ok):
    state = case.state.clone()
    state[C.S_PREV:C.S_PREV + 16] = torch.linspace(0.004, 0.009, 16)  # a previous search size the smoothing can be seen to use
    state[C.S_PREV_OK] = float(prev_ok)
    return state.cuda()


@pytest.mark.parametrize("P", C.UPDATE_P)
def test_update_matches_the_reference(P):
    from hotrack_amd import ext
    case = C.update_case(P)
    kw, state0 = C.to_kernel(case), _incoming(case, 1)
    state, chain = state0, []
    for it in range(3):
        before = state
        state, tr, _ = _one_iteration(C.with_state(case, before), kw, before, f"P {P}, iteration {it}")
        chain.append(tr)
        if P == 1:  # nothing is better: only the search size and the success flag change
            assert float(tr[2]) == 0 and torch.equal(state[:C.S_SEARCH], before[:C.S_SEARCH])
            assert torch.equal(state[C.S_PREV:C.S_PREV_OK], before[C.S_PREV:C.S_PREV_OK]) and float(state[C.S_PREV_OK]) == 0
        elif it == 0:
            assert float(tr[2]) == 1
    whole = state0.clone()
    tr3 = ext.hand_pose_opt(state=whole, iterations=3, scaling_coefficient2=C.C2, beta=C.BETA, trace=True, **kw)
    assert torch.equal(whole, state) and torch.equal(tr3.cpu().double(), torch.stack(chain))


@pytest.mark.parametrize("prev_ok", [0, 1])
@pytest.mark.parametrize("P", [64, 1025])
def test_smoothing_follows_the_previous_success(P, prev_ok):
    case = C.update_case(P)
    before = _incoming(case, prev_ok)
    state, tr, _ = _one_iteration(C.with_state(case, before), C.to_kernel(case), before, f"P {P}, previous success {prev_ok}")
    assert float(tr[2]) == 1 and float(state[C.S_PREV_OK]) == 1
    other, _, _ = _one_iteration(C.with_state(case, _incoming(case, 1 - prev_ok)), C.to_kernel(case), _incoming(case, 1 - prev_ok),
                                 f"P {P}, previous success {1 - prev_ok}")
    assert torch.equal(state[:C.S_SEARCH], other[:C.S_SEARCH])                  # the pose does not depend on it,
    assert not torch.allclose(state[C.S_SEARCH:C.S_PREV], other[C.S_SEARCH:C.S_PREV], rtol=1e-3, atol=0)  # the search size does


@pytest.mark.parametrize("P,at", [(63, 62), (1025, 1024), (8192, 5000)])
def test_exactly_one_better_candidate(P, at):
    """Every row the current estimate except the case's best one, placed where a thread's second candidate (1024) or the last
    wave's lanes pick it up: the mean transform is that row's sample."""
    big = C.update_case(8192)
    best, _ = C.branch_rows(big)
    case = C.single_row_case(big, P, best, at)
    before = _incoming(case, 1)
    state, tr, _ = _one_iteration(C.with_state(case, before), C.to_kernel(case), before, f"one better candidate at {at} of {P}")
    assert float(tr[2]) == 1
    sample = C.candidate_samples(before.cpu(), case.pre)[at]
    assert float((state[C.S_T:C.S_T + 3].cpu().double() - (before[C.S_T:C.S_T + 3].cpu().double() + sample[4:7])).abs().max()) <= 1e-7


@pytest.mark.parametrize("P,at", [(5, 3), (1023, 700)])
def test_equal_and_worse_energies_are_not_better(P, at):
    """Every row the current estimate -- energies EQUAL to candidate 0's -- except the case's worst one: no success, and the
    state keeps its bits but for the search size and the success flag."""
    from hotrack_amd import ext
    big = C.update_case(8192)
    _, worst = C.branch_rows(big)
    case = C.single_row_case(big, P, worst, at)
    before = _incoming(case, 1)
    kw = C.to_kernel(case)
    energy, _, _ = ext.hand_pose_energy(state=before.clone(), **kw)
    e = energy.cpu()
    ties = [q for q in range(P) if q != at]
    assert torch.equal(e[ties].view(torch.int32), e[:1].view(torch.int32).expand(P - 1)) and float(e[at]) > float(e[0])
    state, tr, _ = _one_iteration(C.with_state(case, before), kw, before, f"ties and one worse candidate at {at} of {P}")
    assert float(tr[2]) == 0 and float(state[C.S_PREV_OK]) == 0
    assert torch.equal(state[:C.S_SEARCH], before[:C.S_SEARCH]) and torch.equal(state[C.S_PREV:C.S_PREV_OK], before[C.S_PREV:C.S_PREV_OK])
