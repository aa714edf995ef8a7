"""CPU: the plain reference and the case table of the hand shape-code search kernel's float64 tests (tests/_hand_shape_cases.py).
`step` is anchored to gf_optimize_hand_shape._optimize_torch driving the hand model in float64, the affine basis to the model's
forward pass, and every case to its preconditions: each step well separated along the float64 trajectory, the four (previous
success, success) combinations, both outcomes of the first step and every listed P, D and T reached."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hand_shape_cases as C  # noqa: E402
from _hand_shape_cases import F32, F64  # noqa: E402
from models.hand_model import SyntheticLBSHand  # noqa: E402
from models.optimization_hand import gf_optimize_hand_shape, kp2length  # noqa: E402


def _basis_f64(hm):
    """The model's affine keypoint basis at the rest pose, in float64 end to end."""
    D = hm.num_betas
    betas = torch.cat([torch.zeros(1, D, dtype=F64), torch.eye(D, dtype=F64)])
    with torch.no_grad():
        _, kp = hm(th_pose_coeffs=torch.zeros(D + 1, 48, dtype=F64), th_betas=betas)
    return kp[0], kp[1:] - kp[0]


def test_affine_basis_holds_in_float64():
    hm = SyntheticLBSHand(num_betas=10)
    k0, k = _basis_f64(hm)
    beta = 3 * torch.randn(16, 10, generator=torch.Generator().manual_seed(0), dtype=F64)
    with torch.no_grad():
        _, kp = hm(th_pose_coeffs=torch.zeros(16, 48, dtype=F64), th_betas=beta)
    assert float((k0 + torch.einsum("pd,dkc->pkc", beta, k) - kp).abs().max()) < 1e-12
    assert float((C.bone_lengths(k0, k, beta) - kp2length(kp)).abs().max()) < 1e-12
    # the cases' float32 basis is this one, rounded: what gf_optimize_hand_shape.keypoint_basis hands the kernel
    assert torch.equal(C.model_basis()[0], k0.float()) and torch.equal(C.model_basis()[1], k.float())


@pytest.mark.parametrize("name,iterations", [("success-success", 8), ("fail-then-success", 6), ("row0-nonzero", 4), ("ties-fail", 3)])
def test_step_reproduces_the_torch_route_in_float64(name, iterations):
    """gf_optimize_hand_shape._optimize_torch on the CPU with the model, the candidates and the targets in float64 against `step`
    chained in float64 on the model's float64 basis: the final code and the whole trace."""
    case = C.get_case(name)
    hm = SyntheticLBSHand(num_betas=10)
    opt = gf_optimize_hand_shape({"device": "cpu"}, hand_model=hm, particle_size=case.P)
    opt.pre_sampled_particle, opt.initial_scale = case.pre.double(), case.initial_scale.double()
    opt.scaling_coefficient2, opt.beta, opt.iteration, opt.keep_trace = case.sc2, case.beta, iterations, True
    opt.hand_shape = torch.zeros(1, case.D, dtype=F64)
    opt.old_pred_length = case.targets.double()[None]
    opt._rest_pose = lambda n, device=None: torch.zeros((n, 48), dtype=F64)
    with torch.no_grad():
        want = opt._optimize_torch()
    assert want.dtype == F64 and opt.trace.dtype == F64 and opt.trace.shape == (iterations, 3 + case.D)
    c = C.SimpleNamespace(**vars(case))
    c.k0, c.k = _basis_f64(hm)
    got, trace, _ = C.run(c, F64, iterations)
    assert torch.equal(trace[:, 2], opt.trace[:, 2])
    assert float((got - want[0]).abs().max()) < 1e-10
    assert float((trace - opt.trace).abs().max()) < 1e-10


@pytest.mark.parametrize("name", C.CASES)
def test_every_step_is_well_separated(name):
    case = C.get_case(name)
    _, trace, seps = C.reference_run(name)
    assert len(seps) == case.iterations == trace.shape[0] and bool(torch.isfinite(trace).all())
    for i, (wsum, gap, origin) in enumerate(seps):
        assert C.well_separated(wsum, gap, origin, case.P), (name, i, wsum, gap, origin)
        assert (wsum > 0) == bool(trace[i, 2]), (name, i)


def test_float32_yardstick_follows_the_reference():
    """The same transcription in float32 takes the same branches and lands near the float64 run (it is the GPU test's yardstick)."""
    for name in ("P-1025", "D-16", "success-then-fail", "beta-1"):
        case = C.get_case(name)
        h32, t32, _ = C.run(case, F32)
        h64, t64, _ = C.reference_run(name)
        assert h32.dtype == F32 and t32.dtype == F32
        assert torch.equal(t32[:, 2].double(), t64[:, 2])
        assert float((t32[:, :2].double() - t64[:, :2]).abs().max()) < 1e-4 * float(t64[:, 0].max())
        assert float((h32.double() - h64).abs().max()) < 1e-2


def test_table_reaches_every_branch_and_size():
    seen, first = set(), set()
    for name in C.CASES:
        b = C.branches(C.reference_run(name)[1])
        seen.update(b)
        first.add(b[0][1])
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    assert first == {True, False}
    cases = [C.get_case(n) for n in C.CASES]
    assert {c.P for c in cases if (c.D, c.T) == (10, 3)} >= set(C.P_SWEEP) == {1, 2, 63, 64, 65, 1023, 1024, 1025, 5120, 8191, 8192}
    assert {c.D for c in cases if c.P == 1025} >= set(C.D_SWEEP) == {1, 2, 15, 16}
    assert {c.T for c in cases if c.P == 8192} >= set(C.T_SWEEP) == {1, 2, 500, 1023, 1024}
    assert all(1 <= c.P <= C.MAXP and 1 <= c.D <= C.MAXD and 1 <= c.T <= C.MAXT for c in cases)
    assert all(c.iterations <= 4 for c in cases if c.name != "production")
    # the smoothing constant acts only where both the previous and the current step succeed
    for name in ("beta-0", "beta-1"):
        assert (True, True) in C.branches(C.reference_run(name)[1]), name
    # dynamic LDS: the limit case takes 98.8 KB, and P = 8192 goes beyond 64 KB from T = 471
    assert C.lds_bytes(8192, 1024) == 98768 and C.lds_bytes(8192, 470) <= C.LDS_64K < C.lds_bytes(8192, 471)
    above = sorted(c.name for c in cases if c.lds > C.LDS_64K)
    assert above == ["T-1023", "T-1024", "T-500", "largest"]
    p = C.get_case("production")
    opt = gf_optimize_hand_shape({"device": "cpu"}, hand_model=SyntheticLBSHand(num_betas=10))
    assert (p.P, p.D, p.T, p.iterations, p.sc2, p.beta) == (5120, 10, 10, opt.iteration, opt.scaling_coefficient2, opt.beta) == \
        (5120, 10, 10, 20, 2000, 0.9)
    assert torch.equal(p.pre, opt.pre_sampled_particle) and torch.equal(p.initial_scale, opt.initial_scale)
    assert torch.equal(p.k0, C.model_basis()[0]) and torch.equal(p.k, C.model_basis()[1])


def test_tie_and_exact_cases_are_what_they_claim():
    # tie rows are bit-identical to row 0 and give its energy exactly, in either precision
    for name in ("ties", "ties-fail", "ties-at-end"):
        case = C.get_case(name)
        rows = list(case.ties) + list(range(case.P - case.ties_at_end, case.P))
        assert len(rows) == 7 and not case.pre[[0] + rows].any() and case.pre[1 if name == "ties-at-end" else 8].any()
        for dt in (F32, F64):
            _, e = C.energies(C.initial_state(case), case.k0, case.k, case.pre, case.targets, dt)
            assert bool((e[rows] == e[0]).all())
        bare = C.without_ties(case)
        assert bare.P == case.P - 7 and torch.equal(bare.pre[1:], case.pre[[p for p in range(1, case.P) if p not in rows]])
        h, tr, _ = C.reference_run(name)
        h2, tr2, _ = C.run(bare)
        assert float((h - h2).abs().max()) < 1e-12 and float((tr - tr2).abs().max()) < 1e-12
    assert torch.equal(C.without_ties(C.get_case("ties-at-end")).pre, C.get_case("ties-at-end").pre[:1025])
    assert not C.reference_run("ties-fail")[1][:, 2].any() and C.reference_run("ties")[1][0, 2] == 1
    # the dyadic hand: the rest lengths are exact, so the origin is exactly zero in either precision and every step fails
    case = C.get_case("rest-exact")
    l64 = C.bone_lengths(case.k0, case.k, torch.zeros(1, 10, dtype=F64))
    assert torch.equal(l64 * 1024, torch.round(l64 * 1024)) and torch.equal(case.targets.double(), l64.expand(3, -1))
    assert torch.equal(C.bone_lengths(case.k0, case.k, torch.zeros(1, 10)).double(), l64)
    for dt in (F32, F64):
        h, tr, _ = C.run(case, dt)
        assert not h.any() and not tr[:, :3].any() and bool((tr[:, 3:] == 1e-3).all())
    # a non-zero row 0: the origin is E[0] at that row's shape code, not at the current estimate
    case = C.get_case("row0-nonzero")
    assert case.pre[0].any()
    _, e = C.energies(C.initial_state(case), case.k0, case.k, case.pre, case.targets, F64)
    at = (C.bone_lengths(case.k0, case.k, (case.pre[0].double() * case.initial_scale.double())[None]) - case.targets.double()).abs().mean()
    assert abs(float(e[0] - at)) < 1e-15 and float(C.reference_run("row0-nonzero")[2][0][2]) == float(e[0])
