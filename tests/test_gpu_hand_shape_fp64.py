"""GPU: the hand shape-code search kernel (hotrack_amd/csrc/hand_shape.hip, pn2x_hand_shape_opt) against float64 over the range it
accepts -- the case table of tests/_hand_shape_cases.py: ragged and tiny candidate counts, D = 1..16, up to 1024 target rows (dynamic
LDS above 64 KB), every (previous success, success) combination of the update, exact ties, other length units, beta = 0 and 1.

The search cannot be started from a given state, but a k-iteration run is a bitwise prefix of an n-iteration run, so the kernel's
state after k steps is known from its own outputs.  Every step is then compared TEACHER-FORCED: `step` in float64 (the reference)
and in float32 (the yardstick) from the kernel's state after k - 1 steps, each quantity q in max-norm within

    |kernel - f64| <= 4 |f32 - f64| + 16 u max|q_f64|,   u = 2^-24

with the success flag equal exactly and every step well separated (a condition on the case, never a skip).  Run with -s to see every
ratio |kernel - f64| / (|f32 - f64| + floor) and the worst per quantity."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hand_shape_cases as C  # noqa: E402
from _hand_shape_cases import F32, F64, U  # noqa: E402

pytestmark = pytest.mark.gpu

PN2_OK, PN2_EINVAL, PN2_ENULL, PN2_ERANGE = 0, -1, -2, -3
_WORST = {}
_DEV = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for q, (ratio, where) in sorted(_WORST.items()):
        print(f"\nworst ratio {q}: {ratio:.3f} ({where})", end="")
    print()


def _dev(case):
    if case.name not in _DEV:
        _DEV[case.name] = tuple(x.cuda() for x in (case.k0, case.k, case.pre, case.targets, case.initial_scale))
    return _DEV[case.name]


def _launch(case, iterations, trace=True, out=None):
    from hotrack_amd import ext
    return ext.hand_shape_opt(*_dev(case), case.sc2, case.beta, iterations, out=out, trace=trace)


def _prefix_runs(case):
    """[(h, trace)] of the runs with 1..n iterations on the CPU, the prefix property asserted bitwise."""
    runs = [_launch(case, k) for k in range(1, case.iterations + 1)]
    torch.cuda.synchronize()
    runs = [(h.cpu(), tr.cpu()) for h, tr in runs]
    full = runs[-1][1]
    assert full.shape == (case.iterations, 3 + case.D) and bool(torch.isfinite(full).all())
    for k, (h, tr) in enumerate(runs, 1):
        assert h.shape == (case.D,) and bool(torch.isfinite(h).all())
        assert torch.equal(tr, full[:k]), f"{case.name}: the {k}-iteration trace is no prefix of the {case.iterations}-iteration trace"
    return runs


def _within(where, q, got, f32, f64):
    got, f32, f64 = (torch.as_tensor(v).double().reshape(-1) for v in (got, f32, f64))
    err, yard = float((got - f64).abs().max()), float((f32 - f64).abs().max())
    floor = 16 * U * float(f64.abs().max())
    ratio = err / (yard + floor) if yard + floor > 0 else (0.0 if err == 0 else math.inf)
    print(f"{where} {q}: |kernel - f64| = {err:.3e}, |f32 - f64| = {yard:.3e}, floor = {floor:.3e}, ratio = {ratio:.3f}")
    if ratio > _WORST.get(q, (-1.0, ""))[0]:
        _WORST[q] = (ratio, where)
    assert err <= 4 * yard + floor, f"{where} {q}: {err:.3e} beyond 4 x {yard:.3e} + {floor:.3e}"


def _check_step(case, where, state, row, h_k, reference=None):
    """One teacher-forced step from `state` (the kernel's own) against trace row `row` and the code `h_k` after it.  `reference`:
    the case whose float64 / float32 steps are the reference (the case itself unless given)."""
    ref = reference or case
    args = (ref.k0, ref.k, ref.pre, ref.targets)
    ev = C.energies(state, *args, F64)
    wsum, gap, origin = C.separation(state, *args, _evaluated=ev)
    assert C.well_separated(wsum, gap, origin, ref.P), f"{where}: not well separated (wsum {wsum:.3e}, gap {gap:.3e}, origin {origin:.3e})"
    s64, (o64, m64, ok64) = C.step(state, *args, ref.sc2, ref.beta, F64, _evaluated=ev)
    s32, (o32, m32, ok32) = C.step(state, *args, ref.sc2, ref.beta, F32)
    assert float(row[2]) in (0.0, 1.0) and bool(row[2]) == ok64 == ok32, f"{where}: success {float(row[2])}, float64 {ok64}, float32 {ok32}"
    _within(where, "origin", row[0], o32, o64)
    _within(where, "mean_e", row[1], m32, m64)
    _within(where, "search", row[3:], s32[1], s64[1])
    _within(where, "h", h_k, s32[0], s64[0])
    if not ok64:
        assert row[1] == row[0] and torch.equal(h_k, state[0]), f"{where}: a failed step moved the code or the mean energy"
    return ok64


def _teacher_forced(case, runs):
    state = C.initial_state(case)
    taken = []
    for k, (h_k, tr) in enumerate(runs, 1):
        row = tr[k - 1]
        ok = _check_step(case, f"{case.name} step {k}", state, row, h_k)
        taken.append((bool(state[3]), ok))
        search = row[3:].clone()
        state = (h_k, search, search if ok else state[2], ok)
    return taken


@pytest.mark.parametrize("name", C.CASES)
def test_teacher_forced_parity_with_float64(name):
    case = C.get_case(name)
    taken = _teacher_forced(case, _prefix_runs(case))
    # the kernel took the branches the table was built for
    assert taken == C.branches(C.reference_run(name)[1])


def test_one_candidate_never_moves():
    """P = 1: 15 of the 16 waves have no candidate and candidate 0 is never better than itself."""
    case = C.get_case("P-1")
    runs = _prefix_runs(case)
    h, tr = runs[-1]
    assert not h.any() and not tr[:, 2].any() and torch.equal(tr[:, 1], tr[:, 0])
    state = C.initial_state(case)
    for k, row in enumerate(tr, 1):
        (_, s64, _, _), (o64, _, _) = C.step(state, case.k0, case.k, case.pre, case.targets, case.sc2, case.beta, F64)
        (_, s32, _, _), (o32, _, _) = C.step(state, case.k0, case.k, case.pre, case.targets, case.sc2, case.beta, F32)
        want = o64 * case.sc2 / math.sqrt(case.D) + 1e-3
        assert float((s64 - want).abs().max()) <= 1e-14 * float(want)
        _within(f"P-1 step {k}", "search", row[3:], s32, want.expand(case.D))
        _within(f"P-1 step {k}", "origin", row[0], o32, o64)
        state = (runs[k - 1][0], row[3:].clone(), state[2], False)


def test_zero_origin_fails_every_step_exactly():
    """Targets that are the rest lengths exactly (a hand whose bone lengths are exact in float32): the origin is exactly zero,
    nothing is better, the code stays exactly zero and every search size is exactly 1e-3."""
    case = C.get_case("rest-exact")
    h, tr = _prefix_runs(case)[-1]
    assert not h.any() and not tr[:, :3].any()
    assert torch.equal(tr[:, 3:], torch.full((case.iterations, case.D), 1e-3, dtype=F32))


def test_tie_rows_count_for_nothing():
    """Zero rows of `pre` tie with candidate 0 exactly: they are not better and carry no weight.
    Appended after the other rows they leave every candidate on its thread and summation slot, so the result is bitwise the
    result without them.  As rows 1..7 they move every later candidate to another lane, and a wave's butterfly sums in another
    order: there the run is held to the float64 step of the case WITHOUT the rows by the file's tolerance, the success flag
    (the count of better candidates) exactly -- on a first step that succeeds, and on one where nothing but the ties could."""
    end = C.get_case("ties-at-end")
    bare = C.without_ties(end)
    bare.name = "ties-at-end-removed"
    for k in (1, end.iterations):
        (h, tr), (h0, tr0) = _launch(end, k), _launch(bare, k)
        assert torch.equal(h, h0) and torch.equal(tr, tr0)
    for name, flag in (("ties", True), ("ties-fail", False)):
        case = C.get_case(name)
        h, tr = _launch(case, 1)
        ok = _check_step(case, f"{name} without its tie rows, step 1", C.initial_state(case), tr[0].cpu(), h.cpu(),
                         reference=C.without_ties(case))
        assert ok == flag


def test_largest_case_is_deterministic_and_runs_on_a_side_stream():
    case = C.get_case("largest")
    assert (case.P, case.D, case.T) == (C.MAXP, C.MAXD, C.MAXT) and case.lds > C.LDS_64K
    _dev(case)
    torch.cuda.synchronize()
    h0, tr0 = _launch(case, case.iterations)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        h1, tr1 = _launch(case, case.iterations)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(h0, h1) and torch.equal(tr0, tr1) and bool(torch.isfinite(tr0).all())


def _raw(case, p=None, d=None, t=None, iterations=1, out=None, null=()):
    """The raw C entry with the case's (valid) device buffers; `null`: argument names passed as NULL."""
    from hotrack_amd import ext
    k0, k, pre, targets, init = _dev(case)
    ptr = {"k0": k0, "k": k, "pre": pre, "targets": targets, "initial_scale": init, "out": out}
    ptr = {n: (None if n in null or v is None else v.data_ptr()) for n, v in ptr.items()}
    return ext._lib.pn2x_hand_shape_opt(case.P if p is None else p, case.D if d is None else d, case.T if t is None else t, iterations,
                                        ptr["k0"], ptr["k"], ptr["pre"], ptr["targets"], ptr["initial_scale"], ctypes.c_double(case.sc2),
                                        ctypes.c_double(case.beta), ptr["out"], None, torch.cuda.current_stream().cuda_stream)


def test_no_iterations_is_the_zero_code():
    from hotrack_amd import ext
    case = C.get_case("P-65")
    h, tr = _launch(case, 0)
    assert h.shape == (case.D,) and not h.any() and tr.shape == (0, 3 + case.D)
    mine = torch.full((case.D,), 7.0, device="cuda")
    h, tr = _launch(case, 0, trace=False, out=mine)
    assert h is mine and tr is None and not mine.any()
    # the C entry: no launch, PN2_OK, the caller's buffer as it was -- with or without buffers
    mine.fill_(7.0)
    assert _raw(case, iterations=0, out=mine) == PN2_OK
    assert _raw(case, iterations=0, null=("k0", "k", "pre", "targets", "initial_scale", "out")) == PN2_OK
    torch.cuda.synchronize()
    assert bool((mine == 7.0).all())
    assert ext.hand_shape_opt_supported(case.P, case.D, case.T)


def test_rejected_calls_leave_no_error_pending():
    """Every rejection happens before anything is launched: the wrapper raises, the C entry returns its code, and afterwards the
    device synchronises and a valid call gives the answer it gave before.  Every pointer passed is a valid device buffer or NULL."""
    from hotrack_amd import ext
    case = C.get_case("P-65")
    k0, k, pre, targets, init = _dev(case)
    want = tuple(x.clone() for x in _launch(case, case.iterations))
    out = torch.full((case.D,), 7.0, device="cuda")

    def still_sound():
        torch.cuda.synchronize()
        got = _launch(case, case.iterations)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool((out == 7.0).all())

    def z(*shape):
        return torch.zeros(*shape, device="cuda")

    wrapper = {"P = 8193": (k0, k, z(8193, 10), targets, init),
               "D = 17": (k0, z(17, 21, 3), z(64, 17), targets, z(17)),
               "T = 1025": (k0, k, pre, z(1025, 15), init),
               "k of another D": (k0, k[:9].contiguous(), pre, targets, init),
               "k0 of 20 keypoints": (k0[:20].contiguous(), k, pre, targets, init),
               "targets of 14 bones": (k0, k, pre, z(3, 14), init),
               "1-d targets": (k0, k, pre, z(15), init),
               "initial_scale of another D": (k0, k, pre, targets, z(9))}
    for what, args in wrapper.items():
        with pytest.raises(ValueError):
            ext.hand_shape_opt(*args, case.sc2, case.beta, 2, out=out if what != "D = 17" else None)
        still_sound()
    raw = [(dict(p=8193), PN2_ERANGE), (dict(d=17), PN2_ERANGE), (dict(t=1025), PN2_ERANGE),
           (dict(p=0), PN2_EINVAL), (dict(d=0), PN2_EINVAL), (dict(t=0), PN2_EINVAL), (dict(p=-1), PN2_EINVAL),
           (dict(iterations=-1), PN2_EINVAL), (dict(null=("k0",)), PN2_ENULL), (dict(null=("out",)), PN2_ENULL)]
    for kw, code in raw:
        assert _raw(case, out=out, **kw) == code, kw
        still_sound()
    assert not ext.hand_shape_opt_supported(8193, 10, 1) and not ext.hand_shape_opt_supported(64, 17, 1)
    assert not ext.hand_shape_opt_supported(64, 10, 1025) and ext.hand_shape_opt_supported(8192, 16, 1024)
