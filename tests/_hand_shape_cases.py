"""Seeded cases and a plain reference for the hand shape-code search kernel (hotrack_amd/csrc/hand_shape.hip) over the range
pn2x_hand_shape_opt_supported accepts: P = 1..8192 candidates, D = 1..16 shape dimensions, T = 1..1024 target rows.  Everything
here runs on the CPU; tests/test_hand_shape_cases.py anchors `step` to gf_optimize_hand_shape._optimize_torch and checks every
case's preconditions, tests/test_gpu_hand_shape_fp64.py runs the kernel.

  step          one iteration of the search written out plainly (gf_optimize_hand_shape._optimize_torch with kp2length's energy on
                the affine keypoint basis), in float64 (the reference) or float32 (the yardstick)
  separation    how far one step is from the edge between success and failure, in float64
  CASES         the table: name -> how P, D, T, the basis, the candidates, the targets and the constants are made from a seed

A step is WELL SEPARATED when float32 rounding of the energies cannot change its success flag: either the weights of the better
candidates add up to 1e3 P u origin or more (u = 2^-24), or no candidate is better and the nearest one that is not an exact tie is
1e3 u origin or more away.  Exact ties are bit-identical rows of `pre`: they give bit-identical energies in any arithmetic."""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from models.hand_model import SyntheticLBSHand  # noqa: E402
from models.optimization_hand import _BONE, _PARENT, gf_optimize_hand_shape  # noqa: E402

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
SEPARATION = 1e3
MAXP, MAXD, MAXT = 8192, 16, 1024
LDS_64K = 64 * 1024


def lds_bytes(P, T):
    """The kernel's dynamic LDS (hand_shape.hip, lds_bytes): energies, targets, the bone basis, the per-wave partials, their
    totals and the iteration state."""
    return 4 * (P + 15 * T + 45 * (MAXD + 1) + 16 * (MAXD + 3) + (MAXD + 3) + 3 * MAXD + 4)


# ---- one iteration -------------------------------------------------------------------------------------------------------------
def bone_lengths(k0, k, x):
    """kp2length of kp = k0 + sum_d x_d k[d]: (P, D) shape codes -> (P, 15), in x's dtype."""
    kp = k0.to(x.dtype) + torch.einsum("pd,dkc->pkc", x, k.to(x.dtype))
    return torch.norm(kp[:, _BONE] - kp[:, _PARENT], dim=-1)


def energies(state, k0, k, pre, targets, dtype):
    """-> (sample (P, D), energy (P,)) of one iteration in `dtype`: the mean over the 15 bones, then over the T target rows."""
    h, search = state[0].to(dtype), state[1].to(dtype)
    sample = pre.to(dtype) * search
    length = bone_lengths(k0, k, h + sample)
    tg = targets.to(dtype)
    rows = max(1, (1 << 22) // (15 * tg.shape[0]))  # a (rows, T, 15) temporary of at most 4M entries
    energy = torch.cat([(c[:, None, :] - tg[None]).abs().mean(dim=-1).mean(dim=-1) for c in length.split(rows)])
    return sample, energy


def step(state, k0, k, pre, targets, sc2, beta, dtype, _evaluated=None):
    """One iteration of gf_optimize_hand_shape._optimize_torch from state = (h (D,), search (D,), prev_search (D,), prev_success)
    -> (new state, (origin, mean_e, success)), everything in `dtype`."""
    h, search, prev_search, prev_success = state
    h, prev_search = h.to(dtype), prev_search.to(dtype)
    sample, energy = _evaluated if _evaluated is not None else energies(state, k0, k, pre, targets, dtype)
    origin = energy[0]
    better = energy < origin
    weight = (origin - energy) * better
    success = bool(better.any())
    if success:
        wsum = weight.sum()
        mean_e = (energy * weight).sum() / wsum
        mt = (sample * weight[:, None]).sum(dim=0) / wsum
        h = h + mt
    else:
        mean_e, mt = origin, torch.zeros_like(h)
    s = mt.abs() + 1e-3
    new_search = mean_e * sc2 * s / s.norm() + 1e-3
    if bool(prev_success) and success:
        new_search = beta * new_search + (1 - beta) * prev_search
    if success:
        prev_search = new_search
    return (h, new_search, prev_search, success), (origin, mean_e, success)


def separation(state, k0, k, pre, targets, _evaluated=None):
    """One step in float64 -> (wsum, gap, origin): the sum of the better candidates' weights, and the smallest E_p - origin over
    the candidates p >= 1 that are not exact ties with candidate 0 (inf when there is none)."""
    _, energy = _evaluated if _evaluated is not None else energies(state, k0, k, pre, targets, F64)
    origin = energy[0]
    diff = energy[1:] - origin
    diff = diff[diff != 0]
    wsum = float((-diff[diff < 0]).sum())
    return wsum, (float(diff.min()) if diff.numel() else float("inf")), float(origin)


def well_separated(wsum, gap, origin, P):
    if wsum > 0:
        return wsum >= SEPARATION * P * U * origin
    return gap >= SEPARATION * U * origin


def initial_state(case):
    s = case.initial_scale
    return (torch.zeros_like(s), s, s, True)


def run(case, dtype=F64, iterations=None):
    """`step` chained from the initial state -> (final h, trace rows [origin, mean_e, success, search...], separations)."""
    state, rows, seps = initial_state(case), [], []
    for _ in range(case.iterations if iterations is None else iterations):
        ev = energies(state, case.k0, case.k, case.pre, case.targets, dtype)
        if dtype == F64:
            seps.append(separation(state, case.k0, case.k, case.pre, case.targets, _evaluated=ev))
        state, (origin, mean_e, success) = step(state, case.k0, case.k, case.pre, case.targets, case.sc2, case.beta, dtype, _evaluated=ev)
        rows.append(torch.cat([torch.stack([origin, mean_e, torch.tensor(float(success), dtype=dtype)]), state[1]]))
    trace = torch.stack(rows) if rows else torch.zeros(0, 3 + case.D, dtype=dtype)
    return state[0].to(dtype), trace, seps


# ---- the material of the cases ---------------------------------------------------------------------------------------------------
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def model_basis():
    """(k0 (21,3), k (10,21,3)) float32: SyntheticLBSHand(num_betas=10)'s affine keypoint basis at the rest pose, the one
    gf_optimize_hand_shape.keypoint_basis hands the kernel."""
    def make():
        hm = SyntheticLBSHand(num_betas=10)
        k0, k = hm.shape_keypoint_basis(torch.zeros(1, 3 + hm.num_pose))
        return k0.contiguous(), k.contiguous()
    return _memo("model_basis", make)


def synthetic_basis(D, seed):
    """The model's rest keypoints with D random directions of about 3 mm per unit of the code (the wrist stays put)."""
    g = torch.Generator().manual_seed(7000 + seed)
    k = 0.003 * torch.randn(D, 21, 3, generator=g)
    k[:, 0] = 0
    return model_basis()[0], k.contiguous()


def dyadic_hand():
    """A hand whose bone lengths come out exactly in any arithmetic: every bone vector is (3a, 4a, 0) / 1024 or (0, 4a, 3a) / 1024
    with a small integer a (its length 5a / 1024), a the nearest to the model's own bone.  Differences, squares, their sum and the
    square root are all exact in float32, with or without fused multiply-adds."""
    def make():
        rest = model_basis()[0].double()
        k0 = torch.zeros(21, 3, dtype=F64)
        for f, chain in enumerate(SyntheticLBSHand.FINGERS):
            parent = 0
            for j in chain:
                a = float(torch.round((rest[j] - rest[parent]).norm() * 1024 / 5))
                v = (0.0, 4 * a, 3 * a) if f == 2 else ((3 * a if f > 2 else -3 * a), 4 * a, 0.0)
                k0[j] = k0[parent] + torch.tensor(v, dtype=F64) / 1024
                parent = j
        return k0.float().contiguous()
    return _memo("dyadic_hand", make)


def pre_rows(P, D, seed):
    """The first P rows and D columns of 8192 x 16 seeded N(0, I) draws, row 0 the current estimate."""
    pre = _memo(("pre", seed), lambda: torch.randn(MAXP, MAXD, generator=torch.Generator().manual_seed(3000 + seed)))
    pre = pre[:P, :D].clone()
    pre[0] = 0
    return pre.contiguous()


def make_case(name, P, D, T, seed, iterations=4, basis="model", pre="normal", targets="noisy", initial_scale=5.0, sc2=2000.0,
              beta=0.9, scale=1.0, truth=1.0, noise=2e-5, cluster=0.02, row0=None, ties=(), ties_at_end=0):
    """A case from seeds, CPU float32 tensors: k0 (21,3), k (D,21,3), pre (P,D), targets (T,15), initial_scale (D,).
    basis    "model" (D = 10: SyntheticLBSHand's), "synthetic" (any D), "dyadic" (the model's directions on dyadic_hand())
    targets  "noisy": the bone lengths at a seeded shape code beta* ~ truth N(0, I), each row with N(0, noise^2) added;
             "rest": every row the bone lengths at the zero code, exactly
    pre      "normal": seeded N(0, I) rows; "toward" / "away": rows clustered (`cluster`) around +beta* / initial_scale or
             -beta* / initial_scale, so that the first step's candidates all sit near beta* or all on the far side of the origin;
             "optimiser": gf_optimize_hand_shape's own pre_sampled_particle
    row0     None: a zero row (the current estimate); a number: row 0 is that multiple of a seeded N(0, I) row
    ties     rows set to zero (exact ties with a zero row 0); ties_at_end: that many zero rows appended after the P rows
    scale    k0, k and the targets multiplied by it (lengths in other units)."""
    g = torch.Generator().manual_seed(seed)
    if basis == "model":
        assert D == 10
        k0, k = model_basis()
    elif basis == "dyadic":
        assert D == 10
        k0, k = dyadic_hand(), model_basis()[1]
    else:
        k0, k = synthetic_basis(D, seed)
    k0, k = (k0.double() * scale).float().contiguous(), (k.double() * scale).float().contiguous()
    beta_true = truth * torch.randn(D, generator=g, dtype=F64)
    if targets == "rest":
        tg = bone_lengths(k0, k, torch.zeros(1, D, dtype=F64)).expand(T, -1)
    else:
        tg = bone_lengths(k0, k, beta_true[None]) + scale * noise * torch.randn(T, 15, generator=g, dtype=F64)
    init = torch.full((D,), float(initial_scale))
    if pre == "optimiser":
        opt = gf_optimize_hand_shape({"device": "cpu"}, hand_model=SyntheticLBSHand(num_betas=10), particle_size=P)
        rows, init = opt.pre_sampled_particle.clone(), opt.initial_scale.clone()
    elif pre == "normal":
        rows = pre_rows(P, D, seed)
    else:
        sign = 1.0 if pre == "toward" else -1.0
        rows = (sign * beta_true / initial_scale)[None].float() + cluster * pre_rows(P, D, seed)
        rows[0] = 0
    if row0 is not None:
        rows[0] = row0 * torch.randn(D, generator=g)
    for r in ties:
        rows[r] = 0
    if ties_at_end:
        rows = torch.cat([rows, torch.zeros(ties_at_end, D)])
    return SimpleNamespace(name=name, P=rows.shape[0], D=D, T=T, iterations=iterations, k0=k0, k=k, pre=rows.contiguous(),
                           targets=tg.float().contiguous(), initial_scale=init.float().contiguous(), sc2=float(sc2), beta=float(beta),
                           ties=tuple(ties), ties_at_end=ties_at_end, beta_true=beta_true, lds=lds_bytes(rows.shape[0], T))


def without_ties(case):
    """The case with its tie rows taken out and P reduced accordingly."""
    keep = [p for p in range(case.P - case.ties_at_end) if p not in case.ties]
    c = SimpleNamespace(**vars(case))
    c.pre, c.P, c.ties, c.ties_at_end = case.pre[keep].contiguous(), len(keep), (), 0
    return c


# ---- the table -----------------------------------------------------------------------------------------------------------------
P_SWEEP = (1, 2, 63, 64, 65, 1023, 1024, 1025, 5120, 8191, 8192)
D_SWEEP = (1, 2, 15, 16)
T_SWEEP = (1, 2, 500, 1023, 1024)
TIE_ROWS = tuple(range(1, 8))


def case_specs():
    s = {}

    def add(name, P, D, T, seed, **kw):
        s[name] = dict(P=P, D=D, T=T, seed=seed, **kw)

    for P in P_SWEEP:
        add(f"P-{P}", P, 10, 3, 1)
    for D in D_SWEEP:
        add(f"D-{D}", 1025, D, 3, 1 if D == 1 else 2, basis="synthetic", initial_scale=1.0)
    for T in T_SWEEP:
        add(f"T-{T}", 8192, 10, T, 2, iterations=4 if T <= 2 else 2)
    add("largest", 8192, 16, 1024, 4, iterations=2, basis="synthetic", initial_scale=1.0)
    add("row0-nonzero", 1025, 10, 3, 8, row0=0.3)
    add("ties", 1032, 10, 3, 3, ties=TIE_ROWS, initial_scale=1.0)
    add("ties-at-end", 1025, 10, 3, 3, ties_at_end=7, initial_scale=1.0)
    add("ties-fail", 1032, 10, 3, 6, pre="away", ties=TIE_ROWS)
    add("rest-exact", 768, 10, 3, 7, basis="dyadic", targets="rest")
    add("fail-then-success", 1025, 10, 3, 8, initial_scale=50.0)
    add("success-then-fail", 1025, 10, 3, 9, pre="toward")
    add("success-success", 768, 10, 3, 7, initial_scale=1.0)
    add("fail-fail", 1025, 10, 3, 11, pre="away")
    add("scale-1e-2", 1025, 10, 3, 1, scale=1e-2)
    add("scale-1e2", 1025, 10, 3, 1, scale=1e2, sc2=20.0)
    add("beta-0", 1025, 10, 3, 19, beta=0.0, initial_scale=1.0)
    add("beta-1", 1025, 10, 3, 19, beta=1.0, initial_scale=1.0)
    add("production", 5120, 10, 10, 2, iterations=20, pre="optimiser", noise=2e-4)
    return s


CASES = tuple(case_specs())


def get_case(name):
    """A table case by name, built once (the cases are read-only)."""
    return _memo(("case", name), lambda: make_case(name, **case_specs()[name]))


def reference_run(name):
    """run(get_case(name)) in float64, computed once and shared."""
    return _memo(("run", name), lambda: run(get_case(name)))


def branches(trace):
    """[(previous success, success)] of a trace, the first step's previous success being True."""
    flags = [True] + [bool(v) for v in trace[:, 2].tolist()]
    return list(zip(flags[:-1], flags[1:]))
