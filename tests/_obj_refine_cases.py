"""The object-pose Gauss-Newton refinement (include/pn2_sdf.h: pn2s_obj_refine), restated in numpy from the rule in the header and
at the head of hotrack_amd/csrc/sdf_refine.hip -- numpy only.

`evaluate`, `solve6`, `apply_step` and `refine_np` take the arithmetic as a parameter: with dtype float64 they are the rule in exact-ish
arithmetic (plain sums, no rounding order to mimic); with dtype float32 every operation is rounded once, the fused multiply-adds
are where the rule has them (emulated through a float64 product, exact for float32 operands) and the sums run in the kernel's
order (per lane, xor butterfly per wave, the four waves in order).  One text for both is a shortcut: the two do not check each
other's formulas, only each other's rounding.  What checks the formulas is the finite-difference test of the Jacobian and the
convergence test in tests/test_obj_refine_cases.py.

Volumes are the LINEAR res^3 arrays; the eight corner values are gathered by Distance's index arithmetic, which is what the
corner layout holds.  `CASES` is the table the CPU and GPU tests walk; `build(case)` makes a case's arrays; `trace_of(case)` its
float64 free-running trace.
"""
from __future__ import annotations

import numpy as np

from _obj_opt_cases import distance64  # noqa: F401  (the clamped Distance the residual is compared with)
from _sdf_cases import _axis_angle, make_volume, object_points, random_pose

F32, F64 = np.float32, np.float64
LANES, WAVE = 256, 64
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, EPS = 1e-3, 1e-7, 1e7, 1e-5
MIN_GAIN = 1e-3
TRACE_ROW = 72
BBOX_MIN = -0.2


def tri(k, l):
    return k * 6 - k * (k - 1) // 2 + (l - k)


TRI = [(k, l) for k in range(6) for l in range(k, 6)]


def _fma(a, b, c, dt):
    if dt is F64:
        return a * b + c
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ---- one pass: steps 1-7 ---------------------------------------------------------------------------------------------------------
def points(cam, pose, vol, res, stride, band, dt, bbox_min=BBOX_MIN):
    """Per point: q (n,3), u (n,3) unclamped grid coordinates, r0 the unclamped sample, g (n,3), J (n,6), valid, w -- all in dt."""
    cam = np.asarray(cam, F32).astype(dt).reshape(-1, 3)
    pose = np.asarray(pose).astype(dt).reshape(12)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    vol = np.asarray(vol).astype(dt).reshape(-1)
    s, b0, top = dt(F32(stride)), dt(F32(bbox_min)), dt(res - 1)
    e = cam - t
    q = np.stack([_fma(e[:, 2], R[2, j], _fma(e[:, 1], R[1, j], e[:, 0] * R[0, j], dt), dt) for j in range(3)], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (q - b0) / s
        inside = np.all((u > 0) & (u < top), axis=1)
        c = np.minimum(np.maximum(np.where(np.isnan(u), dt(0), u), dt(0)), top)
        i = c.astype(np.int64)
        f = c - i.astype(dt)
        x, y, z = f[:, 0], f[:, 1], f[:, 2]
        mx, my, mz = dt(1) - x, dt(1) - y, dt(1) - z
        i000 = (i[:, 0] * res + i[:, 1]) * res + i[:, 2]
        last, rr = vol.shape[0] - 1, res * res
        d = [vol[np.minimum(i000 + off, last)] for off in (0, 1, res, 1 + res, rr, 1 + rr, res + rr, 1 + res + rr)]
        c00, c01, c10, c11 = d[0] * mz + d[1] * z, d[2] * mz + d[3] * z, d[4] * mz + d[5] * z, d[6] * mz + d[7] * z
        r0 = (c00 * my + c01 * y) * mx + (c10 * my + c11 * y) * x
        g = np.stack([((c10 - c00) * my + (c11 - c01) * y) / s,
                      ((c01 - c00) * mx + (c11 - c10) * x) / s,
                      (((d[1] - d[0]) * my + (d[3] - d[2]) * y) * mx + ((d[5] - d[4]) * my + (d[7] - d[6]) * y) * x) / s], axis=1)
        J = np.empty((cam.shape[0], 6), dt)
        J[:, 0] = g[:, 1] * q[:, 2] - g[:, 2] * q[:, 1]
        J[:, 1] = g[:, 2] * q[:, 0] - g[:, 0] * q[:, 2]
        J[:, 2] = g[:, 0] * q[:, 1] - g[:, 1] * q[:, 0]
        for k in range(3):
            J[:, 3 + k] = -_fma(R[k, 2], g[:, 2], _fma(R[k, 1], g[:, 1], R[k, 0] * g[:, 0], dt), dt)
        a = np.abs(r0)
        bd = dt(F32(band))
        knee = bd * dt(0.5)
        valid = inside & (a < bd)
        w = np.where(valid, np.where(a <= knee, dt(1), knee / np.where(a > 0, a, dt(1))), dt(0))
    return dict(q=q, u=u, f=f, r0=r0, g=g, J=J, valid=valid, w=w, inside=inside)


def _kernel_order_sum(terms):
    """terms (n,29) float32 -> (29,) float32 summed as the kernel does: lane l takes points l, l + 256, ... in order; per wave the
    xor butterfly 32, 16, .., 1; then the four waves in order."""
    n = terms.shape[0]
    rows = -(-n // LANES)
    pad = np.zeros((rows * LANES, terms.shape[1]), F32)
    pad[:n] = terms
    pad = pad.reshape(rows, LANES, -1)
    acc = np.zeros((LANES, terms.shape[1]), F32)
    for r in range(rows):
        acc = acc + pad[r]
    v = acc.reshape(LANES // WAVE, WAVE, -1)
    lane = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ m]
    out = v[0, 0]
    for wv in range(1, LANES // WAVE):
        out = out + v[wv, 0]
    return out


def evaluate(cam, pose, vol, res, stride, band, dt, exclude=None):
    """One pass -> T (29,): A (21, rows of the upper triangle), b (6), E, n; and the per-point record.  `exclude`: a boolean mask of
    points left out of every sum (the GPU test's sensitive points)."""
    P = points(cam, pose, vol, res, stride, band, dt)
    valid = P["valid"] if exclude is None else P["valid"] & ~exclude
    w = np.where(valid, P["w"], dt(0))
    r = np.where(valid, P["r0"], dt(0))
    J = np.where(valid[:, None], P["J"], dt(0))
    v = w[:, None] * J
    terms = np.empty((J.shape[0], 29), dt)
    for (k, l) in TRI:
        terms[:, tri(k, l)] = v[:, k] * J[:, l]
    for k in range(6):
        terms[:, 21 + k] = v[:, k] * r
    terms[:, 27] = (w * r) * r
    terms[:, 28] = valid.astype(dt)
    T = _kernel_order_sum(terms) if dt is F32 else terms.sum(axis=0)
    return T, P


def cost_of(T, dt):
    return T[27] / max(T[28], dt(1))


# ---- steps 8-9 ------------------------------------------------------------------------------------------------------------------
def solve6(S, lam, eps_n, dt, e_acc=0.0):
    """(A + lam diag A + eps_n I) delta = -b by the rule's Cholesky -> (delta (6,), ok, the damped matrix (6,6))."""
    L = np.zeros((6, 6), dt)
    M = np.zeros((6, 6), dt)
    for (k, l) in TRI:
        M[k, l] = M[l, k] = S[tri(k, l)]
    ok = True
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(6):
            M[k, k] = _fma(dt(lam), S[tri(k, k)], S[tri(k, k)], dt) + dt(eps_n)
        for k in range(6):
            s = M[k, k]
            for m in range(k):
                s = s - L[k, m] * L[k, m]
            ok = ok and bool(s > 0)
            p = np.sqrt(s)
            L[k, k] = p
            for i in range(k + 1, 6):
                e = M[k, i]
                for m in range(k):
                    e = e - L[i, m] * L[k, m]
                L[i, k] = e / p
        y = np.zeros(6, dt)
        for k in range(6):
            e = -S[21 + k]
            for m in range(k):
                e = e - L[k, m] * y[m]
            y[k] = e / L[k, k]
        delta = np.zeros(6, dt)
        for k in range(5, -1, -1):
            e = y[k]
            for m in range(k + 1, 6):
                e = e - L[m, k] * delta[m]
            delta[k] = e / L[k, k]
    gain = dt(0)
    for k in range(6):
        gain = gain - S[21 + k] * delta[k]
    ok = ok and bool(np.all(np.abs(delta) < np.inf)) and bool(gain >= dt(F32(MIN_GAIN)) * dt(e_acc))
    return delta, ok, M


def _normalize3(v, dt):
    mag = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return v / mag if mag > dt(1e-8) else np.array([1, 0, 0], dt)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def apply_step(P, delta, dt):
    """pose' = (ortho6d(R exp([omega]x)), t + dt)."""
    P = np.asarray(P).astype(dt)
    o = np.asarray(delta).astype(dt)[:3]
    th2 = _fma(o[2], o[2], _fma(o[1], o[1], o[0] * o[0], dt), dt)
    th = np.sqrt(th2)
    if th2 < dt(1e-6):
        sa, ca = dt(1) - th2 / dt(6), dt(0.5) - th2 / dt(24)
    else:
        h = np.sin(dt(0.5) * th)
        sa, ca = np.sin(th) / th, dt(2) * h * h / th2
    dg = dt(1) - ca * th2
    c = ca * o
    K = np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], dt)
    dR = np.empty((3, 3), dt)
    for i in range(3):
        for j in range(3):
            dR[i, j] = dg + c[i] * o[j] if i == j else c[i] * o[j] + sa * K[i, j]
    R = P[:9].reshape(3, 3)
    Rn = np.empty((3, 3), dt)
    for i in range(3):
        for j in range(3):
            Rn[i, j] = _fma(R[i, 2], dR[2, j], _fma(R[i, 1], dR[1, j], R[i, 0] * dR[0, j], dt), dt)
    x = _normalize3(Rn[0], dt)
    z = _normalize3(_cross(x, Rn[1]), dt)
    y = _cross(z, x)
    return np.concatenate([x, y, z, P[9:] + np.asarray(delta).astype(dt)[3:]]).astype(dt)


def refine_np(cam, pose, vol, stride, iters=8, band=0.02, dt=F64):
    """The whole rule, free running -> (pose (12,), stats (8,), trace (iters + 1, TRACE_ROW)), all dt."""
    res = round(np.asarray(vol).size ** (1.0 / 3.0))
    cand = np.asarray(pose).astype(dt).reshape(12)
    P, S = cand.copy(), np.zeros(27, dt)
    lam, c_acc, n_acc, c_0, n_0, steps, stepped = dt(LAMBDA0), dt(0), dt(0), dt(0), dt(0), 0, False
    trace = np.zeros((iters + 1, TRACE_ROW), dt)
    for it in range(iters + 1):
        T, _ = evaluate(cam, cand, vol, res, stride, band, dt)
        cnt, cost = T[28], cost_of(T, dt)
        first = it == 0
        accept = first or (stepped and bool(cost <= c_acc) and bool(cnt >= dt(0.5) * n_acc))
        if stepped:
            lam = max(lam / dt(3), dt(LAMBDA_MIN)) if accept else min(lam * dt(10), dt(LAMBDA_MAX))
            steps += int(accept)
        if accept:
            P, S, c_acc, n_acc = cand.copy(), T[:27].copy(), cost, cnt
        if first:
            c_0, n_0 = cost, cnt
        decided, lam_solve, ok, delta = stepped, lam, False, np.zeros(6, dt)
        C = cand.copy()
        if it < iters:
            delta, ok, _ = solve6(S, lam, dt(EPS) * max(n_acc, dt(1)), dt, c_acc * max(n_acc, dt(1)))
            ok = ok and bool(n_acc >= 6)
            if ok:
                cand = apply_step(P, delta, dt)
            else:
                lam, cand, delta = min(lam * dt(10), dt(LAMBDA_MAX)), P.copy(), np.zeros(6, dt)
            stepped = ok
        row = trace[it]
        row[:12], row[12], row[13], row[14], row[15] = P, lam, c_acc, n_acc, float(accept)
        row[16:28], row[28:55], row[55], row[56], row[57], row[58], row[59] = C, T[:27], cost, cnt, lam_solve, float(ok), float(decided)
        row[60:66] = delta
    stats = np.array([c_0, c_acc, n_0, n_acc, steps, lam, 0, 0], dt)
    return P, stats, trace


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# res / stride pairs that keep the +-0.2 m box of Distance (bbox_min = -0.2): stride = 0.4 / (res - 1)
STRIDES = {9: 0.05, 17: 0.025, 41: 0.01}
DEFAULTS = dict(shape="box", res=41, f16=True, iters=8, band=0.02, angle=0.02, trans=0.004, noise=0.0015, special=None)


def _case(name, n, seed, **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, name=name, n=n, seed=seed, **kw)


CASES = (
    _case("n1", 1, 1),                                              # under-determined: no step, pose untouched
    _case("n5", 5, 2),                                              # under-determined
    _case("n63", 63, 3),
    _case("n64", 64, 4, f16=False),
    _case("n65", 65, 5),
    _case("n1024_box", 1024, 6),
    _case("n1024_box_f32", 1024, 6, f16=False),
    _case("n1500_wraps", 1500, 7),                                  # the lane stride wraps five times, the last row partial
    _case("res17_sphere", 257, 8, res=17, shape="sphere", band=0.05),
    _case("res9_sphere_f32", 300, 9, res=9, shape="sphere", f16=False, band=0.05),
    _case("iters0", 256, 10, iters=0),
    _case("iters1", 256, 11, iters=1),
    _case("outside_band", 200, 12, special="far"),                  # every point beyond the band: count 0, pose bit-equal
    _case("on_border", 200, 13, special="border"),                  # every point in the volume's clamped border
    _case("nan_cell", 512, 14, special="nan"),                      # one NaN voxel under the cloud
    _case("at_optimum", 512, 15, angle=0.0, trans=0.0),
    _case("first_step_rejected", 9, 65, angle=0.2, trans=0.015, band=0.03),      # (searched on the CPU: the cost rises by 37 %)
    _case("capsule", 1000, 17, shape="capsule"),                    # the rotation about the axis is unobservable
)


def build(case):
    """-> dict(cam (n,3) f32, pose (12,) f32, vol (res^3,) f16|f32 linear, res, stride, true (12,) f64)."""
    seed, n, res = case["seed"], case["n"], case["res"]
    stride = STRIDES[res]
    vol = make_volume(res, stride, case["shape"], np.float16 if case["f16"] else np.float32).copy()
    pc = object_points(seed, n, case["shape"], noise=case["noise"]).astype(F64)
    rng = np.random.default_rng(seed + 7000)
    if case["special"] == "border":      # beyond the +-0.2 m box on one axis at least: the grid coordinate clamps
        pc = rng.uniform(-0.19, 0.19, (n, 3))
        pc[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.201, 0.3, n)
    if case["special"] == "far":         # the surface scaled by 1.6: every point at least 3 cm outside the box, inside the volume
        pc = pc * 1.6
    R0, t0 = random_pose(seed + 1000)
    cam = (pc @ R0.astype(F64).T + t0).astype(F32)
    if case["special"] == "nan":         # the voxel nearest to point 0: the cells round it sample a NaN
        i = np.clip(np.rint((pc[0] - BBOX_MIN) / stride).astype(int), 0, res - 1)
        vol[(i[0] * res + i[1]) * res + i[2]] = np.nan
    Ri, ti = R0.astype(F64), t0.astype(F64)
    if case["angle"]:
        Ri = Ri @ _axis_angle(rng.standard_normal(3), case["angle"])
    if case["trans"]:
        v = rng.standard_normal(3)
        ti = ti + v / np.linalg.norm(v) * case["trans"]
    pose = np.concatenate([Ri.reshape(9), ti]).astype(F32)
    return dict(cam=cam, pose=pose, vol=vol, res=res, stride=stride, true=np.concatenate([R0.astype(F64).reshape(9), t0.astype(F64)]))


_traces = {}


def trace_of(case, dt=F64):
    """(pose, stats, trace) of the free-running restatement, computed once per process."""
    key = (case["name"], dt)
    if key not in _traces:
        a = build(case)
        _traces[key] = refine_np(a["cam"], a["pose"], a["vol"], a["stride"], case["iters"], case["band"], dt)
    return _traces[key]


def pose_error(pose, true):
    """(rotation angle in rad, translation distance in m) between two 12-vectors."""
    Ra, Rb = np.asarray(pose, F64)[:9].reshape(3, 3), np.asarray(true, F64)[:9].reshape(3, 3)
    cos = np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)
    return float(np.arccos(cos)), float(np.linalg.norm(np.asarray(pose, F64)[9:] - np.asarray(true, F64)[9:]))


# ---- teacher forcing: a trace's own states, every step recomputed in float64 -----------------------------------------------------
COND_MAX = 1e5      # the step is compared only where the float64 condition number of the damped matrix is below this: fp32's
#                     6e-8 then leaves |delta| about 1e-2 relative, which the measured tolerance has to cover and no more
QUANTITIES = ("A", "b", "cost", "delta", "pose")


def sensitive_points(P64, P32, band):
    """A point whose float64 |r| lies within the float32 restatement's error (over the cloud) of the band or the knee, or whose grid
    coordinate lies within that error of a cell face."""
    r64, r32 = P64["r0"], P32["r0"].astype(F64)
    both = np.isfinite(r64) & np.isfinite(r32)
    err_r = np.abs(r32 - r64)[both].max(initial=0.0)
    fin = np.isfinite(P64["u"]) & np.isfinite(P32["u"])
    err_u = np.abs(P32["u"].astype(F64) - P64["u"])[fin].max(initial=0.0)
    a, b = np.abs(r64), float(F32(band))
    with np.errstate(invalid="ignore"):
        near_r = (np.abs(a - b) <= err_r) | (np.abs(a - 0.5 * b) <= err_r)
        near_face = (np.abs(P64["u"] - np.rint(P64["u"])) <= err_u).any(axis=1)
    return near_r | near_face


def teacher_forced(case, trace):
    """For every row of `trace` (the kernel's, or a restatement's): the float64 values of what the row holds, from the row's own
    float32 states.  -> list of dicts: T (29,) of the row's candidate with the sensitive points left out of both sides' count
    comparison (`n_sensitive` says how many), delta and next candidate from the row's accepted pose and lambda (None after the last
    pass or where the row took no step), cond, and `gap`, the float64 cost difference its decision rests on."""
    a = build(case)
    trace = np.asarray(trace, F64)
    out, T_of = [], {}
    for k, row in enumerate(trace):
        cand = row[16:28].astype(F32)
        P64 = points(a["cam"], cand, a["vol"], a["res"], a["stride"], case["band"], F64)
        P32 = points(a["cam"], cand, a["vol"], a["res"], a["stride"], case["band"], F32)
        sens = sensitive_points(P64, P32, case["band"])
        T, _ = evaluate(a["cam"], cand, a["vol"], a["res"], a["stride"], case["band"], F64)
        T_of[cand.tobytes()] = T
        S = T_of[row[:12].astype(F32).tobytes()]          # the accepted pose was a candidate of this or an earlier row
        rec = dict(T=T, n_sensitive=int(sens.sum()), delta=None, next=None, cond=np.inf,
                   gap=abs(cost_of(T, F64) - trace[k - 1, 13]) if k and row[59] else None)
        if k < len(trace) - 1:
            delta, ok, M = solve6(S[:27], row[57], F64(F32(EPS)) * max(S[28], 1.0), F64, S[27])
            rec["cond"] = np.linalg.cond(M) if np.all(np.isfinite(M)) else np.inf
            rec["ok64"] = ok and S[28] >= 6
            if row[58]:
                rec["delta"], rec["next"] = delta, apply_step(row[:12].astype(F32), row[60:66].astype(F32), F64)
        out.append(rec)
    return out


def deviations(case, trace):
    """The largest |trace - float64| per quantity over the rows of one trace (teacher forced), the share of sensitive points and the
    numbers of decisions and of sensitive ones (for a given cost tolerance: see `sensitive_decisions`)."""
    trace = np.asarray(trace, F64)
    recs = teacher_forced(case, trace)
    dev = dict.fromkeys(QUANTITIES, 0.0)
    share = 0.0
    for k, (row, rec) in enumerate(zip(trace, recs)):
        if rec["n_sensitive"] == 0:       # (a sensitive point may sit on either side of the band in the two arithmetics)
            dev["A"] = max(dev["A"], np.abs(row[28:49] - rec["T"][:21]).max())
            dev["b"] = max(dev["b"], np.abs(row[49:55] - rec["T"][21:27]).max())
            dev["cost"] = max(dev["cost"], abs(row[55] - cost_of(rec["T"], F64)))
        share = max(share, rec["n_sensitive"] / len(build(case)["cam"]))
        if rec["delta"] is not None and rec["cond"] < COND_MAX:
            dev["delta"] = max(dev["delta"], np.abs(row[60:66] - rec["delta"]).max())
        if rec["next"] is not None:
            dev["pose"] = max(dev["pose"], np.abs(trace[k + 1, 16:28] - rec["next"]).max())
    return dev, share, recs


def measured_tolerances():
    """4 x the worst |float32 restatement - float64| of each quantity over the case list, and the worst share of sensitive points."""
    worst, share = dict.fromkeys(QUANTITIES, 0.0), {}
    for case in CASES:
        dev, sh, _ = deviations(case, trace_of(case, F32)[2])
        share[case["name"]] = sh
        for q in QUANTITIES:
            worst[q] = max(worst[q], dev[q])
    return {q: 4 * v for q, v in worst.items()}, share
