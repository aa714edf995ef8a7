"""Frames, float64 references and float32 restatements for obj_pose_metrics_kernel (hotrack_amd/csrc/seq_eval.hip): numpy only.

Frames are built in float64, rounded to float32, and referenced in float64 FROM the float32 values.  frames(axis, sym) is one list
per symmetry mode; tile(frames, T) repeats it to T frames so the same frame lands in different workgroups and lanes."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
T_SIZES = (1, 63, 64, 65, 257)
FLIPS = {3: [(1, 1, 1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1)], -1: [(1, 1, 1), (-1, 1, -1)]}   # what rot_diff_rad minimises over
HALF_TURNS = [(1, -1, -1), (-1, 1, -1), (-1, -1, 1)]   # about x, y, z


def rot(axis, ang):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def frames(axis: int, sym: int):
    """{"gR","gt","pR","pt": float32 arrays (F,3,3) / (F,3), "kind": list of F names}.  The relative rotation of a ladder or
    threshold frame is about a body axis perpendicular to column `axis` in the axis modes (so the columns open by that angle),
    about a generic axis otherwise."""
    G = rot([0.3, -0.5, 0.8], 1.1)
    u = np.eye(3)[(axis + 1) % 3] if 0 <= axis <= 2 else np.array([0.36, 0.48, 0.8])
    t0 = np.array([0.02, -0.03, 0.5])
    gR, gt, pR, pt, kind = [], [], [], [], []

    def add(name, g, p, tg=t0, tp=t0 + np.array([0.003, 0.0, -0.004])):
        gR.append(np.asarray(g, np.float64).astype(F32))
        pR.append(np.asarray(p, np.float64).astype(F32))
        gt.append(np.asarray(tg, np.float64).astype(F32))
        pt.append(np.asarray(tp, np.float64).astype(F32))
        kind.append(name)
    for k in range(8):
        Gk = rot([0.1 * k - 0.3, 0.7, 0.2], 0.4 + 0.3 * k)
        add(f"rung{k}", Gk, Gk @ rot(u, 10.0 ** -k))
    G32 = G.astype(F32)
    add("identical", G32, G32)
    for s in HALF_TURNS:
        add("flip" + "".join("+" if v > 0 else "-" for v in s), G32, G32 * np.array(s, F32)[None, :])   # pred = gt diag(s), exact
    add("scaled", G * (1 + 1e-3), G * (1 + 1e-3))
    big = np.array([1000.25, -999.5, 1001.125])
    add("far", G, G @ rot(u, 0.3), big, big + np.array([1e-3, -1e-3, 1e-3]))
    for thr_deg, thr_m, tag in ((5.0, 0.05, "5"), (10.0, 0.10, "10")):
        for da in (-0.1, 0.1):
            for dm in (-0.001, 0.001):
                d = np.array([0.6, 0.0, 0.8]) * (thr_m + dm)
                add(f"thr{tag}{'+' if da > 0 else '-'}{'+' if dm > 0 else '-'}", G, G @ rot(u, np.deg2rad(thr_deg + da)), t0, t0 + d)
    for i in range(4):
        Gi = rot([0.5, 0.1 * i, -0.4], 2.0 + 0.2 * i)
        add("generic", Gi, Gi @ rot([0.2 * i - 0.3, 0.5, 0.4], 0.7 + 0.6 * i), t0, t0 + np.array([0.02 * i, 0.03, -0.01 * i]))
    return {"gR": np.stack(gR), "gt": np.stack(gt), "pR": np.stack(pR), "pt": np.stack(pt), "kind": kind}


def tile(fr, T: int):
    F = len(fr["kind"])
    idx = np.arange(T) % F
    return {k: np.ascontiguousarray(fr[k][idx]) for k in ("gR", "gt", "pR", "pt")}, idx


def _signs(axis):
    return FLIPS.get(axis, [(1, 1, 1)])


def cosines_fp64(fr, axis, sym):
    """(cos (F, n_flips) float64 before the clamp, absum (F, n_flips) = sum |a b| over the products the cosine is made of)."""
    a, b = fr["gR"].astype(np.float64), fr["pR"].astype(np.float64)
    if 0 <= axis <= 2:
        c = (a[:, :, axis] * b[:, :, axis]).sum(-1)
        return c[:, None], np.abs(a[:, :, axis] * b[:, :, axis]).sum(-1)[:, None]
    cs, ab = [], []
    for s in _signs(axis):
        prod = a * b * np.array(s, np.float64)[None, None, :]
        cs.append((prod.sum((1, 2)) - 1) / 2)
        ab.append(np.abs(prod).sum((1, 2)))
    return np.stack(cs, 1), np.stack(ab, 1)


def cosines_fp32(fr, axis, sym):
    """The kernel's cosine in its own sum order in float32 (before the clamp): the same bits under -ffp-contract=off."""
    a, b = fr["gR"].reshape(-1, 9), fr["pR"].reshape(-1, 9)
    if 0 <= axis <= 2:
        d = a[:, axis] * b[:, axis]
        d = d + a[:, 3 + axis] * b[:, 3 + axis]
        d = d + a[:, 6 + axis] * b[:, 6 + axis]
        return d[:, None]
    out = []
    for s in _signs(axis):
        s0, s1, s2 = (F32(v) for v in s)
        tr = np.zeros(a.shape[0], F32)
        for i in range(3):
            tr = tr + ((s0 * a[:, 3 * i] * b[:, 3 * i] + s1 * a[:, 3 * i + 1] * b[:, 3 * i + 1]) + s2 * a[:, 3 * i + 2] * b[:, 3 * i + 2])
        out.append((tr - F32(1)) / F32(2))
    return np.stack(out, 1)


def _angle_deg(c, sym, axis):
    c = np.clip(c, -1.0, 1.0)
    if sym and 0 <= axis <= 2:
        c = np.abs(c)
    return np.degrees(np.arccos(c)).min(-1)


def delta(axis):
    """The derived bound on the float32 cosine as a multiple of sum |a b|: the axis form is three products and two additions
    (<= 3 roundings deep, 4 with margin); the trace form nine products, eight additions, the subtraction of 1 and an exact
    halving (<= 7 deep on the trace, and |trace - 1| <= sum |a b| + 1 <= 4/3 sum |a b| + ..., covered by 11)."""
    return (4 if 0 <= axis <= 2 else 11) * U


def reference(fr, axis, sym):
    """float64 from the float32 values: {"td", "deg", "lo", "hi" (the interval of deg under the cosine bound), "flags" (F,2),
    "deg32" (float64 acos of the restated float32 cosine, in degrees)}."""
    c, ab = cosines_fp64(fr, axis, sym)
    d = delta(axis) * ab
    td = np.linalg.norm(fr["gt"].astype(np.float64) - fr["pt"].astype(np.float64), axis=-1)
    deg = _angle_deg(c, sym, axis)
    if sym and 0 <= axis <= 2:   # |cos|: the interval of |c| under +-d
        lo = _angle_deg(np.minimum(np.abs(c) + d, 1.0), 0, axis)
        hi = _angle_deg(np.maximum(np.abs(c) - d, 0.0), 0, axis)
    else:
        lo = _angle_deg(np.minimum(c + d, 1.0), sym, axis)
        hi = _angle_deg(np.maximum(c - d, -1.0), sym, axis)
    flags = np.stack([(deg <= 5.0) & (td <= 0.05), (deg <= 10.0) & (td <= 0.10)], -1).astype(F32)
    deg32 = _angle_deg(cosines_fp32(fr, axis, sym).astype(np.float64), sym, axis)
    return {"td": td, "deg": deg, "lo": lo, "hi": hi, "flags": flags, "deg32": deg32}


def ulps(x):
    """The float32 spacing at |x| (float64 array in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x)).astype(F32)).astype(np.float64)
