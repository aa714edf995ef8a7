"""Builders and restatements for the IKNet kernel tests (hotrack_amd/csrc/iknet.hip): numpy only, nothing committed as data.

Everything is closed-form from a few integers (the lattice of tests/_iknet_cases.py).  Three kinds of weight sets:

  routing   every layer is an exact selection, so raw_quat is a known column of the kernel's own input pack, bit for bit;
  one dense one layer dense (lattice weights, part of the rows made to cancel), the others routing, so the dense layer's inputs
            are exact fp32 values and an a-priori bound on the fp32 dot product holds per output;
  table     wo = 0 and bo = one row of quat_table(): raw_quat == bo bit for bit, which drives the head's conversion.

quat_table reaches row variation by SEVERAL LAUNCHES (one per table row, each with its own M), not through the routing
weights: the bias delivers every quaternion exactly with no arithmetic in between, and the table stays a plain array."""
import numpy as np

from _iknet_cases import lattice

HID, KIN, K1, NOUT, NHID = 1024, 126, 128, 60, 5
PARENT = [0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
HID_K = (5, 77, 333, 509, 1021)      # hidden layer l routes neuron n to (HID_K[l] n + HID_O[l]) mod 1024: five different odd k
HID_O = (3, 100, 511, 7, 900)
U = 2.0 ** -24
F32 = np.float32
_CACHE = {}


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def keypoints(M: int, salt: int = 1):
    """kp (M,21,3) around (0,0,0.5), a fp32 rotation R (M,3,3) per row and a translation t (M,3,1) near the wrist."""
    kp = lattice((M, 21, 3), 7 * salt + 1, -0.1, 0.1) + np.array([0, 0, 0.5], F32)
    ax = lattice((M, 3), 7 * salt + 2, -1.0, 1.0).astype(np.float64) + np.array([0.05, 0.0, 0.0])
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    ang = lattice((M,), 7 * salt + 3, 0.2, 3.0).astype(np.float64)
    K = np.zeros((M, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    t = kp[:, 0] + lattice((M, 3), 7 * salt + 4, -0.01, 0.01)
    return kp.astype(F32), R.astype(F32), t.astype(F32).reshape(M, 3, 1)


def pack_fp32(kp, R, t, camera: bool) -> np.ndarray:
    """(M,126) the kernel's input pack, operation by operation in float32 (hand_frame and the bone rule of iknet.hip):
    coordinate-major [x0..x20, y0..y20, z0..z20 | bones], bone_k = kp_hf_k - kp_hf_parent(k)."""
    kp = np.asarray(kp, F32)
    M = kp.shape[0]
    if camera:
        hf = kp * F32(5.0)
    else:
        R, t = np.asarray(R, F32).reshape(M, 3, 3), np.asarray(t, F32).reshape(M, 1, 3)
        d = kp - t                                                      # (M,21,3), one rounding each
        hf = np.empty((M, 21, 3), F32)
        for a in range(3):                                              # ((r[a] d0 + r[3+a] d1) + r[6+a] d2) / 0.2f
            r0, r1, r2 = R[:, 0, a, None], R[:, 1, a, None], R[:, 2, a, None]
            hf[:, :, a] = ((r0 * d[:, :, 0] + r1 * d[:, :, 1]) + r2 * d[:, :, 2]) / F32(0.2)
    bone = hf - hf[:, PARENT]
    return np.concatenate([hf.transpose(0, 2, 1).reshape(M, 63), bone.transpose(0, 2, 1).reshape(M, 63)], 1).astype(F32)


# ---- routing weights -------------------------------------------------------------------------------------------------------
def _perm(l: int) -> np.ndarray:
    return (HID_K[l] * np.arange(HID) + HID_O[l]) % HID


def trace(n, after: int) -> np.ndarray:
    """Where the value of neuron n of layer `after` (0: layer 1, 1..5: the hidden layers) stands in the head's input when every
    later hidden layer routes."""
    n = np.asarray(n)
    for l in range(after, NHID):
        n = _perm(l)[n]
    return n


def _zero_set():
    return {"w1": np.zeros((HID, K1), F32), "b1": np.zeros(HID, F32), "wh": np.zeros((NHID, HID, HID), F32),
            "bh": np.zeros((NHID, HID), F32), "wo": np.zeros((NOUT, HID), F32), "bo": np.zeros(NOUT, F32)}


def _route_first(w):
    n = np.arange(1008)
    w["w1"][n, n % KIN] = np.where((n // KIN) % 2 == 0, 1.0, -1.0)


def _route_hidden(w, l):
    w["wh"][l][_perm(l), np.arange(HID)] = 1.0


def column_set(s: int) -> np.ndarray:
    """The pack column every head output reads in routing set s: sets 0, 1, 2 together cover all 126 columns."""
    return (np.arange(NOUT) + 60 * s) % KIN


def routing(s: int):
    """(weights, cols): raw_quat[m, o] = pack[m, cols[o]] exactly.  Layer-1 neuron c + 252 s carries relu(+pack[c]) and neuron
    c + 126 + 252 s carries relu(-pack[c]); the head subtracts the two where the hidden permutations have moved them."""
    w = _zero_set()
    _route_first(w)
    for l in range(NHID):
        _route_hidden(w, l)
    cols, o = column_set(s), np.arange(NOUT)
    w["wo"][o, trace(cols + 252 * s, 0)] = 1.0
    w["wo"][o, trace(cols + 126 + 252 * s, 0)] = -1.0
    return w, cols


def routing_expected(pack, s: int) -> np.ndarray:
    """Follows the selection, multiplies nothing."""
    return np.asarray(pack)[:, column_set(s)]


SELECTED = np.array([0, 1, 2, 3, 1020, 1021, 1022, 1023] + [(37 * i + 6) % 1016 + 4 for i in range(52)])


def bias_case(p: int):
    """(weights, expected (60,)): layer p's (0: b1, 1..5: bh[p-1]) weight is zero, its bias a lattice with both signs, the layers
    after it route, the head reads the SELECTED neurons: raw[m, o] = relu(bias[SELECTED[o]])."""
    w = _zero_set()
    bias = lattice((HID,), 300 + p, -1.0, 1.0)
    if p == 0:
        w["b1"][:] = bias
    else:
        _route_first(w)
        for l in range(p - 1):
            _route_hidden(w, l)
        w["bh"][p - 1] = bias
    for l in range(p, NHID):
        _route_hidden(w, l)
    w["wo"][np.arange(NOUT), trace(SELECTED, p)] = 1.0
    return w, np.maximum(bias[SELECTED], F32(0))


# ---- plain float64 forward -------------------------------------------------------------------------------------------------
def forward_fp64(w, pack):
    """relu(x W^T + b) six times and the head, in float64: [input of layer 1, ..., input of the head, raw]."""
    x = np.zeros((pack.shape[0], K1))
    x[:, :KIN] = pack
    acts = [x]
    x = np.maximum(x @ w["w1"].astype(np.float64).T + w["b1"].astype(np.float64), 0)
    for l in range(NHID):
        acts.append(x)
        x = np.maximum(x @ w["wh"][l].astype(np.float64).T + w["bh"][l].astype(np.float64), 0)
    acts.append(x)
    acts.append(x @ w["wo"].astype(np.float64).T + w["bo"].astype(np.float64))
    return acts


def dense_case(p: int, pack):
    """One dense layer at position p (0: layer 1, 1..5: hidden, 6: head), the others routing.  -> (weights, ref (M,60) float64,
    bound (M,60), ratio (M,60)) with bound = (K + 2) 2^-24 (sum |w x| + |b|) per output and ratio = sum |w x| / |sum w x|.

    Every second selected row is made to cancel against the exact input row (o mod M) of the dense layer: w <- v - ((v.x - tau)
    / x.x) x with tau = sum |v x| / 2000, so its dot product with that row is ~1/2000 of its absolute sum (and positive, so the
    ReLU lets it through); these rows carry no bias."""
    M = pack.shape[0]
    w = _zero_set()
    if p > 0:
        _route_first(w)
    for l in range(NHID):
        if l != p - 1:
            _route_hidden(w, l)
    # the exact input of the dense layer: a permutation of relu(+-pack), or the pack itself
    x = forward_fp64(w, pack)[p]
    K = K1 if p == 0 else HID
    rows = np.arange(NOUT) if p == 6 else SELECTED
    s = (6.0 / (KIN if p == 0 else HID)) ** 0.5
    W = lattice((NOUT if p == 6 else HID, K), 400 + p, -s, s).astype(np.float64)
    b = lattice((W.shape[0],), 420 + p, -0.05, 0.05)
    if p == 0:
        W[:, KIN:] = 0
    for o in range(0, NOUT, 2):
        r, xm = rows[o], x[o % M]
        v = W[r]
        tau = np.abs(v * xm).sum() / 2000.0
        W[r] = v - ((v @ xm - tau) / (xm @ xm)) * xm
        if p == 0:
            W[r, KIN:] = 0
        b[r] = 0
    W = W.astype(F32)
    if p == 0:
        w["w1"], w["b1"] = W, b
    elif p == 6:
        w["wo"], w["bo"] = W, b
    else:
        w["wh"][p - 1], w["bh"][p - 1] = W, b
    if p < 6:
        w["wo"][np.arange(NOUT), trace(SELECTED, p)] = 1.0
    W64, b64 = W.astype(np.float64)[rows], b.astype(np.float64)[rows]
    pre = x @ W64.T + b64
    ref = pre if p == 6 else np.maximum(pre, 0)
    absum = np.abs(x) @ np.abs(W64).T
    bound = (K + 2) * U * (absum + np.abs(b64))
    ratio = absum / np.maximum(np.abs(x @ W64.T), 1e-300)
    return w, ref, bound, ratio


def he_state():
    """Dense He-scaled weights: tests/_iknet_cases.py's state with its BatchNorm folded in float64 (eps 1e-5)."""
    from _iknet_cases import iknet_state
    sd = iknet_state()
    w = _zero_set()
    for i in range(6):
        g = sd[f"bn.{i}.weight"].astype(np.float64) / np.sqrt(sd[f"bn.{i}.running_var"].astype(np.float64) + 1e-5)
        W = sd[f"linear.{i}.weight"].astype(np.float64) * g[:, None]
        b = (sd[f"linear.{i}.bias"].astype(np.float64) - sd[f"bn.{i}.running_mean"]) * g + sd[f"bn.{i}.bias"]
        if i == 0:
            w["w1"][:, :KIN], w["b1"] = W.astype(F32), b.astype(F32)
        else:
            w["wh"][i - 1], w["bh"][i - 1] = W.astype(F32), b.astype(F32)
    w["wo"], w["bo"] = sd["linear.6.weight"], sd["linear.6.bias"]
    return w


# ---- the head's conversion -------------------------------------------------------------------------------------------------
RUNGS = 8
GENERIC = np.array([0.5, -0.3, 0.64, 0.5])   # a generic quaternion (norm ~ 1), scaled by 1e-6 and 1e6 below


def quat_table():
    """(table (16,15,4) float32, groups {name: bool mask (16,15)}).  Groups: 'identity' (+-(1,0,0,0) and the zero quaternion:
    theta must be 0), 'turns' ((0,1,0,0) and (-0.5,0.5,0.5,0.5)), 'near_identity' ((1,1e-9,0,0), (1,1e-4,0,0)), 'scaled'
    (GENERIC x 1e-6 and x 1e6), 'rung{k}+' / 'rung{k}-' (angle 10^-k about three axes, w = +-cos(a/2)), 'random' (not normalised)."""
    if "table" in _CACHE:
        return _CACHE["table"]
    q, names = [], []

    def add(name, v):
        q.append(np.asarray(v, np.float64))
        names.append(name)
    for v in ((1, 0, 0, 0), (-1, 0, 0, 0), (0, 0, 0, 0)):
        add("identity", v)
    for v in ((0, 1, 0, 0), (-0.5, 0.5, 0.5, 0.5)):
        add("turns", v)
    for v in ((1, 1e-9, 0, 0), (1, 1e-4, 0, 0)):
        add("near_identity", v)
    add("scaled", GENERIC * 1e-6)
    add("scaled", GENERIC * 1e6)
    axes = np.array([[1.0, 0, 0], [0.6, 0, -0.8], [2.0, -3.0, 6.0]])
    axes /= np.linalg.norm(axes, axis=-1, keepdims=True)
    for k in range(RUNGS):
        a = 10.0 ** -k
        for sign, tag in ((1.0, "+"), (-1.0, "-")):
            for ax in axes:
                add(f"rung{k}{tag}", np.concatenate([[sign * np.cos(a / 2)], np.sin(a / 2) * ax]))
    n = 16 * 15 - len(q)
    rnd = lattice((n, 4), 500, -2.0, 2.0)
    for v in rnd:
        add("random", v)
    # spread the kinds over the joints: slot i of the list -> (row, joint) by a stride coprime to 240
    table = np.zeros((240, 4), F32)
    name_at = [None] * 240
    for i, (v, nm) in enumerate(zip(q, names)):
        j = (i * 7) % 240
        table[j], name_at[j] = v.astype(F32), nm
    name_at = np.array(name_at).reshape(16, 15)
    groups = {nm: name_at == nm for nm in dict.fromkeys(names)}
    _CACHE["table"] = (table.reshape(16, 15, 4), groups)
    return _CACHE["table"]


def theta_fp64(raw) -> np.ndarray:
    """network/models/iknet.py::quat2axisang in float64 from the fp32 values: (..., 4) -> (..., 3)."""
    q = np.asarray(raw).astype(np.float64)
    q = q / (np.linalg.norm(q, axis=-1, keepdims=True) + 1e-8)
    cosa = q[..., 0]
    sina = np.sqrt(np.maximum(1 - cosa ** 2, 0))[..., None]
    axis = q[..., 1:] / np.maximum(sina, (sina < 1e-8).astype(np.float64))
    return axis * (2 * np.arccos(np.clip(cosa, -1, 1)))[..., None]


def head_fp32(raw):
    """The kernel's head operation by operation in float32 (numpy's arccos for acosf) -> (theta (...,3), s2, s, cw)."""
    q = np.asarray(raw, F32)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z) + F32(1e-8)
    cw, qx, qy, qz = w / nrm, x / nrm, y / nrm, z / nrm
    s2 = F32(1) - cw * cw
    s = np.where(s2 > 0, np.sqrt(np.maximum(s2, F32(0))), F32(0)).astype(F32)
    den = np.where(s < F32(1e-8), np.maximum(s, F32(1)), s).astype(F32)
    ang = F32(2) * np.arccos(np.clip(cw, F32(-1), F32(1)))
    th = np.stack([qx / den * ang, qy / den * ang, qz / den * ang], -1).astype(F32)
    return th, s2, s, cw


def theta_fp32(raw) -> np.ndarray:
    return head_fp32(raw)[0]


def head_tolerances():
    """{group: 4 x the worst |theta_fp32 - theta_fp64| of the group}, recomputed on every run; 0 means compare exactly."""
    table, groups = quat_table()
    err = np.abs(theta_fp32(table).astype(np.float64) - theta_fp64(table)).max(-1)
    return {nm: 4.0 * float(err[mask].max()) for nm, mask in groups.items()}
