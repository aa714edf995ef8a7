"""Cases and restatements for the TSDF fusion tests (hotrack_amd/csrc/tsdf_fuse.hip, network/models/shape_fusion.py).  Not a test file.

`fuse_fp64` restates the rule of include/pn2_sdf.h (pn2s_tsdf_integrate) in float64 numpy, written from the rule alone, and marks
the voxels whose result hangs on a discontinuous choice (the pixel, the truncation gates, the camera plane).  `fuse_fp32` restates
the KERNEL's arithmetic operation by operation in float32 (fmaf as a float64 product and sum rounded once more to float32: exact
but for a rare double rounding, which only matters for the error figures it is used for).  The tolerance the routes are held to
is 4 x the worst |fp32 - fp64| over the case list, recomputed on every run (`tolerances`); fp16 volumes add half an fp16 ulp at
trunc (the priors of the cases are truncated at +-trunc, so no fused value exceeds it).

Scene of every case, camera frame, metres: the synthetic capsule (radius 0.04, core 0.14) at the frame's pose, sphere-traced per
pixel; a background plane at z = 0.9 behind it (so free space is carved); a hand blob (sphere, radius 0.03) in front of part of
it (occluder pixels are only ever free space); holes of zero depth on a lattice; one NaN depth (fp32 depth only)."""
import numpy as np

S_FLIP = np.diag([1.0, -1.0, -1.0])


def capsule_sdf(p, radius=0.04):
    z = np.clip(p[..., 2], -0.07, 0.07)
    return np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2 + (p[..., 2] - z) ** 2) - radius


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def render(R, t, K, h, w, hand=True):
    """depth (h,w) float64 (0 = nothing) and label (h,w): 0 background plane, 1 hand, 2 object."""
    fx, fy, cx, cy = K
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)   # z = 1: the parameter is the depth
    speed = np.linalg.norm(ray, axis=-1)
    z = np.full((h, w), 0.02)
    hit = np.zeros((h, w), dtype=bool)
    for _ in range(200):   # sphere tracing of the capsule
        p = (ray * z[..., None] - t) @ R   # object frame
        d = capsule_sdf(p)
        hit |= d < 1e-9
        z = np.where(hit | (z > 2.0), z, z + d / speed)
    depth = np.full((h, w), 0.9)
    label = np.zeros((h, w), dtype=np.int64)
    obj = hit & (z < 0.9)
    depth[obj], label[obj] = z[obj], 2
    if hand:   # a sphere between the camera and the capsule's +x side (object frame)
        c = R @ np.array([0.03, 0.0, 0.03]) + t
        c = c * 0.6
        b = (ray * c).sum(-1)
        a = (ray * ray).sum(-1)
        disc = b * b - a * ((c * c).sum() - 0.03 ** 2)
        zh = (b - np.sqrt(np.maximum(disc, 0))) / a
        hnd = (disc > 0) & (zh > 0.01) & (zh < depth)
        depth[hnd], label[hnd] = zh[hnd], 1
    return depth, label


# res, voxel_scale, (h, w), volume dtype, depth 'f32' / 'u16', seg factor, seg channels, flip, poses (names), max_weight, carve, prior W
CASES = [
    dict(name="res5_f32", res=5, scale=0.06, hw=(24, 32), vol="float32", depth="f32", f=1, c=3, flip=False, poses=["front"], max_w=64.0, carve=1.0, prior_w=1.0),
    dict(name="res17_f16_flip_F3", res=17, scale=0.016, hw=(24, 32), vol="float16", depth="f32", f=1, c=3, flip=True, poses=["front", "side", "top"], max_w=64.0, carve=1.0, prior_w=2.0),
    dict(name="res33_u16_seg2_F3", res=33, scale=0.008, hw=(48, 64), vol="float32", depth="u16", f=2, c=3, flip=False, poses=["front", "oblique", "side"], max_w=64.0, carve=1.0, prior_w=1.0),
    dict(name="res33_f16_u16_flip", res=33, scale=0.008, hw=(48, 64), vol="float16", depth="u16", f=1, c=1, flip=True, poses=["oblique"], max_w=64.0, carve=1.0, prior_w=8.0),
    dict(name="res17_saturate", res=17, scale=0.016, hw=(48, 64), vol="float32", depth="f32", f=2, c=3, flip=True, poses=["front", "front", "oblique"], max_w=3.0, carve=1.0, prior_w=2.0),
    dict(name="res33_close_F3", res=33, scale=0.008, hw=(24, 32), vol="float32", depth="f32", f=1, c=3, flip=False, poses=["close", "front", "close2"], max_w=64.0, carve=0.5, prior_w=1.0),
    dict(name="res5_f16_u16_F3", res=5, scale=0.06, hw=(48, 64), vol="float16", depth="u16", f=1, c=3, flip=False, poses=["close", "side", "front"], max_w=64.0, carve=1.0, prior_w=0.0),
    dict(name="res17_u16_carve0", res=17, scale=0.016, hw=(24, 32), vol="float32", depth="u16", f=1, c=1, flip=False, poses=["close2"], max_w=64.0, carve=0.0, prior_w=1.0),
    # a segment factor that is no power of two (the kernels divide where the factors 1 and 2 above shift: csrc/frame_device.h)
    dict(name="res17_u16_seg3_F2", res=17, scale=0.016, hw=(24, 33), vol="float32", depth="u16", f=3, c=3, flip=False, poses=["front", "oblique"], max_w=64.0, carve=1.0, prior_w=1.0),
]
DEPTH_SCALE = 0.001
MAX_EXCLUDED = 0.02

_POSES = {   # (R, t): q = R p + t; the volume spans +-0.13 m round the object
    "front": (_rot([1, 0, 0], 0.3), [0.01, -0.005, 0.32]),
    "side": (_rot([0, 1, 0], 1.4) @ _rot([1, 0, 0], 0.2), [-0.02, 0.01, 0.30]),
    "top": (_rot([1, 0, 0], 1.5), [0.0, 0.02, 0.35]),
    "oblique": (_rot([1, 2, 3], 2.1), [0.03, 0.02, 0.28]),
    "close": (_rot([0, 1, 0], np.pi / 2), [0.0, 0.01, 0.10]),      # the capsule's axis along camera x: part of the volume behind the camera
    "close2": (_rot([1, 0, 0], np.pi / 2) @ _rot([0, 0, 1], 0.4), [0.06, 0.0, 0.09]),
}


def build(case):
    """The inputs of a case as numpy arrays (what both restatements and, converted, both routes take)."""
    h, w = case["hw"]
    K = np.array([1.25 * w, 1.25 * w, (w - 1) / 2 + 0.3, (h - 1) / 2 - 0.2])
    F = len(case["poses"])
    depth, seg, rot, trans = [], [], [], []
    for k, name in enumerate(case["poses"]):
        R, t = _POSES[name]
        R, t = np.asarray(R, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)   # fp32-exact poses
        d, label = render(R, t, K, h, w)
        d[(np.arange(h)[:, None] * 7 + np.arange(w)[None, :] * 3 + k) % 23 == 0] = 0.0   # holes
        d = d.astype(np.float32)
        if case["depth"] == "u16":
            d = np.clip(np.rint(d.astype(np.float64) / DEPTH_SCALE), 0, 65535).astype(np.uint16)
        else:
            d[h // 2, w // 3] = np.nan
        f = case["f"]
        low = label[::f, ::f]
        if case["c"] == 3:
            s = np.zeros(low.shape + (3,), dtype=np.uint8)
            s[..., 0][low == 1] = 255
            s[..., 1][low == 2] = 255
        else:
            s = low.astype(np.uint8)[..., None]
        if case["flip"]:
            R, t = S_FLIP @ R, S_FLIP @ t
        depth.append(d), seg.append(s), rot.append(R.astype(np.float32)), trans.append(t.astype(np.float32))
    res, scale = case["res"], case["scale"]
    trunc = 3 * scale if res > 5 else 0.05
    ax = (np.arange(res) - res // 2) * scale
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)
    vol = np.clip(capsule_sdf(g, 0.03), -trunc, trunc).astype(case["vol"])
    return dict(volume=vol, weight=np.full((res,) * 3, case["prior_w"], dtype=np.float32), voxel_scale=scale, depth=np.stack(depth),
                seg=np.stack(seg), intrinsics=np.tile(K.astype(np.float32), (F, 1)), rotation=np.stack(rot), translation=np.stack(trans),
                trunc=trunc, obj_class=(1, 255) if case["c"] == 3 else (0, 2), depth_scale=DEPTH_SCALE if case["depth"] == "u16" else None,
                flip_yz=case["flip"], carve_weight=case["carve"], max_weight=case["max_w"])


def fuse_fp64(a):
    """-> (V, W, compare): the rule in float64 from the fp32-exact inputs, and the voxels that are compared."""
    vol = a["volume"]
    res = vol.shape[0]
    V, W = vol.astype(np.float64).reshape(-1), a["weight"].astype(np.float64).reshape(-1)
    V, W = V.copy(), W.copy()
    scale, trunc = float(np.float32(a["voxel_scale"])), float(np.float32(a["trunc"]))
    carve, max_w = float(np.float32(a["carve_weight"])), float(np.float32(a["max_weight"]))
    idx = np.arange(res) - res // 2
    gx, gy, gz = np.meshgrid(idx, idx, idx, indexing="ij")
    p = np.stack([gx, gy, gz], axis=-1).reshape(-1, 3).astype(np.float64) * scale
    compare = np.ones(res ** 3, dtype=bool)
    F, H, Wd = a["depth"].shape
    Hs, Ws, C = a["seg"].shape[1:]
    f = H // Hs
    channel, value = a["obj_class"]
    for k in range(F):
        R, t = a["rotation"][k].astype(np.float64), a["translation"][k].astype(np.float64)
        fx, fy, cx, cy = a["intrinsics"][k].astype(np.float64)
        q = p @ R.T + t
        if a["flip_yz"]:
            q = q * np.array([1.0, -1.0, -1.0])
        compare &= ~(np.abs(q[:, 2] - 1e-6) < 1e-4)
        front = q[:, 2] > 1e-6
        zs = np.where(front, q[:, 2], 1.0)
        pu, pv = q[:, 0] / zs * fx + cx, q[:, 1] / zs * fy + cy
        for x in (pu, pv):   # within 1e-3 pixel of a half-integer (the image border is one)
            frac = x - np.floor(x)
            compare &= ~(front & (np.abs(frac - 0.5) < 1e-3))
        u, v = np.rint(pu), np.rint(pv)
        ok = front & (u >= 0) & (u <= Wd - 1) & (v >= 0) & (v <= H - 1)
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        D = a["depth"][k][vi, ui]
        D = D.astype(np.float64) * a["depth_scale"] if a["depth_scale"] is not None else D.astype(np.float64)
        ok &= np.isfinite(D) & (D > 0)
        D = np.where(ok, D, 1.0)
        obj = a["seg"][k][vi // f, ui // f, channel] == value
        d = D - q[:, 2]
        compare &= ~(ok & (np.abs(d + trunc) < 1e-5) & obj)
        compare &= ~(ok & (np.abs(d - trunc) < 1e-5) & ~obj)
        upd = ok & np.where(obj, d >= -trunc, d > trunc)
        s = np.where(obj, np.minimum(d, trunc), trunc)
        g = np.where(obj, 1.0, carve)
        upd &= g != 0
        Wn = W + g
        with np.errstate(invalid="ignore", divide="ignore"):
            Vn = (V * W + s * g) / Wn
        V = np.where(upd, Vn, V)
        W = np.where(upd, np.minimum(Wn, max_w), W)
    return V.reshape(vol.shape), W.reshape(vol.shape), compare.reshape(vol.shape)


def _fma(x, y, z):
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def fuse_fp32(a):
    """The kernel's arithmetic in float32 -> (V, W, touched) with V NOT yet rounded to the volume's type."""
    f32 = np.float32
    vol = a["volume"]
    res = vol.shape[0]
    V, W = vol.astype(f32).reshape(-1).copy(), a["weight"].astype(f32).reshape(-1).copy()
    scale, trunc, carve, max_w = f32(a["voxel_scale"]), f32(a["trunc"]), f32(a["carve_weight"]), f32(a["max_weight"])
    idx = (np.arange(res) - res // 2).astype(f32)
    gx, gy, gz = (x.reshape(-1) * scale for x in np.meshgrid(idx, idx, idx, indexing="ij"))
    touched = np.zeros(res ** 3, dtype=bool)
    F, H, Wd = a["depth"].shape
    Hs, Ws, C = a["seg"].shape[1:]
    f = H // Hs
    channel, value = a["obj_class"]
    with np.errstate(all="ignore"):
        for k in range(F):
            R, t = a["rotation"][k].astype(f32), a["translation"][k].astype(f32)
            fx, fy, cx, cy = a["intrinsics"][k].astype(f32)
            q = [_fma(np.broadcast_to(R[i, 2], gz.shape), gz, _fma(np.broadcast_to(R[i, 0], gx.shape), gx,
                                                                     _fma(np.broadcast_to(R[i, 1], gy.shape), gy, np.broadcast_to(t[i], gy.shape))))
                 for i in range(3)]
            if a["flip_yz"]:
                q[1], q[2] = -q[1], -q[2]
            front = q[2] > f32(1e-6)
            u, v = np.rint(q[0] / q[2] * fx + cx), np.rint(q[1] / q[2] * fy + cy)
            assert u.dtype == f32
            ok = front & (u >= 0) & (u <= f32(Wd - 1)) & (v >= 0) & (v <= f32(H - 1))
            ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
            D = a["depth"][k][vi, ui]
            D = (D.astype(np.float64) * a["depth_scale"]).astype(f32) if a["depth_scale"] is not None else D.astype(f32)
            ok &= (D > 0) & np.isfinite(D)
            obj = a["seg"][k][vi // f, ui // f, channel] == value
            d = D - q[2]
            upd = ok & np.where(obj, ~(d < -trunc), d > trunc)
            s = np.where(obj, np.minimum(d, trunc), trunc).astype(f32)
            g = np.where(obj, f32(1), carve).astype(f32)
            upd &= g != 0
            Wn = W + g
            Vn = _fma(V, W, s * g) / Wn
            V = np.where(upd, Vn, V)
            W = np.where(upd, np.minimum(Wn, max_w), W)
            touched |= upd
    return V.reshape(vol.shape), W.reshape(vol.shape), touched.reshape(vol.shape)


_CACHE = {}


def reference(case):
    """(inputs, V64, W64, compare) of a case, computed once per process; the arrays are read-only."""
    hit = _CACHE.get(case["name"])
    if hit is None:
        a = build(case)
        hit = (a,) + fuse_fp64(a)
        for x in list(a.values()) + list(hit[1:]):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _CACHE[case["name"]] = hit
    return hit


def tolerances():
    """(tol V for an fp32 volume, tol W): 4 x the worst |fp32 restatement - fp64| over the compared voxels of every case."""
    if "tol" not in _CACHE:
        dv = dw = 0.0
        for case in CASES:
            a, V64, W64, cmp = reference(case)
            V32, W32, _ = fuse_fp32(a)
            dv = max(dv, float(np.abs(V32.astype(np.float64) - V64)[cmp].max()))
            dw = max(dw, float(np.abs(W32.astype(np.float64) - W64)[cmp].max()))
        _CACHE["tol"] = (4 * dv, 4 * dw)
    return _CACHE["tol"]


def half_ulp_f16(x):
    """Half the spacing of binary16 at |x| (normal range)."""
    return 0.5 * 2.0 ** (np.floor(np.log2(abs(float(x)))) - 10)


def check(case, V, W, what):
    """Asserts a route's result (numpy arrays of the volume's and float32 type) against the float64 restatement."""
    a, V64, W64, cmp = reference(case)
    tol_v, tol_w = tolerances()
    if case["vol"] == "float16":
        tol_v = tol_v + half_ulp_f16(a["trunc"])
    excluded = 1.0 - cmp.mean()
    dv = float(np.abs(V.astype(np.float64) - V64)[cmp].max())
    dw = float(np.abs(W.astype(np.float64) - W64)[cmp].max())
    changed = float((V64 != a["volume"].astype(np.float64))[cmp].mean())
    print("%s %s: |dV| %.3e (tol %.3e)  |dW| %.3e (tol %.3e)  excluded %.2f %%  changed %.1f %%"
          % (what, case["name"], dv, tol_v, dw, tol_w, 100 * excluded, 100 * changed))
    assert excluded <= MAX_EXCLUDED, (case["name"], excluded)
    assert tol_v > 0 and dv <= tol_v and dw <= tol_w, (case["name"], dv, tol_v, dw, tol_w)
    return dv, dw


def to_torch(a, device):
    """The inputs of `build` as the routes' arguments: (positional tensors ..., keyword dict)."""
    import torch
    t = lambda x: torch.from_numpy(np.array(x, order="C")).to(device)   # (a copy: the references are read-only)
    depth = a["depth"]
    depth = torch.from_numpy(depth.view(np.int16).copy()).to(device) if depth.dtype == np.uint16 else t(depth)
    args = (t(a["volume"].copy()), t(a["weight"].copy()), a["voxel_scale"], depth, t(a["seg"]), t(a["intrinsics"]), t(a["rotation"]),
            t(a["translation"]))
    kw = dict(trunc=a["trunc"], obj_class=a["obj_class"], depth_scale=a["depth_scale"], flip_yz=a["flip_yz"],
              carve_weight=a["carve_weight"], max_weight=a["max_weight"])
    return args, kw
