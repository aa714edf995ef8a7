"""Cases and restatements for the volume raycast tests (hotrack_amd/csrc/sdf_raycast.hip, network/models/volume_render.py).  Not a
test file.

`raycast_fp64` restates the rule of include/pn2_sdf.h (pn2s_volume_raycast) in float64 numpy, every fused operation as a plain product
and sum.  `raycast_fp32` restates the KERNEL's arithmetic operation by operation in float32 (fmaf as a float64 product and sum rounded
once more to float32: exact but for a rare double rounding, which only matters for the error figures it is used for).  Both walk the
same steps (`_cast`), which is the rule's text line by line.  `sensitive` marks the pixels whose result hangs on a discontinuous
choice -- which step crosses the surface, a ray grazing the silhouette or the box -- by marching again in float64 with half the
minimum step (0.25 voxels) and step_scale 0.5: a pixel whose hit status changes, or whose depth moves by more than 1e-5 m, is left
out, and so is a pixel whose ray sampled a NaN.  At most MAX_EXCLUDED of an image may be left out.  The tolerance the routes are held
to is 4 x the worst |fp32 - fp64| over the case list, recomputed on every run (`tolerances`), for the depth and for the normal's
angle; normals are compared where the float64 gradient (a difference of two samples one voxel apart, voxel_scale for a true distance
field) is at least GRADIENT_FLOOR voxel_scale long, and the pixels below that floor count as left out.

Volumes: the synthetic capsule of _tsdf_cases (radius 0.04), true distances or truncated at 3 voxels (rendered with step_scale 0.8, as
VolumeFusion's volumes are); poses and intrinsics are _tsdf_cases' own."""
import numpy as np

from _tsdf_cases import S_FLIP, _POSES, _rot, capsule_sdf

MAX_EXCLUDED = 0.02
GRADIENT_FLOOR = 0.25

POSES = dict(_POSES)
POSES["beside"] = (_rot([1, 0, 0], 0.3), [0.6, 0.0, 0.3])        # the box lies outside the image: every ray misses it
POSES["inside"] = (_rot([0, 1, 0], 0.4), [0.0, 0.0, 0.005])      # the camera sits inside the capsule: no ray starts outside

# name, res, voxel_scale, (h, w), volume dtype, flip, poses, volume kind, and what differs from the defaults
CASES = [
    dict(name="res5_f32", res=5, scale=0.06, hw=(24, 32), vol="float32", flip=False, poses=["front"], kind="true"),
    dict(name="res17_f16_flip_trunc_F3", res=17, scale=0.016, hw=(24, 32), vol="float16", flip=True, poses=["front", "side", "top"], kind="trunc"),
    dict(name="res33_f32_F3", res=33, scale=0.008, hw=(48, 64), vol="float32", flip=False, poses=["front", "oblique", "side"], kind="true"),
    dict(name="res33_f16_flip_trunc", res=33, scale=0.008, hw=(48, 64), vol="float16", flip=True, poses=["oblique"], kind="trunc"),
    dict(name="res33_close_F3", res=33, scale=0.008, hw=(24, 32), vol="float32", flip=False, poses=["close", "front", "close2"], kind="true"),
    dict(name="res17_23x31_flip_trunc_F3", res=17, scale=0.016, hw=(23, 31), vol="float32", flip=True, poses=["oblique", "top", "close"], kind="trunc"),
    dict(name="res33_f16_close2", res=33, scale=0.008, hw=(23, 31), vol="float16", flip=False, poses=["close2", "close"], kind="true"),
    dict(name="res17_miss", res=17, scale=0.016, hw=(24, 32), vol="float32", flip=False, poses=["beside"], kind="true", hits=False),
    dict(name="res17_inside", res=17, scale=0.016, hw=(24, 32), vol="float16", flip=True, poses=["inside"], kind="true", hits=False),
    dict(name="res17_all_positive", res=17, scale=0.016, hw=(24, 32), vol="float32", flip=False, poses=["front"], kind="positive", hits=False),
    dict(name="res17_all_negative", res=17, scale=0.016, hw=(24, 32), vol="float16", flip=False, poses=["front"], kind="negative", hits=False),
    dict(name="res33_nan_cell", res=33, scale=0.008, hw=(48, 64), vol="float32", flip=False, poses=["front"], kind="nan"),
    dict(name="res17_max_steps_1", res=17, scale=0.016, hw=(24, 32), vol="float32", flip=False, poses=["front"], kind="true", max_steps=1, hits=False),
]
NAN_CELL = (22, 16, 21)   # of res33_nan_cell: outside the capsule, on the camera's side of it


def build(case):
    """The inputs of a case as numpy arrays and plain values (what both restatements and, converted, both routes take)."""
    h, w = case["hw"]
    K = np.array([1.25 * w, 1.25 * w, (w - 1) / 2 + 0.3, (h - 1) / 2 - 0.2])
    rot, trans = [], []
    for name in case["poses"]:
        R, t = POSES[name]
        R, t = np.asarray(R, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)   # fp32-exact poses
        if case["flip"]:
            R, t = S_FLIP @ R, S_FLIP @ t
        rot.append(R.astype(np.float32)), trans.append(t.astype(np.float32))
    res, scale = case["res"], case["scale"]
    ax = (np.arange(res) - res // 2) * scale
    vol = capsule_sdf(np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1), 0.04)
    kind = case["kind"]
    if kind == "trunc":
        vol = np.clip(vol, -3 * scale, 3 * scale)
    elif kind in ("positive", "negative"):
        vol = np.full_like(vol, 0.05 if kind == "positive" else -0.05)
    elif kind == "nan":
        vol[NAN_CELL] = np.nan
    F = len(case["poses"])
    return dict(volume=vol.astype(case["vol"]), voxel_scale=scale, intrinsics=np.tile(K.astype(np.float32), (F, 1)), rotation=np.stack(rot),
                translation=np.stack(trans), hw=(h, w), flip_yz=case["flip"], step_scale=0.8 if kind == "trunc" else 1.0, min_step=0.5,
                refine=8, max_steps=case.get("max_steps"))


def _fma32(x, y, z):
    return (np.asarray(x, np.float64) * np.asarray(y, np.float64) + np.asarray(z, np.float64)).astype(np.float32)


def _cast(a, dt, fma, min_step=None, step_scale=None):
    """The rule, step by step (the numbers are those of the head of sdf_raycast.hip), in the type `dt` with `fma` for its fused
    operations -> dict(depth (F,H,W), hit, normal (F,H,W,3), gnorm: the gradient's length before normalisation, tainted: a NaN was
    sampled, speed)."""
    vol = a["volume"].astype(dt)
    res = vol.shape[0]
    H, W = a["hw"]
    scale = dt(np.float32(a["voxel_scale"]))
    step_scale = dt(np.float32(a["step_scale"] if step_scale is None else step_scale))
    min_step = dt(np.float32(a["min_step"] if min_step is None else min_step))
    max_steps = a["max_steps"] or 8 * res
    lo = dt(-(res // 2)) * scale
    top = dt(res - 1)
    hi = lo + top * scale
    zero = dt(0)

    def sample(p0, p1, p2):   # 3.
        g = [np.fmin(np.fmax((p - lo) / scale, zero), top) for p in (p0, p1, p2)]
        i = [np.minimum(x.astype(np.int64), res - 2) for x in g]
        x, y, z = (gg - ii.astype(dt) for gg, ii in zip(g, i))
        v = lambda da, db, dc: vol[i[0] + da, i[1] + db, i[2] + dc]
        one = dt(1)
        mx, my, mz = one - x, one - y, one - z
        return (((v(0, 0, 0) * mz + v(0, 0, 1) * z) * my + (v(0, 1, 0) * mz + v(0, 1, 1) * z) * y) * mx
                + ((v(1, 0, 0) * mz + v(1, 0, 1) * z) * my + (v(1, 1, 0) * mz + v(1, 1, 1) * z) * y) * x)

    out = {k: [] for k in ("depth", "hit", "normal", "gnorm", "tainted", "speed", "steps")}
    with np.errstate(all="ignore"):
        for k in range(a["rotation"].shape[0]):
            R, t, K = a["rotation"][k].astype(dt), a["translation"][k].astype(dt), a["intrinsics"][k].astype(dt)
            v, u = np.mgrid[0:H, 0:W]
            cx, cy, cz = (u.astype(dt) - K[2]) / K[0], (v.astype(dt) - K[3]) / K[1], dt(1)   # 1.
            if a["flip_yz"]:
                cy, cz = -cy, -cz
            d = [fma(R[2, j], cz, fma(R[0, j], cx, R[1, j] * cy)) for j in range(3)]
            o = [-fma(R[2, j], t[2], fma(R[0, j], t[0], R[1, j] * t[1])) for j in range(3)]
            speed = np.sqrt(fma(d[2], d[2], fma(d[0], d[0], d[1] * d[1])))
            lo_t = [(lo - o[j]) / d[j] for j in range(3)]   # 2.
            hi_t = [(hi - o[j]) / d[j] for j in range(3)]
            z_in = np.fmax(np.fmax(np.fmin(lo_t[0], hi_t[0]), np.fmin(lo_t[1], hi_t[1])), np.fmin(lo_t[2], hi_t[2]))
            z_out = np.fmin(np.fmin(np.fmax(lo_t[0], hi_t[0]), np.fmax(lo_t[1], hi_t[1])), np.fmax(lo_t[2], hi_t[2]))
            z_in = np.fmax(z_in, dt(np.float32(1e-3)))
            ray = z_out > z_in
            at = lambda zz: sample(fma(zz, d[0], o[0]), fma(zz, d[1], o[1]), fma(zz, d[2], o[2]))
            z = np.where(ray, z_in, zero).astype(dt)   # 4.
            s = at(z)
            tainted = ray & np.isnan(s)
            alive = ray & (s > 0)
            hit = np.zeros((H, W), dtype=bool)
            steps = np.zeros((H, W), dtype=np.int64)
            za, zb, sa, sb = (np.zeros((H, W), dtype=dt) for _ in range(4))
            m = min_step * scale
            for _ in range(max_steps):
                if not alive.any():
                    break
                dz = np.fmax(s * step_scale, m) / speed
                zn = np.fmin(z + dz, z_out)
                sn = at(zn)
                tainted |= alive & np.isnan(sn)
                cross = alive & (sn <= 0)
                za, sa, zb, sb = np.where(cross, z, za), np.where(cross, s, sa), np.where(cross, zn, zb), np.where(cross, sn, sb)
                hit |= cross
                steps += alive
                alive = alive & ~cross & (zn < z_out)
                z, s = np.where(alive, zn, z), np.where(alive, sn, s)
            for _ in range(a["refine"]):   # 5.
                zm = (za + zb) * dt(0.5)
                sm = at(zm)
                tainted |= hit & np.isnan(sm)
                neg = sm <= 0
                zb, sb, za, sa = np.where(neg, zm, zb), np.where(neg, sm, sb), np.where(neg, za, zm), np.where(neg, sa, sm)
            zh = za + (zb - za) * sa / (sa - sb)
            p = [fma(zh, d[j], o[j]) for j in range(3)]   # 6.
            e = dt(0.5) * scale
            g = []
            for j in range(3):
                plus, minus = list(p), list(p)
                plus[j], minus[j] = p[j] + e, p[j] - e
                sp, sm = sample(*plus), sample(*minus)
                tainted |= hit & (np.isnan(sp) | np.isnan(sm))
                g.append(sp - sm)
            n2 = fma(g[2], g[2], fma(g[0], g[0], g[1] * g[1]))
            ok = n2 > 0
            length = np.sqrt(np.where(ok, n2, dt(1)))
            g = [np.where(ok, x / length, zero) for x in g]
            n = [fma(R[i, 2], g[2], fma(R[i, 0], g[0], R[i, 1] * g[1])) for i in range(3)]
            if a["flip_yz"]:
                n[1], n[2] = -n[1], -n[2]
            out["depth"].append(np.where(hit, zh, zero)), out["hit"].append(hit & (zh > 0))
            out["normal"].append(np.where(hit[..., None], np.stack(n, axis=-1), zero))
            out["gnorm"].append(np.where(hit & ok, np.sqrt(np.where(ok, n2, zero)), zero)), out["tainted"].append(tainted)
            out["speed"].append(speed), out["steps"].append(steps)
    return {k: np.stack(x) for k, x in out.items()}


def raycast_fp64(a, **kw):
    return _cast(a, np.float64, lambda x, y, z: x * y + z, **kw)


def raycast_fp32(a):
    return _cast(a, np.float32, _fma32)


def sensitive(case):
    """(F,H,W) bool: the pixels of a case that are left out of every comparison (the module's docstring)."""
    return reference(case)[2]


_CACHE = {}


def reference(case):
    """(inputs, float64 result, left-out pixels, pixels whose normal is compared) of a case, computed once per process; read-only."""
    hit = _CACHE.get(case["name"])
    if hit is None:
        a = build(case)
        ref = raycast_fp64(a)
        again = raycast_fp64(a, min_step=0.25, step_scale=0.5)
        sens = (ref["hit"] != again["hit"]) | (ref["hit"] & again["hit"] & (np.abs(ref["depth"] - again["depth"]) > 1e-5))
        sens |= ref["tainted"] | again["tainted"]
        flat = ref["hit"] & ~sens & (ref["gnorm"] < GRADIENT_FLOOR * float(np.float32(a["voxel_scale"])))
        hit = (a, ref, sens, ref["hit"] & ~sens & ~flat, flat)
        for x in list(a.values()) + list(ref.values()) + list(hit[2:]):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _CACHE[case["name"]] = hit
    return hit[:4]


def excluded(case):
    """Per frame, the share of the image that is left out of the comparison: sensitive pixels and normals below the floor."""
    reference(case)
    _, _, sens, _, flat = _CACHE[case["name"]]
    return (sens | flat).reshape(sens.shape[0], -1).mean(axis=1)


def angle(n1, n2):
    """The angle between unit vectors (..., 3), in float64 and well conditioned at 0."""
    n1, n2 = n1.astype(np.float64), n2.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(n1, n2), axis=-1), (n1 * n2).sum(-1))


def tolerances():
    """(tol depth in metres, tol normal angle in radians): 4 x the worst |fp32 restatement - fp64| over the compared pixels of every case."""
    if "tol" not in _CACHE:
        dz = da = 0.0
        for case in CASES:
            a, ref, sens, shade = reference(case)
            r32 = raycast_fp32(a)
            both = ref["hit"] & r32["hit"] & ~sens
            if both.any():
                dz = max(dz, float(np.abs(r32["depth"].astype(np.float64) - ref["depth"])[both].max()))
            both = both & shade
            if both.any():
                da = max(da, float(angle(r32["normal"], ref["normal"])[both].max()))
        _CACHE["tol"] = (4 * dz, 4 * da)
    return _CACHE["tol"]


def check(case, depth, normal, what):
    """Asserts a route's result (numpy float32 arrays; normal may be None) against the float64 restatement."""
    a, ref, sens, shade = reference(case)
    tol_z, tol_a = tolerances()
    depth = np.asarray(depth)
    assert depth.shape == ref["depth"].shape and depth.dtype == np.float32
    cmp = ~sens
    got_hit = depth > 0
    wrong = int(((got_hit != ref["hit"]) & cmp).sum())
    both = got_hit & ref["hit"] & cmp
    dz = float(np.abs(depth.astype(np.float64) - ref["depth"])[both].max()) if both.any() else 0.0
    da = 0.0
    if normal is not None:
        normal = np.asarray(normal)
        assert normal.shape == ref["normal"].shape and normal.dtype == np.float32
        assert not normal[~got_hit].any()   # no hit: the zero normal
        if (both & shade).any():
            da = float(angle(normal, ref["normal"])[both & shade].max())
            assert np.allclose(np.linalg.norm(normal[both & shade].astype(np.float64), axis=-1), 1.0, atol=1e-6)
    worst = float(excluded(case).max())
    print("%s %s: hits %d  wrong hit status %d  |dz| %.3e (tol %.3e)  angle %.3e (tol %.3e)  left out %.2f %%"
          % (what, case["name"], int(ref["hit"].sum()), wrong, dz, tol_z, da, tol_a, 100 * worst))
    assert worst <= MAX_EXCLUDED, (case["name"], worst)
    assert bool(ref["hit"].any()) == case.get("hits", True), case["name"]
    assert not (depth[cmp] < 0).any() and not np.isnan(depth[cmp]).any()
    assert wrong == 0, (case["name"], wrong)
    assert tol_z > 0 and dz <= tol_z, (case["name"], dz, tol_z)
    assert tol_a > 0 and da <= tol_a, (case["name"], da, tol_a)
    return dz, da


def to_torch(a, device):
    """The inputs of `build` as the routes' arguments: (positional ..., keyword dict)."""
    import torch
    t = lambda x: torch.from_numpy(np.array(x, order="C")).to(device)   # (a copy: the references are read-only)
    args = (t(a["volume"]), a["voxel_scale"], t(a["intrinsics"]), t(a["rotation"]), t(a["translation"]), a["hw"])
    kw = dict(flip_yz=a["flip_yz"], step_scale=a["step_scale"], min_step=a["min_step"], refine=a["refine"], max_steps=a["max_steps"])
    return args, kw
