"""The depth-frame contract (include/pn2_ext.h: pn2x_depth_frame_clouds) restated in numpy, and small frames to run it on.

The restatement works operation by operation in np.float32 (float64 where the contract says double), so the kernels' outputs are
compared with it bit for bit.  The generator draws segments as blobs on a tilted plane with noise and dropped pixels, puts the
crop centres on the plane, and asserts in float64 that no pixel of a case lies within 1e-5 m of a crop radius nor within 1e-9
of the validity threshold: nothing is left out of the exact comparison."""
import numpy as np

F32 = np.float32
HO3D_DEPTH_SCALE = 0.00012498664727900177
NPOINT, CAP = 64, 320
TILE = 1024


# ---- the slot rule -------------------------------------------------------------------------------------------------------------
def slot_of_rank(n: int, cap: int) -> np.ndarray:
    """(n,) int64: the slot of the point of rank r, -1 where it is dropped."""
    r = np.arange(n, dtype=np.int64)
    if n <= cap:
        return r
    s0, s1 = r * cap // n, (r + 1) * cap // n
    return np.where(s1 > s0, s0, -1)


def fill_cloud(pts: np.ndarray, cap: int) -> np.ndarray:
    """(n,3) points in rank order -> the (cap,3) buffer: the slot rule, the padding with the point of rank 0, zeros when empty."""
    cloud = np.zeros((cap, 3), dtype=F32)
    n = len(pts)
    if n == 0:
        return cloud
    slot = slot_of_rank(n, cap)
    cloud[slot[slot >= 0]] = pts[slot >= 0]
    if n < cap:
        cloud[n:] = pts[0]
    return cloud


# ---- per-pixel arithmetic ------------------------------------------------------------------------------------------------------
def _decode(depth: np.ndarray, depth_scale) -> np.ndarray:
    if depth.dtype == np.uint16:
        return (depth.astype(np.float64) * np.float64(depth_scale)).astype(F32)
    assert depth.dtype == F32
    return depth


def _upsampled_seg(seg: np.ndarray, h: int, w: int) -> np.ndarray:
    hs, ws = seg.shape[:2]
    assert h % hs == 0 and w % ws == 0 and h // hs == w // ws
    f = h // hs
    return seg[(np.arange(h) // f)[:, None], (np.arange(w) // f)[None, :]]


def classify(depth, seg, intr, classes, flip_yz, depth_scale=None, dtype=F32):
    """One frame.  classes: ((channel, value, centre (3,), radius), ...).  -> points (h,w,3), valid (h,w), and per class
    (segment match (h,w), distance to the centre (h,w)), all in `dtype` (float32: the kernel's arithmetic; float64: the margins)."""
    h, w = depth.shape
    z = _decode(depth, depth_scale)
    valid = z > F32(1e-6)
    z = z.astype(dtype)
    fx, fy, cx, cy = (dtype(v) for v in intr)
    u = np.arange(w, dtype=dtype)[None, :]
    v = np.arange(h, dtype=dtype)[:, None]
    x = ((u - cx) * z) / fx
    y = ((v - cy) * z) / fy
    if flip_yz:
        y, z = -y, -z
    full = _upsampled_seg(seg, h, w)
    per_class = []
    for channel, value, centre, _ in classes:
        c = np.asarray(centre).astype(dtype)
        dx, dy, dz = x - c[0], y - c[1], z - c[2]
        per_class.append((full[..., channel] == value, np.sqrt((dx * dx + dy * dy) + dz * dz)))
    return np.stack([x, y, z], axis=-1), valid, per_class


def restate(case: dict) -> dict:
    """clouds (B,2,cap,3), counts (B,2), background (B,H,W), and the padded buffers' points in rank order per (frame, class)."""
    depth, seg, cap = case["depth"], case["seg"], case["cap"]
    B, H, W = depth.shape
    clouds = np.zeros((B, 2, cap, 3), dtype=F32)
    counts = np.zeros((B, 2), dtype=np.int32)
    background = np.zeros((B, H, W), dtype=np.uint8)
    for b in range(B):
        classes = [(ch, val, centre[b], radius) for ch, val, centre, radius in (case["hand"], case["obj"])]
        pts, valid, per_class = classify(depth[b], seg[b], case["intrinsics"][b], classes, case["flip_yz"], case["depth_scale"])
        background[b] = (_upsampled_seg(seg[b], H, W) == 0).all(axis=-1)
        for k, (match, dist) in enumerate(per_class):
            flag = valid & match & (dist < F32(classes[k][3]))
            counts[b, k] = flag.sum()
            clouds[b, k] = fill_cloud(pts[flag], cap)   # (boolean indexing walks the pixels in row-major order)
    return {"clouds": clouds, "counts": counts, "background": background}


def near_radius(case: dict, key: str) -> bool:
    """Whether, in float64, a valid pixel of some frame lies within 1e-5 m of the crop radius of class `key`."""
    ch, val, centre, radius = case[key]
    for b in range(case["depth"].shape[0]):
        _, valid, per_class = classify(case["depth"][b], case["seg"][b], case["intrinsics"][b], [(ch, val, centre[b], radius)],
                                       case["flip_yz"], case["depth_scale"], dtype=np.float64)
        if (np.abs(per_class[0][1][valid] - float(F32(radius))) < 1e-5).any():
            return True
    return False


def assert_margins(case: dict) -> None:
    for b in range(case["depth"].shape[0]):
        z = _decode(case["depth"][b], case["depth_scale"]).astype(np.float64)
        assert not (np.abs(z - 1e-6) < 1e-9).any(), case["name"]
    assert not near_radius(case, "hand") and not near_radius(case, "obj"), case["name"]


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def _class_codes(c: int):
    return ((0, 255), (1, 255)) if c == 3 else ((0, 1), (0, 2))


def make_case(name, seed, B, H, W, f, C, blobs, flip_yz=False, u16=False, cap=CAP, radii=(0.15, 0.25), zero_share=0.1):
    """blobs[b][k] = None (no pixel of class k in frame b) or dict(at=(row, col) in depth pixels, r=blob radius in pixels,
    n=exact pixel count to trim the class to (f == 1 only) or None, from_pixel=first flat pixel index the class may have or None)."""
    rng = np.random.default_rng(seed)
    Hs, Ws = H // f, W // f
    fx = fy = 0.9 * W
    cx, cy = W / 2 - 0.37, H / 2 + 0.21
    intr = np.tile(np.array([fx, fy, cx, cy], dtype=F32), (B, 1))
    intr[:, :2] += rng.uniform(-1, 1, (B, 2)).astype(F32)
    vv, uu = np.mgrid[0:H, 0:W]
    depth = np.zeros((B, H, W), dtype=F32)
    seg = np.zeros((B, Hs, Ws, C), dtype=np.uint8)
    centres = np.zeros((2, B, 3), dtype=F32)
    codes = _class_codes(C)
    scale = HO3D_DEPTH_SCALE if u16 else None
    raw = np.zeros((B, H, W), dtype=np.uint16)
    for b in range(B):
        a, c = rng.uniform(-0.0015, 0.0015, 2)
        z = 0.5 + a * (uu - W / 2) + c * (vv - H / 2) + rng.normal(0, 0.002, (H, W))
        z[rng.random((H, W)) < zero_share] = 0.0
        depth[b] = z.astype(F32)
        if u16:
            raw[b] = np.rint(z / scale).astype(np.uint16)
        sv, su = np.mgrid[0:Hs, 0:Ws]
        for k in range(2):
            blob = blobs[b][k]
            row, col = blob["at"] if blob else (H // 2, W // 2)
            zc = 0.5 + a * (col - W / 2) + c * (row - H / 2)   # on the plane, whether or not the pixel itself was dropped
            p = np.array([(col - float(intr[b, 2])) * zc / float(intr[b, 0]), (row - float(intr[b, 3])) * zc / float(intr[b, 1]), zc])
            centres[k, b] = (p * ([1, -1, -1] if flip_yz else [1, 1, 1])).astype(F32)
            if blob:
                inside = ((sv * f + (f - 1) / 2 - row) / blob["r"]) ** 2 + ((su * f + (f - 1) / 2 - col) / (1.3 * blob["r"])) ** 2 < 1
                if C == 3:
                    seg[b, ..., codes[k][0]][inside] = codes[k][1]
                else:
                    seg[b, ..., 0][inside & (seg[b, ..., 0] == 0)] = codes[k][1]
    case = {"name": name, "depth": raw if u16 else depth, "depth_scale": scale, "seg": seg, "intrinsics": intr, "cap": cap,
            "flip_yz": bool(flip_yz), "hand": codes[0] + (centres[0], radii[0]), "obj": codes[1] + (centres[1], radii[1])}
    # radii clear of every pixel by 1e-5 m: step the nominal radius until none is near (depends on the inputs alone)
    for key in ("hand", "obj"):
        while near_radius(case, key):
            case[key] = case[key][:3] + (float(F32(case[key][3] + 3.1e-5)),)
    # trim the classes to their exact counts / first pixels by clearing segment bytes (the restatement's own flags say which)
    for b in range(B):
        for k, key in enumerate(("hand", "obj")):
            blob = blobs[b][k]
            if not blob or (blob.get("n") is None and blob.get("from_pixel") is None):
                continue
            ch, val, centre, radius = case[key]
            _, valid, per_class = classify(case["depth"][b], seg[b], intr[b], [(ch, val, centre[b], radius)], flip_yz, scale)
            flag = (valid & per_class[0][0] & (per_class[0][1] < F32(radius))).reshape(-1)
            ranked = np.flatnonzero(flag)
            drop = ranked[ranked < blob["from_pixel"]] if blob.get("from_pixel") is not None else ranked[blob["n"]:]
            if blob.get("n") is not None:
                assert f == 1 and len(ranked) >= blob["n"], (name, b, k, len(ranked))
            seg[b, (drop // W) // f, (drop % W) // f, ch] = 0
    assert_margins(case)
    return case


def _blob(at, r, n=None, from_pixel=None):
    return dict(at=at, r=r, n=n, from_pixel=from_pixel)


def cases():
    """The test frames; every (frame, class) count regime the contract names occurs (checked by tests/test_depth_frame_cpu.py)."""
    return [
        # 48 x 64, segment at full resolution, one channel: a cloud above cap and one of exactly cap pixels
        make_case("48x64_c1", 1, 1, 48, 64, 1, 1, [[_blob((20, 22), 16), _blob((28, 44), 14, n=CAP)]]),
        # 60 x 80 with the segment at 30 x 40 x 3, y and z flipped: npoint <= n < cap, and a class whose first pixel is in the last tile
        make_case("60x80_seg30x40", 2, 1, 60, 80, 2, 3, [[_blob((20, 30), 6), _blob((56, 40), 5, from_pixel=4 * TILE)]], flip_yz=True),
        # 50 x 70, three frames, uint16 depth at HO3D's scale, flipped: a different count per frame and class, one of them empty
        make_case("50x70_u16_b3", 3, 3, 50, 70, 1, 3,
                  [[_blob((25, 20), 9, n=10), None], [_blob((22, 30), 17), _blob((30, 45), 10, n=100)],
                   [_blob((47, 35), 8, from_pixel=3 * TILE), _blob((20, 40), 15, n=CAP)]], flip_yz=True, u16=True),
        # 51 x 67: an odd pixel count, so the second frame's rows start off every vector alignment
        make_case("51x67_b2", 4, 2, 51, 67, 1, 1, [[_blob((25, 30), 15), _blob((10, 10), 5, n=NPOINT - 1)],
                                                    [_blob((30, 20), 7, n=NPOINT), _blob((25, 45), 14, n=CAP + 1)]]),
        # 48 x 64 uint16, not flipped, the segment at 24 x 32 x 1
        make_case("48x64_u16_seg24x32", 5, 1, 48, 64, 2, 1, [[_blob((24, 20), 12), _blob((24, 46), 5)]], u16=True),
    ]


def factor_cases():
    """The two ways a kernel finds a pixel's segment cell, which cases() does not tell apart (its factors are 1 and 2): two frames
    of 12 x 12 depth, cap 64, three channels, over segments of 12 x 12 (f = 1), 3 x 3 (f = 4, a power of two: the shift) and 4 x 4
    (f = 3: the division), each with fp32 and with uint16 depth.  Both classes have pixels in every frame."""
    blobs = [[_blob((4, 4), 4), _blob((7, 8), 4)], [_blob((7, 5), 5), _blob((4, 8), 4)]]
    return [make_case("12x12_f%d_%s" % (f, "u16" if u16 else "f32"), 20 + 2 * f + u16, 2, 12, 12, f, 3, blobs, flip_yz=bool(u16), u16=u16,
                      cap=64) for f in (1, 4, 3) for u16 in (False, True)]
