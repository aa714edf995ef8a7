"""SDF volume -> triangle mesh: an independent numpy float64 restatement of the algorithm of DESIGN.md 8k (include/pn2_sdf.h:
pn2s_volume_mesh_count / _emit), the test volumes, and the mesh checks.  Shares no code with the kernel or the torch route.

The restatement walks tetrahedron by tetrahedron and inside set by inside set; whether a triangle faces outwards is decided
here on the tetrahedron's own corner coordinates (normal of the edge midpoints against the vector from the inside corners'
centroid to the outside corners'), not by a table; mesh vertices are found by their keys (7 * linear(lower endpoint) + class)
with a sort and a binary search."""
import itertools

import numpy as np

CLASS_OFFSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]  # +x +y +z +xy +xz +yz +xyz
PERMS = list(itertools.permutations(range(3)))  # xyz xzy yxz yzx zxy zyx


def vertex_tolerance(res, voxel_scale):
    """Per coordinate, kernel (fp32) against the restatement (fp64): three roundings in t and one in the final multiply-add, at the
    box's largest coordinate, with a factor 2 in hand."""
    return 8 * 2.0 ** -24 * (res // 2 + 1) * voxel_scale


def _tet_corners(perm):
    a, b, _ = perm
    t1 = np.zeros(3, dtype=np.int64)
    t1[a] = 1
    t2 = t1.copy()
    t2[b] = 1
    return [np.zeros(3, dtype=np.int64), t1, t2, np.ones(3, dtype=np.int64)]


def _tet_triangles(corners, m):
    """Triangles of a tetrahedron with inside set m -> list of triangles, each three (p, q) corner pairs with p < q."""
    ins = [i for i in range(4) if (m >> i) & 1]
    outs = [i for i in range(4) if not (m >> i) & 1]
    pair = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (1, 3):
        lone, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
        tris = [[pair(lone, r) for r in rest]]
    elif len(ins) == 2:
        (i, j), (k, l) = ins, outs
        tris = [[pair(i, k), pair(i, l), pair(j, l)], [pair(i, k), pair(j, l), pair(j, k)]]
    else:
        return []
    mid = lambda e: (corners[e[0]] + corners[e[1]]) / 2.0
    outward = np.mean([corners[i] for i in outs], axis=0) - np.mean([corners[i] for i in ins], axis=0)
    fixed = []
    for tri in tris:
        n = np.cross(mid(tri[1]) - mid(tri[0]), mid(tri[2]) - mid(tri[0]))
        s = float(n @ outward)
        assert abs(s) > 1e-9
        fixed.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return fixed


def restate(volume, voxel_scale, level=0.0):
    """-> (keys int64 (nv,), verts float64 (nv,3), faces int64 (nf,3)).  voxel_scale and level are taken as the fp32 numbers the
    C entry receives; everything after that is float64."""
    V = np.asarray(volume).astype(np.float64)
    res = V.shape[0]
    assert V.shape == (res, res, res) and res >= 2
    vs, lv = float(np.float32(voxel_scale)), float(np.float32(level))
    inside = V < lv
    lin = np.arange(res ** 3, dtype=np.int64).reshape(res, res, res)
    h = res // 2
    sl = lambda o: tuple(slice(o[d], res - 1 + o[d]) for d in range(3))  # the corner + o of every cell

    # ---- mesh vertices: every crossing edge, by class ----
    keys, pos = [], []
    for c, o in enumerate(CLASS_OFFSETS):
        lo = tuple(slice(0, res - o[d]) for d in range(3))
        hi = tuple(slice(o[d], res) for d in range(3))
        cross = inside[lo] != inside[hi]
        idx = np.argwhere(cross)
        if len(idx) == 0:
            continue
        sa, sb = V[lo][cross], V[hi][cross]
        t = (lv - sa) / (sb - sa)
        pa = (idx - h) * vs
        pos.append(pa + t[:, None] * (np.asarray(o, dtype=np.float64) * vs))
        keys.append(7 * lin[lo][cross] + c)
    if not keys:
        return np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    keys, pos = keys[order], pos[order]
    assert (np.diff(keys) > 0).all()

    # ---- triangles ----
    n_in = sum(inside[sl(o)].astype(np.int64) for o in itertools.product((0, 1), repeat=3))
    cells = np.argwhere((n_in > 0) & (n_in < 8))  # lexicographic = ascending cell linear index
    rows = []  # (cell linear, tetrahedron, triangle, key0, key1, key2)
    for k, perm in enumerate(PERMS):
        T = _tet_corners(perm)
        flags = np.stack([inside[tuple((cells + T[i]).T)] for i in range(4)], axis=1)
        m = (flags * (1 << np.arange(4))).sum(axis=1)
        for case in range(1, 15):
            sel = cells[m == case]
            if len(sel) == 0:
                continue
            for j, tri in enumerate(_tet_triangles(T, case)):
                ks = []
                for p, q in tri:
                    cls = CLASS_OFFSETS.index(tuple(int(x) for x in T[q] - T[p]))
                    ks.append(7 * lin[tuple((sel + T[p]).T)] + cls)
                rows.append(np.stack([lin[tuple(sel.T)], np.full(len(sel), k), np.full(len(sel), j), *ks], axis=1))
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    faces = np.searchsorted(keys, rows[:, 3:])
    assert (keys[faces] == rows[:, 3:]).all()
    return keys, pos, faces.astype(np.int64)


# ---- mesh checks -----------------------------------------------------------------------------------------------------------
def unpaired_edges(faces):
    """Directed edges that do not occur exactly once with their reverse exactly once -> (k,2) array (empty: closed, oriented
    manifold)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros((0, 2), np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    big = int(e.max()) + 1
    code, rev = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    uniq, cnt = np.unique(code, return_counts=True)
    at = np.searchsorted(uniq, rev)
    at_ok = at < len(uniq)
    has_rev = np.zeros(len(e), bool)
    has_rev[at_ok] = uniq[at[at_ok]] == rev[at_ok]
    own = cnt[np.searchsorted(uniq, code)]
    return e[(own != 1) | ~has_rev]


def euler_characteristic(n_verts, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return int(n_verts) - len(np.unique(e, axis=0)) + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- volumes ---------------------------------------------------------------------------------------------------------------
def grid(res, voxel_scale):
    ax = (np.arange(res) - res // 2) * float(voxel_scale)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)


def single_cell(pattern, dtype=np.float32):
    """res = 2: corner (ix,iy,iz) is inside iff bit ix + 2 iy + 4 iz of `pattern`; magnitudes in [0.1, 1) from the pattern's seed."""
    mag = np.random.default_rng(1000 + pattern).uniform(0.1, 1.0, 8)
    v = np.empty((2, 2, 2), dtype=np.float64)
    for o in range(8):
        v[o & 1, (o >> 1) & 1, o >> 2] = -mag[o] if (pattern >> o) & 1 else mag[o]
    return v.astype(dtype)


def sphere(res, voxel_scale, radius, centre=(0.0, 0.0, 0.0)):
    return np.linalg.norm(grid(res, voxel_scale) - np.asarray(centre), axis=-1) - radius


def octahedron(res=9, voxel_scale=0.01):
    """|x|+|y|+|z| - 3 voxels, built from the integer grid so that the values ON the surface are exactly 0 (= the level)."""
    i = np.abs(np.arange(res) - res // 2)
    return ((i[:, None, None] + i[None, :, None] + i[None, None, :]) - 3).astype(np.float64) * float(np.float32(voxel_scale))


def torus(res=33, voxel_scale=0.01, R=0.09, r=0.04):
    g = grid(res, voxel_scale)
    return np.sqrt((np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - R) ** 2 + g[..., 2] ** 2) - r


def touching_spheres(res=17, voxel_scale=0.01):
    """Two spheres of radius 3.25 voxels whose centres lie 6.5 voxels apart along x: they meet at x = 0.25 voxel, between grid
    vertices."""
    a = sphere(res, voxel_scale, 3.25 * voxel_scale, (-3.0 * voxel_scale, 0, 0))
    b = sphere(res, voxel_scale, 3.25 * voxel_scale, (3.5 * voxel_scale, 0, 0))
    return np.minimum(a, b)


def open_surface(res=9, voxel_scale=0.01):
    """A sphere larger than the box's inscribed one, off centre: the surface leaves the box through several faces."""
    return sphere(res, voxel_scale, 4.6 * voxel_scale, (0.7 * voxel_scale, -0.4 * voxel_scale, 0.3 * voxel_scale))


CLOSED = {  # name -> (volume float64, voxel_scale, level, Euler characteristic or None)
    "sphere3": (sphere(3, 0.01, 0.008), 0.01, 0.0, 2),
    "sphere9": (sphere(9, 0.01, 0.0317), 0.01, 0.0, 2),
    "sphere9_level_up": (sphere(9, 0.01, 0.0263), 0.01, 0.005, 2),
    "sphere9_level_down": (sphere(9, 0.01, 0.0341), 0.01, -0.005, 2),
    "octahedron9": (octahedron(), 0.01, 0.0, 2),
    "torus33": (torus(), 0.01, 0.0, 0),
    "touching17": (touching_spheres(), 0.01, 0.0, None),        # (whether the two merge is the grid's matter)
    "sphere65": (sphere(65, 0.004, 0.1017), 0.004, 0.0, 2),     # 65^3 / 256 = 1073 workgroup sums: two chunks of the scan
    "sphere21": (sphere(21, 0.01, 0.0771), 0.01, 0.0, 2),       # 21^3 = 9261 = 36 * 256 + 45: a partly filled last workgroup
}
OPEN = {"open9": (open_surface(), 0.01, 0.0)}


def on_box_face(keys, res):
    """For mesh vertices given by their keys: True where the vertex's edge lies in one of the box's six faces."""
    keys = np.asarray(keys, dtype=np.int64)
    v, c = keys // 7, keys % 7
    lo = np.stack([v // (res * res), (v // res) % res, v % res], axis=1)
    hi = lo + np.asarray(CLASS_OFFSETS)[c]
    return (((lo == 0) & (hi == 0)) | ((lo == res - 1) & (hi == res - 1))).any(axis=1)


def capsule_sdf(p):
    """float64 signed distance to the capsule of datasets/synthetic.py (radius 0.04, core 0.14 along z), restated."""
    p = np.asarray(p, dtype=np.float64)
    dz = p[..., 2] - np.clip(p[..., 2], -0.07, 0.07)
    return np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2 + dz ** 2) - 0.04


def capsule_surface_bound(voxel_scale, r=0.04):
    """|capsule_sdf(vertex)| <= L^2 / (8 (r - L)) + 2 ulp_fp16, L = sqrt(3) voxel: linear interpolation along the longest edge
    class across a surface of curvature <= 1 / (r - L), plus the rounding of the stored values: an endpoint of a crossing edge
    lies within L of the surface, so its value is at most L in magnitude and ulp_fp16 is binary16's spacing at L."""
    L = np.sqrt(3.0) * voxel_scale
    return L * L / (8 * (r - L)) + 2 * 2.0 ** (np.floor(np.log2(L)) - 10)
