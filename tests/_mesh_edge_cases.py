"""Edge cases of the mesh -> signed-distance path beyond tests/_mesh_cases.py: sliver triangles, meshes away from the origin and
at other scales, queries on the surface and in the planes of its faces, other topologies, and the launch shapes of the kernel.
Pure numpy, seeded; every array is read-only; the reference is `_mesh_cases.oracle_uncached` (float64 from the same fp32
inputs), computed once per case and process.

A case is (name, verts fp32, faces int32, queries fp32, checks, volume): `checks` names what `check` asserts --
  mag       | |d| - |oracle| | <= tol(case)
  wn        |winding - oracle| <= WN_TOL
  sign      signs equal where the oracle's |d| >= SIGN_MIN (and, with `open`, its winding is >= 1e-3 away from 0.5); at most
            SIGN_SKIP_MAX of the queries may be left out
  box       |d - box_sdf| <= tol(case): the mesh's surface is the box of _mesh_cases
  positive  d > 0
  contact   the queries lie on the surface: |d| <= tol(case), d and the winding finite, no sign
-- and `volume` is (res, stride) where the queries are grid(res, stride), for the volume entry.

tol(case) = MAG_TOL * max(1, L / 0.25) with L the largest absolute coordinate among the case's vertices and queries: MAG_TOL is
the bound for coordinates up to ~0.2 m and the rounding of (query - vertex) grows with the coordinates."""
import functools
from collections import namedtuple

import numpy as np

import _mesh_cases as MC

Case = namedtuple("Case", "name verts faces queries checks volume")
OPEN_WN_MARGIN = 1e-3  # 10 WN_TOL: signs of an open mesh are compared where the oracle's winding is this far from 0.5

SLIVER_RATIOS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6)  # height / base; 1e-6 lands just above the degeneracy threshold (sin^2 1e-12)
SLIVER_SHAPES = ("cap", "needle", "skew")
SLIVER_BASE = 0.1
SLIVER_OFFSETS = (0.0, 0.05)
BOX_SLIVER_RATIOS = (1e-3, 1e-4, 1e-5, 1e-6)
FACE_COUNTS = (1, 511, 512, 513, 1024, 1025)  # around the kernel's LDS chunk of 512 triangles
POINT_COUNTS = (1, 255, 256, 257)             # around its workgroup of 256 queries
SMALL_VOLUMES = ((3, 0.1), (5, 0.05))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _case(name, v, f, q, checks, volume=None):
    v, f, q = _ro(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(q, np.float32))
    return Case(name, v, f, q, tuple(checks), volume)


def tol(case):
    L = max(float(np.abs(case.verts).max()), float(np.abs(case.queries).max()))
    return MC.MAG_TOL * max(1.0, L / 0.25)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _rows(p):
    return tuple(p[:, k] for k in range(3))


# ---- A: single slivers -----------------------------------------------------------------------------------------------------------
def sliver_names(shape, ratio):
    return [f"sliver_{shape}_{ratio:g}_o{order}{'r' if rev else ''}_t{off:g}" for order in range(3) for rev in (0, 1)
            for off in SLIVER_OFFSETS]


def _sliver(name):
    _, shape, ratio, order, off = name.split("_")
    ratio, rev, order, off = float(ratio), order.endswith("r"), int(order[1]), float(off[1:])
    b, h = SLIVER_BASE, float(ratio) * SLIVER_BASE
    third = {"cap": (0.47 * b, h, 0.0), "needle": (b, h, 0.0), "skew": (0.01 * b, h, 0.0)}[shape]
    tri = np.array([(0.0, 0.0, 0.0), (b, 0.0, 0.0), third])
    tri = np.roll(tri, -order, axis=0)
    if rev:
        tri = tri[[0, 2, 1]]
    seed = [SLIVER_SHAPES.index(shape), SLIVER_RATIOS.index(ratio), order, int(rev), int(off > 0)]
    rng = np.random.default_rng([7] + seed)
    shift = np.array([off, -off, off])
    v32 = (tri @ _rotation(rng).T + shift).astype(np.float32)
    v = v32.astype(np.float64)  # the triangle the kernel sees
    n = np.cross(v[1] - v[0], v[2] - v[0])
    n /= np.linalg.norm(n)
    k = 2000
    q1 = rng.uniform(-0.15, 0.15, (k, 3)) + shift
    s, r = np.sqrt(rng.random((k, 1))), rng.random((k, 1))
    height = rng.uniform(1e-3, 5e-2, (k, 1)) * rng.choice([-1.0, 1.0], (k, 1))
    q2 = v[0] * (1 - s) + v[1] * (s * (1 - r)) + v[2] * (s * r) + n * height
    lengths = np.array([np.linalg.norm(v[(i + 1) % 3] - v[i]) for i in range(3)])
    long_edges = np.argsort(lengths)[1:]
    e = long_edges[rng.integers(0, 2, k)]
    start, end = v[e], v[(e + 1) % 3]
    along = end - start
    perp = np.cross(n, along / np.linalg.norm(along, axis=-1, keepdims=True))
    q3 = start + along * rng.random((k, 1)) + perp * rng.normal(0.0, 0.2 * h, (k, 1)) + n * height
    return _case(name, v32, [[0, 1, 2]], np.concatenate([q1, q2, q3]), ("mag",))


def sliver_height(case):
    """The smallest altitude of the (single) triangle as its fp32 vertices hold it, in float64."""
    v = case.verts.astype(np.float64)
    area2 = np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0]))
    return float(area2 / max(np.linalg.norm(v[(i + 1) % 3] - v[i]) for i in range(3)))


def edge_distance(case):
    """float64 distance of the case's queries to the nearest edge of its (single) triangle."""
    v, p = case.verts.astype(np.float64), _rows(case.queries.astype(np.float64))
    d2 = [MC._segment_dist2(p, tuple(v[i]), tuple(v[(i + 1) % 3])) for i in range(3)]
    return np.sqrt(np.minimum(np.minimum(d2[0], d2[1]), d2[2]))


# ---- B: the box with sliver faces -------------------------------------------------------------------------------------------------
def _box_with_slivers():
    """On four faces of the box a vertex strictly inside a triangle, at BOX_SLIVER_RATIOS x edge above one of its edges, splits
    the triangle into three.  The box's faces are axis-aligned, so the new vertex is exactly coplanar: the surface and box_sdf
    are unchanged."""
    v32, f = MC.mesh("box")
    v, f = list(v32.astype(np.float64)), [tuple(t) for t in f]
    for i, (fi, ratio) in enumerate(zip((0, 3, 6, 9), BOX_SLIVER_RATIOS)):  # triangles of four different box faces
        ia, ib, ic = f[fi]
        tri = [v[ia], v[ib], v[ic]]
        s, e, o = (tri[(i + j) % 3] for j in range(3))  # the edge differs from insert to insert (legs and hypotenuse)
        foot = s + 0.47 * (e - s)
        along = (e - s) / np.linalg.norm(e - s)
        inward = (o - foot) - along * np.dot(o - foot, along)
        p = (foot + ratio * np.linalg.norm(e - s) * inward / np.linalg.norm(inward)).astype(np.float32)
        axis = [k for k in range(3) if tri[0][k] == tri[1][k] == tri[2][k]]
        assert len(axis) == 1
        p[axis[0]] = np.float32(tri[0][axis[0]])
        p = p.astype(np.float64)
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        for x, y in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            assert np.dot(np.cross(y - x, p - x), n) > 0, "the inserted vertex is not strictly inside its triangle"
        ip = len(v)
        v.append(p)
        f[fi] = (ia, ib, ip)
        f += [(ib, ic, ip), (ic, ia, ip)]
    return _case("box_with_slivers", np.array(v), np.array(f), MC.grid(), ("mag", "sign", "wn", "box"))


# ---- C: placement and scale -------------------------------------------------------------------------------------------------------
def _placed(name):
    v, f = MC.mesh("torus24")
    v, q = v.astype(np.float64), MC.grid()[::2].astype(np.float64)
    if name == "torus_shifted":
        t = np.array([0.3, -0.2, 0.25])
        v, q = v + t, q + t
    elif name == "torus_x10":
        v, q = v * 10.0, q * 10.0
    elif name == "torus_x0.01":
        v, q = v * 0.01, q * 0.01
    elif name == "volume_torus_small":
        return _case(name, v * 0.4 + np.array([0.03, -0.02, 0.025]), f, MC.grid(), ("mag", "sign"), (25, 0.0167))
    return _case(name, v, f, q, ("mag", "sign", "wn"))


# ---- D: contact and coplanar queries ----------------------------------------------------------------------------------------------
def _contact(mesh_name):
    v32, f = MC.mesh(mesh_name)
    v = v32.astype(np.float64)
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    mid = (v[edges[:, 0]] + v[edges[:, 1]]) / 2
    centroid = (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / 3
    return _case(f"contact_{mesh_name}", v32, f, np.concatenate([v, mid, centroid]), ("contact",))


def _coplanar_box():
    """Queries in the six face planes of the box but outside it, and on the lines through its twelve edges beyond the corners:
    the solid angle's numerator is zero or rounding noise for the coplanar faces; box_sdf is exact and positive there."""
    v32, f = MC.mesh("box")
    half = MC.BOX_HALF
    rng = np.random.default_rng(11)
    q = []
    for k in range(3):
        for sgn in (-1.0, 1.0):
            p = rng.uniform(-0.15, 0.15, (40, 3))
            j = (k + 1 + rng.integers(0, 2, 40)) % 3  # one in-plane coordinate is pushed past the face
            p[np.arange(40), j] = rng.choice([-1.0, 1.0], 40) * (half[j] + rng.uniform(1e-3, 0.1, 40))
            p[:, k] = sgn * half[k]
            q.append(p)
    for k in range(3):  # the edges parallel to axis k
        i, j = (k + 1) % 3, (k + 2) % 3
        for si in (-1.0, 1.0):
            for sj in (-1.0, 1.0):
                p = np.empty((10, 3))
                p[:, i], p[:, j] = si * half[i], sj * half[j]
                p[:, k] = rng.choice([-1.0, 1.0], 10) * (half[k] + rng.uniform(1e-3, 0.1, 10))
                q.append(p)
    return _case("coplanar_box", v32, f, np.concatenate(q), ("mag", "box", "positive", "wn"))


# ---- E: topology ----------------------------------------------------------------------------------------------------------------
def _topology(name):
    v32, f = MC.mesh("box")
    v = v32.astype(np.float64)
    if name == "box_reversed":
        return _case(name, v, f[:, [0, 2, 1]], MC.grid(), ("mag", "sign", "wn"))
    if name == "two_boxes":
        return _case(name, np.concatenate([v, v + np.array([0.09, 0.02, -0.03])]), np.concatenate([f, f + 8]), MC.grid(),
                     ("mag", "sign", "wn"))
    if name == "nested_boxes":  # the same orientation: the winding number is 2 inside the inner box
        return _case(name, np.concatenate([v, v * 2.0]), np.concatenate([f, f + 8]), MC.grid(), ("mag", "sign", "wn"))
    if name == "box_open":  # the +z quad removed: a fractional winding number
        return _case(name, v, f[:10], MC.grid(), ("mag", "sign", "wn", "open"))
    raise KeyError(name)


# ---- F: launch shapes -------------------------------------------------------------------------------------------------------------
def _launch(name):
    kind, n = name.rsplit("_", 1)
    if kind == "faces":  # an open mesh: the first n faces of torus48
        v, f = MC.mesh("torus48")
        return _case(name, v, f[:int(n)], MC.grid()[::2], ("mag", "wn"))
    v, f = MC.mesh("torus24")
    if kind == "points":
        return _case(name, v, f, MC.grid()[:int(n)], ("mag", "wn"))
    res, stride = SMALL_VOLUMES[[r for r, _ in SMALL_VOLUMES].index(int(n))]
    return _case(name, v, f, MC.grid(res, stride), ("mag",), (res, stride))


SLIVERS = tuple(n for s in SLIVER_SHAPES for r in SLIVER_RATIOS for n in sliver_names(s, r))
PLACED = ("torus_shifted", "torus_x10", "torus_x0.01")
CONTACT = ("contact_box", "contact_torus24")
TOPOLOGY = ("box_reversed", "two_boxes", "nested_boxes", "box_open")
LAUNCH = tuple(f"faces_{n}" for n in FACE_COUNTS) + tuple(f"points_{m}" for m in POINT_COUNTS)
VOLUMES = ("volume_torus_small",) + tuple(f"volume_{r}" for r, _ in SMALL_VOLUMES)
MESH_CASES = ("box_with_slivers",) + PLACED + CONTACT + ("coplanar_box",) + TOPOLOGY + LAUNCH  # every case but the slivers
SIGNED = ("box_with_slivers",) + PLACED + ("volume_torus_small",) + TOPOLOGY  # the cases whose signs are compared


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("sliver_"):
        return _sliver(name)
    if name == "box_with_slivers":
        return _box_with_slivers()
    if name in PLACED or name == "volume_torus_small":
        return _placed(name)
    if name in CONTACT:
        return _contact(name[len("contact_"):])
    if name == "coplanar_box":
        return _coplanar_box()
    if name in TOPOLOGY:
        return _topology(name)
    return _launch(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (signed distance, winding number) of the float64 brute force on the case, read-only."""
    c = case(name)
    return _ro(*MC.oracle_uncached(c.queries, c.verts, c.faces))


def sign_mask(c, d_ref, w_ref):
    """The queries whose signs are compared."""
    keep = np.abs(d_ref) >= MC.SIGN_MIN
    if "open" in c.checks:
        keep &= np.abs(w_ref - 0.5) >= OPEN_WN_MARGIN
    return keep


def magnitude_error(c, got):
    """max | |d| - |oracle| | (NaN counts as infinite)."""
    err = np.abs(np.abs(np.asarray(got, np.float64).reshape(-1)) - np.abs(reference(c.name)[0]))
    return float(np.nan_to_num(err, nan=np.inf).max())


def check(c, got, got_wn=None, label=""):
    """Prints each figure of the case's checks, then asserts them."""
    d_ref, w_ref = reference(c.name)
    got = np.asarray(got, np.float64).reshape(-1)
    bound, label = tol(c), f"{label}, {c.name}"
    assert got.shape == d_ref.shape
    assert np.isfinite(got).all(), f"{label}: non-finite distances"
    failures = []
    if "mag" in c.checks:
        mag = float(np.abs(np.abs(got) - np.abs(d_ref)).max())
        over = float((np.abs(np.abs(got) - np.abs(d_ref)) > bound).mean())
        print(f"{label}: max | |d| - |oracle| | = {mag:.3e} m (bound {bound:.3e}), {over:.2%} of the queries beyond it")
        if mag > bound:
            failures.append(f"magnitude differs from the oracle by {mag:.3e} > {bound:.3e} ({over:.2%} of the queries)")
    if "box" in c.checks:
        err = float(np.abs(got - MC.box_sdf(c.queries)).max())
        print(f"{label}: max |d - box closed form| = {err:.3e} m (bound {bound:.3e})")
        if err > bound:
            failures.append(f"differs from the box's closed form by {err:.3e}")
    if "contact" in c.checks:
        worst = float(np.abs(got).max())
        print(f"{label}: max |d| on the surface = {worst:.3e} m (bound {bound:.3e})")
        if worst > bound:
            failures.append(f"|d| = {worst:.3e} at a query on the surface")
    if "positive" in c.checks and not (got > 0).all():
        failures.append(f"{int((got <= 0).sum())} queries outside the box are not positive")
    if "sign" in c.checks:
        keep = sign_mask(c, d_ref, w_ref)
        wrong = int(((got < 0) != (d_ref < 0))[keep].sum())
        print(f"{label}: {int((~keep).sum())} of {keep.size} queries left out of the sign check, {wrong} wrong signs")
        assert (~keep).mean() <= MC.SIGN_SKIP_MAX, f"{label}: {(~keep).mean():.3%} of the queries are left out of the sign check"
        if wrong:
            failures.append(f"{wrong} signs differ from the oracle")
    if got_wn is not None:
        got_wn = np.asarray(got_wn, np.float64).reshape(-1)
        assert np.isfinite(got_wn).all(), f"{label}: non-finite winding numbers"
        if "wn" in c.checks:
            wn_err = float(np.abs(got_wn - w_ref).max())
            print(f"{label}: max |winding - oracle| = {wn_err:.3e}")
            if wn_err > MC.WN_TOL:
                failures.append(f"winding numbers differ from the oracle by {wn_err:.3e}")
    assert not failures, f"{label}: " + "; ".join(failures)
