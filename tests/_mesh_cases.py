"""Test meshes and the two oracles of the mesh -> signed-distance path (include/pn2_sdf.h: pn2s_mesh_sdf_*).

(a) Closed forms: the SDF of an axis-aligned box, of a torus and of the synthetic capsule.  A box mesh has exactly the box's
    SDF; torus and capsule meshes are inscribed tessellations (every vertex on the surface), so their SDF lies within the
    tessellation's sagitta of the analytic one -- `sagitta` measures it on the mesh.
(b) `oracle`: a float64 numpy brute force of the definition -- the closest point of every triangle by Ericson's region walk
    (Real-Time Collision Detection 5.1.5; not the edge/face decomposition the kernel and the torch route use; in the face
    region the distance to the plane, so that a sliver's ill-conditioned weights do not enter), the sign from the
    generalised winding number with the Van Oosterom-Strackee solid angle.  Results are cached per (mesh, query set).

Tolerances (fp32 against float64, measured on the CPU over the three meshes x the 25^3 grid: magnitude within 3.2e-8 m, winding
number within 3.6e-6 of 0 or 1):
  MAG_TOL  3e-7 m   | |d| - |oracle| |: ten times the measured difference (FMA contraction, another association);
  SIGN_MIN 1e-5 m   signs are compared where the oracle's |d| is at least this; at most SIGN_SKIP_MAX of the points may be closer;
  WN_TOL   1e-4     winding number against the oracle's."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAG_TOL, SIGN_MIN, SIGN_SKIP_MAX, WN_TOL = 3e-7, 1e-5, 0.01, 1e-4
BOX_HALF = np.array([0.0313, 0.0471, 0.0837], dtype=np.float32).astype(np.float64)  # as the fp32 vertices hold them
TORUS_R, TORUS_r = 0.09, 0.035
TORUS_ANGLE, TORUS_SHIFT = 0.37, np.array([0.011, -0.007, 0.013])


def _torus_rot():
    c, s = np.cos(TORUS_ANGLE), np.sin(TORUS_ANGLE)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])  # rotation about y


def box_mesh():
    """12 outward-oriented faces over the 8 corners of the box with half-extents BOX_HALF."""
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * BOX_HALF
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # -x +x -y +y -z +z
    f = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v.astype(np.float32), np.array(f, dtype=np.int32)


def torus_mesh(nu, nv):
    """2 nu nv faces, vertices on the torus (R 0.09, r 0.035) rotated 0.37 rad about y and shifted by TORUS_SHIFT."""
    u = np.arange(nu) * 2 * np.pi / nu
    w = np.arange(nv) * 2 * np.pi / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    ring = TORUS_R + TORUS_r * np.cos(W)
    v = np.stack([ring * np.cos(U), ring * np.sin(U), TORUS_r * np.sin(W)], -1).reshape(-1, 3)
    v = v @ _torus_rot().T + TORUS_SHIFT
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v.astype(np.float32), np.array(f, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """'box' | 'torus24' (576 faces) | 'torus48' (2688 faces) -> (verts float32, faces int32), read-only."""
    v, f = {"box": box_mesh, "torus24": lambda: torus_mesh(24, 12), "torus48": lambda: torus_mesh(48, 28)}[name]()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


MESHES = ("box", "torus24", "torus48")


def grid(res=25, stride=0.0167):
    """(res^3, 3) float32 voxel centres in the volume's element order: ((ix,iy,iz) - res//2) * stride as an fp32 product."""
    ax = (np.arange(res) - res // 2).astype(np.float32) * np.float32(stride)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def box_sdf(p):
    q = np.abs(np.asarray(p, np.float64)) - BOX_HALF
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def torus_sdf(p):
    q = (np.asarray(p, np.float64) - TORUS_SHIFT) @ _torus_rot()  # rows: R^T (p - shift)
    return np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - TORUS_R) ** 2 + q[..., 2] ** 2) - TORUS_r


def sagitta(verts, faces, analytic_sdf, n=12):
    """Largest distance between an inscribed tessellation and the surface it samples: max |analytic_sdf| over a barycentric
    lattice of (n+1)(n+2)/2 points on every face (vertices, edge midpoints and centroid-like interior points included).  The
    mesh is a graph over the smooth surface along its normals with offsets of at most this, so the two signed distances differ
    by no more than it; 2 % are added for the lattice's own resolution."""
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    worst = 0.0
    for i in range(n + 1):
        for j in range(n + 1 - i):
            s, t = i / n, j / n
            worst = max(worst, float(np.abs(analytic_sdf(a * (1 - s - t) + b * s + c * t)).max()))
    return 1.02 * worst


# ---- the float64 brute force ------------------------------------------------------------------------------------------------------
def _d3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _s3(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _x3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _segment_dist2(p, s, e):
    d = _s3(e, s)
    ll = _d3(d, d)
    q = _s3(p, s)
    t = np.clip(_d3(q, d) / np.where(ll > 0, ll, 1.0), 0.0, 1.0)
    r = (q[0] - t * d[0], q[1] - t * d[1], q[2] - t * d[2])
    return _d3(r, r)


def oracle_uncached(points, verts, faces, chunk_elems=1 << 18):
    """-> (signed distance (M,), winding number (M,)) in float64.  Vectors are (x, y, z) tuples of (points, faces) arrays; the
    chunks of points run on a few threads (numpy releases the interpreter lock inside its loops)."""
    p_all = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(verts, np.float64)
    a, b, c = (tuple(v[faces[:, k], j][None] for j in range(3)) for k in range(3))  # (1,F) per component
    ab, ac = _s3(b, a), _s3(c, a)
    abab, abac, acac = _d3(ab, ab), _d3(ab, ac), _d3(ac, ac)
    nrm = _x3(ab, ac)
    degenerate = (_d3(nrm, nrm) <= 1e-24 * abab * acac)[0]  # (F,)
    g = np.nonzero(degenerate)[0]
    dist = np.empty(len(p_all))
    wn = np.empty(len(p_all))
    step = max(1, chunk_elems // len(faces))

    def chunk(p0):
        p = tuple(p_all[p0:p0 + step, j, None] for j in range(3))  # (P,1)
        ap = _s3(p, a)
        d1, d2 = _d3(ab, ap), _d3(ac, ap)
        d3, d4, d5, d6 = d1 - abab, d2 - abac, d1 - abac, d2 - acac  # ab.bp, ac.bp, ab.cp, ac.cp
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        inv = 1.0 / (va + vb + vc)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        # Ericson's regions in his order: A, B, edge AB, C, edge AC, edge BC, face; (sv, sw) = barycentric weights of b and c
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        sv, sw = vb * inv, vc * inv
        for cond, cv, cw in reversed(list(zip(conds, [0.0, 1.0, d1 / (d1 - d3), 0.0, 0.0, 1 - wbc], [0.0, 0.0, 0.0, 1.0, d2 / (d2 - d6), wbc]))):
            sv, sw = np.where(cond, cv, sv), np.where(cond, cw, sw)
        r = tuple(ap[k] - ab[k] * sv - ac[k] * sw for k in range(3))
        dd = _d3(r, r)
        # in the face region the closest point is the projection: the distance to the plane.  The weights' determinants lose
        # 1e-16 / sin^2 of their digits on a sliver, which slides r along the plane; the regions' sign tests and the normal do not.
        face = ~functools.reduce(np.logical_or, conds)
        dd = np.where(face, _d3(ap, nrm) ** 2 / _d3(nrm, nrm), dd)
        if len(g):  # a segment or a point: the nearest of its three (possibly empty) edges
            ag, bg, cg = (tuple(x[:, g] for x in t) for t in (a, b, c))
            dd[:, g] = np.minimum(np.minimum(_segment_dist2(p, ag, bg), _segment_dist2(p, bg, cg)), _segment_dist2(p, cg, ag))
        dist[p0:p0 + step] = np.sqrt(dd.min(-1))
        ua, ub, uc = _s3(a, p), _s3(b, p), _s3(c, p)  # vertex - point
        la, lb, lc = np.sqrt(_d3(ua, ua)), np.sqrt(_d3(ub, ub)), np.sqrt(_d3(uc, uc))
        omega = 2.0 * np.arctan2(_d3(ua, _x3(ub, uc)), la * lb * lc + _d3(ua, ub) * lc + _d3(ub, uc) * la + _d3(uc, ua) * lb)
        omega[:, degenerate] = 0.0
        wn[p0:p0 + step] = omega.sum(-1) / (4.0 * np.pi)

    with np.errstate(divide="ignore", invalid="ignore"), ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(chunk, range(0, len(p_all), step)))
    return np.where(wn > 0.5, -dist, dist), wn


@functools.lru_cache(maxsize=None)
def oracle(name, res=25, stride=0.0167):
    """The brute force for mesh `name` on grid(res, stride), computed once per process and read-only."""
    v, f = mesh(name)
    d, w = oracle_uncached(grid(res, stride), v, f)
    d.setflags(write=False)
    w.setflags(write=False)
    return d, w


def check_against_oracle(got, d_ref, got_wn=None, wn_ref=None, label=""):
    """The acceptance criteria of the header: prints each figure, then asserts."""
    got, d_ref = np.asarray(got, np.float64), np.asarray(d_ref, np.float64)
    assert np.isfinite(got).all(), f"{label}: non-finite distances"
    mag = float(np.abs(np.abs(got) - np.abs(d_ref)).max())
    near = np.abs(d_ref) < SIGN_MIN
    wrong = int(((got < 0) != (d_ref < 0))[~near].sum())
    print(f"{label}: max | |d| - |oracle| | = {mag:.3e} m, {int(near.sum())} of {near.size} points nearer than {SIGN_MIN} m left out "
          f"of the sign check, {wrong} wrong signs")
    if got_wn is not None:
        wn_err = float(np.abs(np.asarray(got_wn, np.float64) - wn_ref).max())
        print(f"{label}: max |winding - oracle| = {wn_err:.3e}")
    assert mag <= MAG_TOL, f"{label}: magnitude differs from the oracle by {mag}"
    assert near.mean() <= SIGN_SKIP_MAX, f"{label}: {near.mean():.3%} of the points are left out of the sign check"
    assert wrong == 0, f"{label}: {wrong} signs differ from the oracle"
    if got_wn is not None:
        assert wn_err <= WN_TOL, f"{label}: winding numbers differ from the oracle by {wn_err}"


def with_degenerate_faces(verts, faces):
    """The mesh plus degenerate faces: a vertex three times, an edge with a repeated end (both ways round), and three
    collinear vertices (a new vertex at the midpoint of the first face's first edge)."""
    v = np.asarray(verts, np.float32)
    i, j = int(faces[0, 0]), int(faces[0, 1])
    mid = ((v[i].astype(np.float64) + v[j].astype(np.float64)) / 2).astype(np.float32)
    v2 = np.concatenate([v, mid[None]])
    extra = np.array([[i, i, i], [i, j, j], [j, i, j], [i, len(v), j]], dtype=np.int32)
    return v2, np.concatenate([np.asarray(faces), extra])
