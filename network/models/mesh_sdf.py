"""Triangle mesh -> the trackers' SDF volume: the reference's `load_obj_oracle` (optimization_obj.py:163-182, "directly compute
the SDF volume from a mesh if we assume the mesh is known"; commented out there because it needs kaolin's
point_to_mesh_distance / check_sign) and its ground-truth cloud for the chamfer columns
(`trimesh.sample.sample_surface(mesh, 2048)`, track_network.py:398).  Nothing of kaolin, trimesh or open3d is used.

Definition (include/pn2_sdf.h): |d| = the exact minimum over all triangles of the distance to the triangle's closest point
(face, edge or vertex); inside (negative) iff the generalised winding number (1/4pi) sum_f Omega_f exceeds 0.5, Omega_f by
the Van Oosterom-Strackee formula; a degenerate triangle counts as its segment or point and has no solid angle.

Two routes with the same definition (tests/test_mesh_sdf.py, tests/test_gpu_mesh_sdf.py):
  * the kernel route (hotrack_amd/csrc/mesh_sdf.hip): fp32 tensors on the GPU, nothing of size voxels x faces is written;
  * the torch route: CPU tensors, other dtypes, or route='torch' -- the same expressions as torch operations, chunked over
    the query points so that a (points x faces) temporary stays at CHUNK_FLOATS floats.
The first time the torch route runs the reason is printed (once per reason)."""
from __future__ import annotations

import math
import struct

import numpy as np
import torch

_said = set()
CHUNK_FLOATS = 1 << 22  # torch route: elements of one (points x faces) temporary (a dozen are alive at a time)
DEGENERATE = 1e-12      # |n|^2 <= DEGENERATE |b-a|^2 |c-a|^2: the triangle is a segment or a point (include/pn2_sdf.h)
FACE_MARGIN_EPS = 8.0   # the face region ends this many eps x |point - vertex| inside each edge's line (fp32: 2^-20, the kernel's)


# ---- files ----------------------------------------------------------------------------------------------------------------
def _fan(poly):
    return [(poly[0], poly[i], poly[i + 1]) for i in range(1, len(poly) - 1)]


def _load_obj(path):
    verts, faces = [], []
    with open(path, "r", errors="replace") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f":
                poly = []
                for item in tok[1:]:  # a, a/b, a//c, a/b/c; 1-based, negative = counted from the last vertex read so far
                    i = int(item.split("/")[0])
                    poly.append(i - 1 if i > 0 else len(verts) + i)
                faces += _fan(poly)
    return verts, faces


_PLY_TYPES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H", "uint16": "H",
              "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d", "float64": "d"}


def _load_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.find(b"\n", end) + 1
    fmt, elements = None, []  # elements: [name, count, [(property name, type) | (name, count type, item type)]]
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            elements[-1][2].append((tok[4], tok[2], tok[3]) if tok[1] == "list" else (tok[2], tok[1]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
    verts, faces = [], []
    if fmt == "ascii":
        words = iter(data[body:].split())
        read = lambda typ: (float if _PLY_TYPES[typ] in "fd" else int)(next(words))
    else:
        pos = [body]

        def read(typ):
            code = "<" + _PLY_TYPES[typ]
            val = struct.unpack_from(code, data, pos[0])[0]
            pos[0] += struct.calcsize(code)
            return val
    for name, count, props in elements:
        for _ in range(count):
            row = {}
            for prop in props:
                if len(prop) == 3:
                    row[prop[0]] = [read(prop[2]) for _ in range(read(prop[1]))]
                else:
                    row[prop[0]] = read(prop[1])
            if name == "vertex":
                verts.append((row["x"], row["y"], row["z"]))
            elif name == "face":
                faces += _fan(row["vertex_indices"] if "vertex_indices" in row else row["vertex_index"])
    return verts, faces


def load_mesh(path):
    """-> (verts float32 (nv,3), faces int32 (nf,3)) numpy arrays.  Wavefront OBJ (`v` / `f` lines, `f a/b/c` forms, negative
    indices) and PLY (ASCII or binary little-endian; `vertex` x/y/z and `face` index lists, other properties and elements are
    skipped); polygons are fan-triangulated."""
    path = str(path)
    with open(path, "rb") as fh:
        ply = fh.read(3) == b"ply"
    verts, faces = _load_ply(path) if ply else _load_obj(path)
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(verts) == 0 or len(faces) == 0:
        raise ValueError(f"{path}: no vertices or no faces")
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError(f"{path}: a face index lies outside [0, {len(verts)})")
    return verts, faces.astype(np.int32)


# ---- the torch route --------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _segment(q, s, e, inv_len2):
    """Squared distance to the segment s -> e given q = point - s ((P,1) against (F,) broadcasts)."""
    d = _sub(e, s)
    t = (_dot(q, d) * inv_len2).clamp(0.0, 1.0)
    r = (q[0] - t * d[0], q[1] - t * d[1], q[2] - t * d[2])
    return _dot(r, r)


def signed_distance_torch(points, verts, faces, return_winding: bool = False):
    """The definition above as torch operations, any device / floating dtype: (M,) signed, unclamped [, (M,) winding numbers]."""
    points, verts = points.reshape(-1, 3), verts.reshape(-1, 3).to(points.dtype)
    faces = faces.reshape(-1, 3).long().to(verts.device)
    nv, nf = verts.shape[0], faces.shape[0]
    if nv == 0 or nf == 0:
        raise ValueError("the mesh is empty")
    if int(faces.min()) < 0 or int(faces.max()) >= nv:
        raise ValueError("mesh_sdf: a face index lies outside [0, number of vertices)")
    A, B, C = (tuple(verts[faces[:, k], j] for j in range(3)) for k in range(3))  # per vertex: (x, y, z), each (F,)
    e0, e2, ec = _sub(B, A), _sub(C, B), _sub(A, C)  # the edges a->b, b->c, c->a
    d00, d11, d22 = _dot(e0, e0), _dot(ec, ec), _dot(e2, e2)
    zero, one = torch.zeros_like(d00), torch.ones_like(d00)
    inv = lambda x, ok: torch.where(ok, one / torch.where(ok, x, one), zero)
    il0, il1, il2 = inv(d00, d00 > 0), inv(d22, d22 > 0), inv(d11, d11 > 0)
    # The face's side of the record in float64, as the prepare kernel builds it: the cross product of a sliver's edges cancels
    # to eps / sin(angle) of its digits, which in the queries' precision would tilt the plane.  unit normal, |edge| * margin.
    A64, B64, C64 = (tuple(x.double() for x in V) for V in (A, B, C))
    f0, f1, f2 = _sub(B64, A64), _sub(C64, A64), _sub(C64, B64)
    n64 = _cross(f0, f1)
    nn64 = _dot(n64, n64)
    proper = nn64 > DEGENERATE * _dot(f0, f0) * _dot(f1, f1)
    scale = torch.where(proper, nn64, torch.ones_like(nn64)).rsqrt()
    n = tuple((x * scale).to(verts.dtype) for x in n64)
    margin = FACE_MARGIN_EPS * torch.finfo(verts.dtype).eps
    k0, k1, k2 = ((_dot(f, f).sqrt() * margin).to(verts.dtype) for f in (f0, f2, f1))
    out = torch.empty(points.shape[0], dtype=points.dtype, device=points.device)
    wn = torch.empty_like(out)
    step = max(1, CHUNK_FLOATS // nf)
    for p0 in range(0, points.shape[0], step):
        P = tuple(points[p0:p0 + step, j, None] for j in range(3))  # (P,1) each
        a, b, c = _sub(P, A), _sub(P, B), _sub(P, C)                 # point - vertex, (P,F) each
        d2 = torch.minimum(torch.minimum(_segment(a, A, B, il0), _segment(b, B, C, il1)), _segment(c, C, A, il2))
        la, lb, lc = _dot(a, a).sqrt(), _dot(b, b).sqrt(), _dot(c, c).sqrt()
        # the face, where the projection falls inside the triangle by more than rounding: n . (edge x (point - start)) is
        # |edge| times the projection's distance inside that edge's line (include/pn2_sdf.h)
        inside = (proper & (_dot(n, _cross(e0, a)) >= k0 * la) & (_dot(n, _cross(e2, b)) >= k1 * lb)
                  & (_dot(n, _cross(ec, c)) >= k2 * lc))
        nd = _dot(a, n)
        d2 = torch.where(inside, torch.minimum(d2, nd * nd), d2)
        num = -_dot(a, _cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        # a degenerate triangle adds exactly zero, whatever rounding leaves in den (atan2(0, den < 0) would be pi)
        w_p = torch.where(proper, torch.atan2(num, den), zero).sum(dim=1) * (1.0 / (2.0 * math.pi))
        d = d2.min(dim=1)[0].sqrt()
        out[p0:p0 + step] = torch.where(w_p > 0.5, -d, d)
        wn[p0:p0 + step] = w_p
    return (out, wn) if return_winding else out


# ---- mesh -> volume -----------------------------------------------------------------------------------------------------------
def _kernel_route(route, verts) -> bool:
    if route == "torch":
        return False
    why = (f"the mesh is on {verts.device.type}" if not verts.is_cuda else
           f"the vertices are {verts.dtype}" if verts.dtype != torch.float32 else None)
    if why is not None:
        if route == "kernel":
            raise RuntimeError(f"mesh_to_volume: the kernel route needs fp32 GPU tensors ({why})")
        if why not in _said:
            _said.add(why)
            print(f"[Mesh SDF] the torch route runs: {why}")
        return False
    return True


def grid_points(res: int, voxel_scale: float, device=None) -> torch.Tensor:
    """(res^3, 3) fp32 voxel centres in the volume's element order: ((ix,iy,iz) - res//2) * voxel_scale, an fp32 product."""
    ax = (torch.arange(res, dtype=torch.int32, device=device) - res // 2).to(torch.float32) * torch.tensor(voxel_scale, dtype=torch.float32)
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)


def mesh_signed_distance(points, verts, faces, return_winding: bool = False, route=None):
    """Signed distance of points (M,3) to the mesh, by the kernel (fp32 GPU tensors) or the torch route."""
    if _kernel_route(route, verts):
        from hotrack_amd import sdf
        return sdf.mesh_signed_distance(points.to(verts.device).contiguous(), verts.contiguous(), faces.to(torch.int32).contiguous(),
                                        return_winding)
    return signed_distance_torch(points.to(verts.device), verts, faces, return_winding)


def mesh_to_volume(verts, faces, res: int, voxel_scale: float, clamp: float = 0.1, dtype=torch.float16, route=None):
    """(res,res,res) SDF volume of the mesh on the trackers' grid (voxel centre ((ix,iy,iz) - res//2) * voxel_scale), clamped to
    +-clamp and rounded once to `dtype`, on the mesh's device.  Warns when the winding number at the first corner voxel is not
    within 0.05 of 0: the mesh is open, inverted, or reaches past the volume."""
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    res = int(res)
    if res <= 1 or res % 2 == 0:
        raise ValueError(f"res must be odd and > 1, got {res}")
    if not (voxel_scale > 0 and clamp > 0):
        raise ValueError("voxel_scale and clamp must be positive")
    faces = faces.to(verts.device)
    h = res // 2
    corner = torch.full((1, 3), -h, dtype=torch.float32, device=verts.device) * torch.tensor(voxel_scale, dtype=torch.float32)
    if _kernel_route(route, verts):
        from hotrack_amd import sdf
        verts, faces = verts.contiguous(), faces.to(torch.int32).contiguous()
        vol = sdf.mesh_sdf_volume(verts, faces, res, voxel_scale, clamp, dtype)
        w0 = sdf.mesh_signed_distance(corner, verts, faces, return_winding=True)[1]
    else:
        verts = verts.float() if not verts.is_floating_point() else verts
        pts = grid_points(res, voxel_scale, verts.device).to(verts.dtype)
        d, w = signed_distance_torch(pts, verts, faces, return_winding=True)
        vol = d.clamp(-clamp, clamp).to(dtype).reshape(res, res, res)
        w0 = w[:1]
    w0 = float(w0[0])
    if abs(w0) > 0.05:
        print(f"[Mesh SDF] WARNING: winding number {w0:.3f} at the volume's corner voxel (expected 0): the mesh is open or "
              f"inverted, or it reaches past the +-{h * voxel_scale:.3f} m volume; signs may be wrong")
    return vol


def sample_surface(verts, faces, n: int, seed: int = 0) -> torch.Tensor:
    """(n,3) fp32 points uniform over the mesh's surface (faces drawn by area, then uniform barycentric coordinates), from a
    generator seeded with `seed`: the counterpart of trimesh.sample.sample_surface(mesh, n) (track_network.py:398).
    Returned on the CPU; the draw does not depend on the device the mesh lives on."""
    v = torch.as_tensor(np.array(verts) if isinstance(verts, np.ndarray) else verts).detach().cpu().double().reshape(-1, 3)
    f = torch.as_tensor(np.array(faces) if isinstance(faces, np.ndarray) else faces).detach().cpu().long().reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = torch.linalg.cross(b - a, c - a).norm(dim=-1)
    if not float(area.sum()) > 0:
        raise ValueError("sample_surface: the mesh has no area")
    g = torch.Generator().manual_seed(int(seed))
    pick = torch.multinomial(area / area.sum(), int(n), replacement=True, generator=g)
    r = torch.rand((int(n), 2), dtype=torch.float64, generator=g)
    s = r[:, :1].sqrt()  # (1 - s) a + s (1 - r2) b + s r2 c is uniform over the triangle
    return (a[pick] + (b[pick] - a[pick]) * (s * (1 - r[:, 1:])) + (c[pick] - a[pick]) * (s * r[:, 1:])).float()


# ---- volume -> mesh -----------------------------------------------------------------------------------------------------------
# Marching tetrahedra on the Kuhn split of every cell (hotrack_amd/csrc/sdf_mesh.hip states the algorithm).
# A cell's corner is named by offset bits x = 1, y = 2, z = 4.
_VM_CLASS_BITS = (1, 2, 4, 3, 5, 6, 7)                                # edge class -> offset: +x +y +z +xy +xz +yz +xyz
_VM_TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))  # xyz xzy yxz yzx zxy zyx
_VM_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))          # of a tetrahedron's corners
_vm_tables = {}


def _vm_tet_table(corners):
    """(16,6) edge ids: for every inside set of the tetrahedron with these corner bits, the corners of triangle 0 and of
    triangle 1 as edges of the tetrahedron, outward oriented.  One inside (or outside) corner i, the others j < k < l: the
    edges (i,j) (i,k) (i,l).  Two inside i < j, two outside k < l: the quad (i,k) (i,l) (j,l) (j,k) cut along (i,k)-(j,l).  A
    triangle that faces inwards has its last two corners swapped; that is decided here in integers, on twice the edges'
    midpoints against (outside corners' centroid - inside corners' centroid) scaled by the two counts."""
    xyz = [[(c >> d) & 1 for d in range(3)] for c in corners]
    mid2 = lambda e: [xyz[_VM_EDGES[e][0]][d] + xyz[_VM_EDGES[e][1]][d] for d in range(3)]
    eid = lambda p, q: _VM_EDGES.index((min(p, q), max(p, q)))
    table = [[0] * 6 for _ in range(16)]
    for m in range(1, 15):
        ins = [i for i in range(4) if (m >> i) & 1]
        outs = [i for i in range(4) if not (m >> i) & 1]
        if len(ins) == 2:
            (i, j), (k, l) = ins, outs
            tris = [[eid(i, k), eid(i, l), eid(j, l)], [eid(i, k), eid(j, l), eid(j, k)]]
        else:
            lone, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
            tris = [[eid(lone, r) for r in rest]]
        outward = [len(ins) * sum(xyz[i][d] for i in outs) - len(outs) * sum(xyz[i][d] for i in ins) for d in range(3)]
        row = []
        for tri in tris:
            p0, p1, p2 = (mid2(e) for e in tri)
            a, b = [p1[d] - p0[d] for d in range(3)], [p2[d] - p0[d] for d in range(3)]
            n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
            s = sum(n[d] * outward[d] for d in range(3))
            assert s != 0
            row += tri if s > 0 else [tri[0], tri[2], tri[1]]
        table[m][:len(row)] = row
    return table


def volume_mesh_torch(volume, voxel_scale: float, level: float = 0.0):
    """The algorithm of hotrack_amd/csrc/sdf_mesh.hip as torch operations (any device): per-voxel masks of owned crossing
    edges, their exclusive prefix, and the same popcount look-up of a triangle's corners -> (verts fp32 (nv,3), faces int32
    (nf,3)), the kernel's output index for index."""
    V = volume.detach().float()
    dev = V.device
    res = V.shape[0]
    i64 = dict(dtype=torch.int64, device=dev)
    vs = torch.tensor(float(voxel_scale), dtype=torch.float32, device=dev)
    lv = torch.tensor(float(level), dtype=torch.float32, device=dev)
    inside = V < lv
    bits = lambda o: ((o & 1), (o >> 1) & 1, o >> 2)
    lin_off = lambda o: (o & 1) * res * res + ((o >> 1) & 1) * res + (o >> 2)
    mask = torch.zeros((res, res, res), **i64)
    for c, o in enumerate(_VM_CLASS_BITS):
        lo = tuple(slice(0, res - b) for b in bits(o))
        hi = tuple(slice(b, res) for b in bits(o))
        mask[lo] |= (inside[lo] != inside[hi]).to(torch.int64) << c
    mask = mask.reshape(-1)
    popc = torch.tensor([bin(i).count("1") for i in range(128)], **i64)
    count = popc[mask]
    prefix = torch.cumsum(count, 0) - count
    verts = torch.empty((int(count.sum()), 3), dtype=torch.float32, device=dev)
    flat = V.reshape(-1)
    for c, o in enumerate(_VM_CLASS_BITS):
        v = torch.nonzero((mask >> c) & 1).reshape(-1)
        if v.numel() == 0:
            continue
        sa, sb = flat[v], flat[v + lin_off(o)]
        t = (lv - sa) / (sb - sa)
        ijk = torch.stack([v // (res * res), (v // res) % res, v % res], dim=1)
        pa = (ijk - res // 2).to(torch.float32) * vs
        step = torch.tensor(bits(o), dtype=torch.float32, device=dev) * vs
        verts[prefix[v] + popc[mask[v] & ((1 << c) - 1)]] = pa + t[:, None] * step
    # the cells that hold a crossing, in ascending linear index, and the corner flags of each as a byte
    code = torch.zeros((res - 1,) * 3, **i64)
    for o in range(8):
        code |= inside[tuple(slice(b, res - 1 + b) for b in bits(o))].to(torch.int64) << o
    cells = torch.nonzero((code > 0) & (code < 255))
    code = code[cells[:, 0], cells[:, 1], cells[:, 2]]
    lin = (cells[:, 0] * res + cells[:, 1]) * res + cells[:, 2]
    if "tets" not in _vm_tables:
        _vm_tables["tets"] = [_vm_tet_table(t) for t in _VM_TETS]
    ntri_of = torch.tensor([{0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(m).count("1")] for m in range(16)], **i64)
    m4 = torch.stack([sum(((code >> t[i]) & 1) << i for i in range(4)) for t in _VM_TETS], dim=1)  # (cells, 6)
    ntri = ntri_of[m4]
    start = (torch.cumsum(ntri.reshape(-1), 0) - ntri.reshape(-1)).reshape(-1, 6)
    faces = torch.empty((int(ntri.sum()), 3), dtype=torch.int32, device=dev)
    class_of = torch.tensor([0, 0, 1, 3, 2, 4, 5, 6], **i64)  # offset bits -> edge class
    ep = torch.tensor([e[0] for e in _VM_EDGES], **i64)
    eq = torch.tensor([e[1] for e in _VM_EDGES], **i64)
    for k, tet in enumerate(_VM_TETS):
        table = torch.tensor(_vm_tables["tets"][k], **i64)
        corner = torch.tensor(tet, **i64)
        for j in range(2):
            sel = torch.nonzero(ntri[:, k] > j).reshape(-1)
            if sel.numel() == 0:
                continue
            for q in range(3):
                e = table[m4[sel, k], 3 * j + q]
                lo, hi = corner[ep[e]], corner[eq[e]]
                at = lin[sel] + (lo & 1) * res * res + ((lo >> 1) & 1) * res + (lo >> 2)
                below = (torch.ones_like(lo) << class_of[hi ^ lo]) - 1
                faces[start[sel, k] + j, q] = (prefix[at] + popc[mask[at] & below]).to(torch.int32)
    return verts, faces


def volume_to_mesh(volume, voxel_scale: float, level: float = 0.0, route=None):
    """The level set of a (res,res,res) SDF volume as a welded, outward-oriented triangle mesh in the volume's grid (voxel centre
    ((ix,iy,iz) - res//2) * voxel_scale) -> (verts fp32 (nv,3), faces int32 (nf,3)) on the volume's device: the reference's
    sdf2mesh (optimization_obj.py:399-405) on the volume itself.  The kernel route (hotrack_amd.sdf.volume_mesh) takes fp16 /
    fp32 GPU volumes; the torch route anything else, or route='torch'.  Both give the same vertices (to fp32 rounding) in the
    same order and the same faces; a volume with no crossing gives (0,3) / (0,3)."""
    volume = torch.as_tensor(volume)
    if volume.dim() != 3 or tuple(volume.shape) != (volume.shape[0],) * 3 or volume.shape[0] < 2:
        raise ValueError(f"volume must be (res,res,res) with res >= 2, got shape {tuple(volume.shape)}")
    if not (float(voxel_scale) > 0 and math.isfinite(float(voxel_scale)) and math.isfinite(float(level))):
        raise ValueError(f"voxel_scale must be finite and > 0 and level finite, got {voxel_scale} and {level}")
    kernel = route != "torch"
    if kernel:
        why = (f"the volume is on {volume.device.type}" if not volume.is_cuda else
               f"the volume is {volume.dtype}" if volume.dtype not in (torch.float16, torch.float32) else None)
        if why is not None:
            if route == "kernel":
                raise RuntimeError(f"volume_to_mesh: the kernel route needs an fp16 / fp32 GPU volume ({why})")
            if why not in _said:
                _said.add(why)
                print(f"[Mesh SDF] the torch route runs: {why}")
            kernel = False
    if kernel:
        from hotrack_amd import sdf
        return sdf.volume_mesh(volume.contiguous(), float(voxel_scale), float(level))
    return volume_mesh_torch(volume, voxel_scale, level)


def save_mesh(path, verts, faces) -> None:
    """Write a triangle mesh as binary little-endian PLY (float x y z; uchar-counted int index lists) or, for a path ending in
    .obj, as Wavefront OBJ; `load_mesh` reads either back (the PLY bit for bit)."""
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    path = str(path)
    if path.lower().endswith(".obj"):
        with open(path, "w") as fh:
            fh.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist())
            fh.writelines("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in f.tolist())
        return
    rows = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rows["n"], rows["i"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rows.tobytes())


# ---- the trackers' side -------------------------------------------------------------------------------------------------------
_volumes = {}  # (mesh key, res, voxel_scale, device) -> volume; a dataset that repeats an object does not rebuild


def frame_mesh(frame0, device):
    """The mesh of a sequence's first frame -> (key, verts fp32 (nv,3), faces int32 (nf,3)) on `device`, or None.
    'obj_mesh': {'vertices', 'faces'} tensors / arrays (key: data pointers and shapes); 'obj_mesh_path': a file (key: the path)."""
    if "obj_mesh" in frame0:
        v, f = torch.as_tensor(frame0["obj_mesh"]["vertices"]), torch.as_tensor(frame0["obj_mesh"]["faces"])
        key = ("tensors", v.data_ptr(), tuple(v.shape), f.data_ptr(), tuple(f.shape))
    elif "obj_mesh_path" in frame0:
        key = ("path", str(frame0["obj_mesh_path"]))
        if key in _meshes:
            return (key, *_meshes[key])
        v, f = (torch.from_numpy(x) for x in load_mesh(frame0["obj_mesh_path"]))
    else:
        return None
    v, f = v.float().reshape(-1, 3).to(device).contiguous(), f.to(torch.int32).reshape(-1, 3).to(device).contiguous()
    if key[0] == "path":
        _meshes[key] = (v, f)
    return key, v, f


_meshes = {}


def frame_volume(frame0, res: int, voxel_scale: float, device):
    """The SDF volume built from the first frame's mesh (cached per mesh, size and device), or None when it carries no mesh."""
    mesh = frame_mesh(frame0, device)
    if mesh is None:
        return None
    key = (mesh[0], int(res), float(voxel_scale), str(device))
    if key not in _volumes:
        # (the frame's own tensors are kept with the volume: the key's data pointers stay theirs)
        _volumes[key] = (mesh_to_volume(mesh[1], mesh[2], res, voxel_scale), frame0.get("obj_mesh"))
    return _volumes[key][0]
