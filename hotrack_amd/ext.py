"""Python binding of the MI355X-side extensions (include/pn2_ext.h). GPU tensors only."""
from __future__ import annotations

import ctypes
import os

import torch

from . import pointnet2_hip as _native

_lib = _native._lib
_vp, _ci = ctypes.c_void_p, ctypes.c_int
_lib.pn2x_kabsch.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_kabsch.restype = _ci


def kabsch(x: torch.Tensor, y: torch.Tensor):
    """Rigid fit y ~= R x + t.  x (B|1, num, 3), y (B, num, 3) -> R (B,3,3), t (B,3,1)."""
    x = x.float().contiguous()
    y = y.float().contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, num, _ = y.shape
    xb = x.shape[0]
    if xb not in (1, B) or x.shape[1] != num:
        raise ValueError(f"kabsch: x {tuple(x.shape)} does not match y {tuple(y.shape)}")
    px = _native._ptr(x, "x", torch.float32, xb * num * 3)
    py = _native._ptr(y, "y", torch.float32, B * num * 3)
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=y.device)
    t = torch.empty((B, 3, 1), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _native._check(_lib.pn2x_kabsch(B, xb, num, px, py, R.data_ptr(), t.data_ptr(), _native._stream(y)), "kabsch")
    return R, t


_lib.pn2x_kabsch_backward.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_kabsch_backward.restype = _ci


def kabsch_backward(x: torch.Tensor, y: torch.Tensor, R: torch.Tensor, grad_R, grad_t) -> torch.Tensor:
    """dL/dy (B,num,3) through (R, t) = kabsch(x, y) given dL/dR (B,3,3) and dL/dt (B,3,1) (either may be None)."""
    x = x.float().contiguous()
    y = y.float().contiguous()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, num, _ = y.shape
    f32 = torch.float32
    gR = None if grad_R is None else _native._ptr(grad_R.contiguous(), "grad_R", f32, B * 9)
    gt = None if grad_t is None else _native._ptr(grad_t.contiguous(), "grad_t", f32, B * 3)
    dy = torch.empty_like(y)
    with torch.cuda.device(y.device):
        _native._check(_lib.pn2x_kabsch_backward(B, x.shape[0], num, _native._ptr(x, "x", f32, x.shape[0] * num * 3),
                                                 _native._ptr(y, "y", f32, B * num * 3), _native._ptr(R.contiguous(), "R", f32, B * 9),
                                                 gR, gt, dy.data_ptr(), _native._stream(y)), "kabsch_backward")
    return dy


class KabschFit(torch.autograd.Function):
    """(R, t) = kabsch(x, y), differentiable with respect to y: one launch forward (pn2x_kabsch), one backward."""

    @staticmethod
    def forward(ctx, x, y):
        R, t = kabsch(x, y)
        ctx.save_for_backward(x, y, R)
        return R, t

    @staticmethod
    def backward(ctx, grad_R, grad_t):
        x, y, R = ctx.saved_tensors
        return None, kabsch_backward(x, y, R, grad_R, grad_t)


_cl = ctypes.c_long
_lib.pn2x_sa_mlp_max.argtypes = [_ci] * 7 + [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _cl, _ci, _ci, _vp]
_lib.pn2x_sa_mlp_max.restype = _ci
_lib.pn2x_sa_mlp_max_supported.argtypes = [_ci] * 4
_lib.pn2x_sa_mlp_max_supported.restype = _ci
_lib.pn2x_three_nn_weights.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_three_nn_weights.restype = _ci
_lib.pn2x_three_interpolate_pm.argtypes = [_ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _ci, _vp]
_lib.pn2x_three_interpolate_pm.restype = _ci
_lib.pn2x_gather_rows.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
_lib.pn2x_gather_rows.restype = _ci
_lib.pn2x_bias_act_pm.argtypes = [_cl, _ci, _vp, _ci, _vp, _cl, _ci, _vp]
_lib.pn2x_bias_act_pm.restype = _ci


def sa_mlp_max_supported(k: int, c1: int, c2: int, c3: int) -> bool:
    return bool(_lib.pn2x_sa_mlp_max_supported(k, c1, c2, c3))


def _rows(t: torch.Tensor, name: str, cols: int):
    """Validate a point-major (B, R, >=cols) fp32 tensor whose rows may be a column block of a wider
    buffer (last dim contiguous, uniform row stride).  Returns (data_ptr, row_stride)."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError(f"{name}: expected a 3-D float32 GPU tensor")
    B, R, C = t.shape
    if C < cols or t.stride(2) != 1 or (R > 1 and B > 1 and t.stride(0) != R * t.stride(1)):
        raise ValueError(f"{name}: unsupported layout shape={tuple(t.shape)} strides={t.stride()}")
    return t.data_ptr(), t.stride(1)


def sa_mlp_max(idx: torch.Tensor, w2, b2, w3, b3, *, a1f=None, xyz=None, cxyz=None, wx=None, b1=None, cadd=None,
               out=None, point_major=False) -> torch.Tensor:
    """Fused SA scale (include/pn2_ext.h: pn2x_sa_mlp_max).
    idx (B,S,K) int32; a1f (B,N,>=C1) rows; xyz (B,N,3); cxyz (B,S,3); wx (C1,3); b1 (C1); cadd (B,S,>=C1).
    Returns (B,C3,S), or (B,S,C3) if point_major; `out` may be a (B,S,C3) column block of a wider buffer."""
    return _sa_mlp_max(idx, w2, b2, w3, b3, None, a1f, xyz, cxyz, wx, b1, cadd, out, point_major)


_lib.pn2x_sa_mlp_max_classes.argtypes = [_ci] * 7 + [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _cl, _ci, _ci, _vp]
_lib.pn2x_sa_mlp_max_classes.restype = _ci
_lib.pn2x_sa_mlp_max_classes_supported.argtypes = [_ci] * 4
_lib.pn2x_sa_mlp_max_classes_supported.restype = _ci
_lib.pn2x_sa_class_lists.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp]
_lib.pn2x_sa_class_lists.restype = _ci
_lib.pn2x_sa_class_lists2.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp] * 2 + [_vp]
_lib.pn2x_sa_class_lists2.restype = _ci


def sa_mlp_max_classes_supported(k: int, c1: int, c2: int, c3: int) -> bool:
    """Does pn2x_sa_mlp_max_classes (the fused SA scale that skips ball-query padding) cover this neighbourhood size and widths?"""
    return bool(_lib.pn2x_sa_mlp_max_classes_supported(k, c1, c2, c3))


def sa_class_partition(counts: torch.Tensor):
    """The class rule of sa_class_lists as plain torch (any device; the statement the tests hold the kernel to): counts (B,S)
    -> (ids (B*S,) int32: the centroids b*S + s with count 17..32 in ascending order, then those with 9..16, then those with
    <= 8; sizes (3,) int32)."""
    c = counts.reshape(-1)
    ids = torch.arange(c.numel(), dtype=torch.int32, device=c.device)
    masks = (c > 16, (c > 8) & (c <= 16), c <= 8)
    return torch.cat([ids[m] for m in masks]), torch.stack([m.sum() for m in masks]).to(torch.int32)


def _class_lists_args(counts, n, what):
    """Validated (B, S, n, counts pointer, list, sizes) of one partition problem."""
    if not isinstance(counts, torch.Tensor) or counts.dim() != 2 or counts.dtype != torch.int32 or not counts.is_cuda:
        raise TypeError(f"{what}: counts must be a (B,S) int32 GPU tensor")
    if int(n) < 1:
        raise ValueError(f"{what}: n >= 1")
    B, S = counts.shape
    pc = _native._ptr(counts, "counts", torch.int32, B * S)
    lst = torch.empty((B * S, 4), dtype=torch.int32, device=counts.device)
    sizes = torch.empty(3, dtype=torch.int32, device=counts.device)
    return B, S, int(n), pc, lst, sizes


def sa_class_lists(counts: torch.Tensor, n: int):
    """Class lists of the class walk from the ball query's hit counts (include/pn2_ext.h: pn2x_sa_class_lists): counts (B,S) int32
    -> (lst (B*S,4) int32 records {b*S + s, b*n, b, s}, sizes (3,) int32), one launch, nothing synchronises with the host.
    n: points per cloud of the level the index lists name."""
    B, S, n, pc, lst, sizes = _class_lists_args(counts, n, "sa_class_lists")
    with torch.cuda.device(counts.device):
        _native._check(_native._call(_lib.pn2x_sa_class_lists, "sa_class_lists2_kernel", None, B, S, n, pc, lst.data_ptr(),
                                     sizes.data_ptr(), _native._stream(counts)), "sa_class_lists")
    return lst, sizes


def sa_class_lists_pair(counts_a: torch.Tensor, n_a: int, counts_b: torch.Tensor, n_b: int):
    """sa_class_lists of two problems -- both levels of a forward -- in ONE launch (include/pn2_ext.h: pn2x_sa_class_lists2)
    -> ((lst_a, sizes_a), (lst_b, sizes_b)), each what sa_class_lists returns for its problem."""
    a = _class_lists_args(counts_a, n_a, "sa_class_lists_pair")
    b = _class_lists_args(counts_b, n_b, "sa_class_lists_pair")
    if counts_a.device != counts_b.device:
        raise ValueError("sa_class_lists_pair: both problems on one device")
    with torch.cuda.device(counts_a.device):
        _native._check(_native._call(_lib.pn2x_sa_class_lists2, "sa_class_lists2_kernel", None, *a[:4], a[4].data_ptr(), a[5].data_ptr(),
                                     *b[:4], b[4].data_ptr(), b[5].data_ptr(), _native._stream(counts_a)), "sa_class_lists_pair")
    return (a[4], a[5]), (b[4], b[5])


def sa_mlp_max_classes(idx: torch.Tensor, classes, w2, b2, w3, b3, *, a1f=None, xyz=None, cxyz=None, wx=None, b1=None, cadd=None,
                       out=None, point_major=False) -> torch.Tensor:
    """sa_mlp_max over ball-query lists without their padding (include/pn2_ext.h: pn2x_sa_mlp_max_classes): idx (B,S,32) whose
    slots past a centroid's hit count repeat slot 0, classes = sa_class_lists(counts, N).  Bit-identical to sa_mlp_max."""
    if not (isinstance(classes, (tuple, list)) and len(classes) == 2):
        raise TypeError("sa_mlp_max_classes: classes must be the (list, sizes) pair of sa_class_lists")
    return _sa_mlp_max(idx, w2, b2, w3, b3, classes, a1f, xyz, cxyz, wx, b1, cadd, out, point_major)


def _sa_mlp_max(idx, w2, b2, w3, b3, classes, a1f, xyz, cxyz, wx, b1, cadd, out, point_major, record=False):
    """The one place that validates the twelve tensors of a scale (an absent `out` is allocated, (B,C3,S) or, point_major,
    (B,S,C3)), then launches it through its positional entry -> out; or, `record`, hands the scale back as the _SaProblem of
    sa_mlp_max_pair.  (One function, not a validator the launch path calls: a record built to be read back, or a tuple passed
    through one more call, costs the positional entries 0.7 - 1.5 us of their 15 us per call.)"""
    B, S, K = idx.shape
    C1, C2, C3 = w2.shape[1], w2.shape[0], w3.shape[0]
    f32 = torch.float32
    N = a1f.shape[1] if a1f is not None else xyz.shape[1]
    pa, lda = (None, 0) if a1f is None else _rows(a1f, "a1f", C1)
    pc, ldc = (None, 0) if cadd is None else _rows(cadd, "cadd", C1)
    px = None if xyz is None else _native._ptr(xyz, "xyz", f32, B * N * 3)
    pcx = None if cxyz is None else _native._ptr(cxyz, "cxyz", f32, B * S * 3)
    pwx = None if wx is None else _native._ptr(wx, "wx", f32, C1 * 3)
    pb1 = None if b1 is None else _native._ptr(b1, "b1", f32, C1)
    pi = _native._ptr(idx, "idx", torch.int32, B * S * K)
    pw2, pb2 = _native._ptr(w2, "w2", f32, C2 * C1), _native._ptr(b2, "b2", f32, C2)
    pw3, pb3 = _native._ptr(w3, "w3", f32, C3 * C2), _native._ptr(b3, "b3", f32, C3)
    if out is None:
        out = torch.empty((B, S, C3) if point_major else (B, C3, S), dtype=f32, device=idx.device)
        ob, os_, oc = (S * C3, C3, 1) if point_major else (C3 * S, 1, S)
        po = out.data_ptr()
    else:
        po, ld = _rows(out, "out", C3)
        ob, os_, oc = out.stride(0), ld, 1
    if record:
        return _SaProblem(N, S, K, pa, lda, px, pcx, pwx, pb1, pc, ldc, pi, pw2, pb2, pw3, pb3, po, ob, os_, oc)
    if classes is not None:
        lst, sizes = classes
        pl = _native._ptr(lst, "classes list", torch.int32, B * S * 4)
        ps = _native._ptr(sizes, "classes sizes", torch.int32, 3)
        if lst.device != idx.device or sizes.device != idx.device:
            raise ValueError("sa_mlp_max_classes: classes on another device than idx")
        with torch.cuda.device(idx.device):
            _native._check(_native._call(_lib.pn2x_sa_mlp_max_classes, "sa_mlp_max_classes_kernel", None, B, N, S, K, C1, C2, C3, pa, lda,
                                         px, pcx, pwx, pb1, pc, ldc, pi, pl, ps, pw2, pb2, pw3, pb3, po, ob, os_, oc,
                                         _native._stream(idx)), "sa_mlp_max_classes")
        return out
    with torch.cuda.device(idx.device):
        _native._check(_native._call(_lib.pn2x_sa_mlp_max, "sa_mlp_max_kernel", None, B, N, S, K, C1, C2, C3, pa, lda, px, pcx,
                                     pwx, pb1, pc, ldc, pi, pw2, pb2, pw3, pb3, po, ob, os_, oc, _native._stream(idx)),
                       "sa_mlp_max")
    return out


class _SaProblem(ctypes.Structure):
    """include/pn2_ext.h: pn2x_sa_problem."""
    _fields_ = [("n", _ci), ("s", _ci), ("k", _ci), ("a1f", _vp), ("a1f_ld", _ci), ("xyz", _vp), ("cxyz", _vp), ("wx", _vp),
                ("b1", _vp), ("cadd", _vp), ("cadd_ld", _ci), ("idx", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp),
                ("out", _vp), ("out_b", _cl), ("out_s", _ci), ("out_c", _ci)]


_lib.pn2x_sa_mlp_max_pair.argtypes = [_ci] * 4 + [ctypes.POINTER(_SaProblem)] * 2 + [_vp]
_lib.pn2x_sa_mlp_max_pair.restype = _ci
_lib.pn2x_sa_mlp_max_pair_supported.argtypes = [_ci] * 5
_lib.pn2x_sa_mlp_max_pair_supported.restype = _ci


def sa_mlp_max_pair(p0: dict, p1: dict) -> None:
    """Both scales of a keypoint-query module in ONE launch (pn2x_sa_mlp_max_pair).  p0 / p1: the keyword arguments of
    sa_mlp_max (idx, w2, b2, w3, b3, a1f, xyz, cxyz, wx, b1, cadd, out -- `out` required, a (B,S,C3) row block).  Falls back
    to two launches when the combination is not covered by the pair kernel."""
    keys = ("idx", "w2", "b2", "w3", "b3", "a1f", "xyz", "cxyz", "wx", "b1", "cadd", "out")
    a = [{k: p.get(k) for k in keys} for p in (p0, p1)]
    C1, C2, C3 = a[0]["w2"].shape[1], a[0]["w2"].shape[0], a[0]["w3"].shape[0]
    same = all(tuple(a[1][k].shape) == tuple(a[0][k].shape) for k in ("w2", "w3"))
    modes = [(p["a1f"] is not None, p["xyz"] is not None, p["cadd"] is not None) for p in a]
    if not (same and modes[0] == modes[1] and modes[0][0] and modes[0][1]
            and _lib.pn2x_sa_mlp_max_pair_supported(a[0]["idx"].shape[2], a[1]["idx"].shape[2], C1, C2, C3)):
        for p in a:
            sa_mlp_max(p["idx"], p["w2"], p["b2"], p["w3"], p["b3"], a1f=p["a1f"], xyz=p["xyz"], cxyz=p["cxyz"], wx=p["wx"], b1=p["b1"],
                       cadd=p["cadd"], out=p["out"])
        return
    B = a[0]["idx"].shape[0]
    if a[0]["out"] is None or a[1]["out"] is None:
        raise TypeError("sa_mlp_max_pair: out is required")
    q0, q1 = (_sa_mlp_max(classes=None, point_major=False, record=True, **p) for p in a)
    with torch.cuda.device(a[0]["idx"].device):
        _native._check(_native._call(_lib.pn2x_sa_mlp_max_pair, "sa_mlp_max_pair_kernel", None, B, C1, C2, C3, ctypes.byref(q0),
                                     ctypes.byref(q1), _native._stream(a[0]["idx"])), "sa_mlp_max_pair")


_lib.pn2x_mlp2_rows.argtypes = [_cl] + [_ci] * 3 + [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp]
_lib.pn2x_mlp2_rows.restype = _ci
_lib.pn2x_mlp2_rows_supported.argtypes = [_ci] * 3
_lib.pn2x_mlp2_rows_supported.restype = _ci


_lib.pn2x_sa_set_compute_units.argtypes = [_ci]
_lib.pn2x_sa_set_compute_units.restype = _ci


def sa_set_compute_units(n: int) -> None:
    """CUs the persistent SA grids may occupy (0 = all): a serving loop with several batches in flight leaves a few to the
    other stream (include/pn2_ext.h: pn2x_sa_set_compute_units)."""
    _native._check(_lib.pn2x_sa_set_compute_units(int(n)), "sa_set_compute_units")


def mlp2_rows_supported(c1: int, c2: int, c3: int) -> bool:
    return bool(_lib.pn2x_mlp2_rows_supported(c1, c2, c3))


def mlp2_rows(x: torch.Tensor, w2, b2, w3, b3, out: torch.Tensor = None, w2e=None) -> torch.Tensor:
    """relu(relu(x[:, :c1] W2^T + x[:, c1:c1+3] W2e^T + b2) W3^T + b3) over the rows of a 2-D float32 GPU tensor (last dim
    contiguous, any row stride) in one launch (include/pn2_ext.h: pn2x_mlp2_rows).  `w2e` (c2, 3) or None; `out` may be a
    column block of a wider buffer whose row stride is a multiple of 4 floats and whose first element is 16-byte aligned (rows are
    stored as 16-byte quads)."""
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("mlp2_rows: x must be a 2-D float32 GPU tensor with a contiguous last dimension")
    R = x.shape[0]
    C1, C2, C3 = w2.shape[1], w2.shape[0], w3.shape[0]
    f32 = torch.float32
    ldx = x.stride(0) if R > 1 else x.shape[1]
    if x.shape[1] < C1 + (3 if w2e is not None else 0) or (w2e is not None and ldx < C1 + 4):
        raise ValueError("mlp2_rows: x has too few columns")
    if out is None:
        out = torch.empty((R, C3), dtype=f32, device=x.device)
    if out.dim() != 2 or out.shape[0] != R or out.shape[1] < C3 or out.stride(1) != 1 or out.dtype != f32 or out.device != x.device:
        raise ValueError("mlp2_rows: out must be (rows, >= c3) float32 on the same device")
    if (R > 1 and out.stride(0) % 4) or out.data_ptr() % 16:
        raise ValueError("mlp2_rows: out needs a row stride that is a multiple of 4 floats and a 16-byte aligned first element")
    with torch.cuda.device(x.device):
        _native._check(_native._call(_lib.pn2x_mlp2_rows, "mlp2_rows_kernel", None, R, C1, C2, C3, x.data_ptr(), ldx,
                                     _native._ptr(w2, "w2", f32, C2 * C1), None if w2e is None else _native._ptr(w2e, "w2e", f32, C2 * 3),
                                     _native._ptr(b2, "b2", f32, C2), _native._ptr(w3, "w3", f32, C3 * C2),
                                     _native._ptr(b3, "b3", f32, C3), out.data_ptr(), out.stride(0) if R > 1 else out.shape[1], _native._stream(x)),
                       "mlp2_rows")
    return out


def three_nn_weights(unknown: torch.Tensor, known: torch.Tensor):
    """unknown (B,n,3), known (B,m>=3,3) -> (weight (B,n,3) normalised inverse distances, idx (B,n,3) int32)."""
    B, n, _ = unknown.shape
    m = known.shape[1]
    f32 = torch.float32
    w = torch.empty((B, n, 3), dtype=f32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
    with torch.cuda.device(unknown.device):
        _native._check(_lib.pn2x_three_nn_weights(B, n, m, _native._ptr(unknown, "unknown", f32, B * n * 3),
                                                  _native._ptr(known, "known", f32, B * m * 3), w.data_ptr(), idx.data_ptr(),
                                                  _native._stream(unknown)), "three_nn_weights")
    return w, idx


def three_interpolate_pm(points: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """points (B,M,C) rows, idx/weight (B,n,3) -> out (B,n,C) rows (may be a column block of a wider buffer)."""
    B, M, C = points.shape
    n = idx.shape[1]
    pp, ldp = _rows(points, "points", C)
    po, ldo = _rows(out, "out", C)
    with torch.cuda.device(points.device):
        _native._check(_lib.pn2x_three_interpolate_pm(B, C, M, n, pp, ldp, _native._ptr(idx, "idx", torch.int32, B * n * 3),
                                                      _native._ptr(weight, "weight", torch.float32, B * n * 3), po, ldo,
                                                      _native._stream(points)), "three_interpolate_pm")
    return out


_lib.pn2x_three_nn_interpolate_pm.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _ci, _vp]
_lib.pn2x_three_nn_interpolate_pm.restype = _ci
_lib.pn2x_three_nn_interpolate_pm_supported.argtypes = [_ci] * 6
_lib.pn2x_three_nn_interpolate_pm_supported.restype = _ci
_lib.pn2x_three_nn_interpolate_pm_rows.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp]
_lib.pn2x_three_nn_interpolate_pm_rows.restype = _ci
_lib.pn2x_three_nn_interpolate_pm_rows_supported.argtypes = [_ci] * 6
_lib.pn2x_three_nn_interpolate_pm_rows_supported.restype = _ci
_lib.pn2x_three_nn_interpolate_pm_rows_act.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _ci, _vp]
_lib.pn2x_three_nn_interpolate_pm_rows_act.restype = _ci
_lib.pn2x_three_nn_interpolate_pm_rows_act_supported.argtypes = [_ci] * 6
_lib.pn2x_three_nn_interpolate_pm_rows_act_supported.restype = _ci


def three_nn_interpolate_pm(unknown: torch.Tensor, known: torch.Tensor, points: torch.Tensor, out: torch.Tensor, rows=None,
                            wx: torch.Tensor = None, bias: torch.Tensor = None, relu: bool = False) -> torch.Tensor:
    """out (B,n,C) rows <- three_interpolate_pm(points, *three_nn_weights(unknown, known)[::-1]) -- one launch when the sizes are
    covered (include/pn2_ext.h: pn2x_three_nn_interpolate_pm), the two launches otherwise; same floats either way.
    rows=(lst, counts), the pair row_lists returns: only the rows lst[b, :counts[b, 1]] of cloud b are searched, blended and
    written (pn2x_three_nn_interpolate_pm_rows, always one launch); every other row of `out` is left as it is.
    wx (C,3) and bias (C,): the rows get act(blend + wx @ unknown[row] + bias) instead, act = ReLU when `relu`
    (pn2x_three_nn_interpolate_pm_rows_act: the blend in the same order, then the x, y, z terms as one fma each, then the bias) -- the
    listed rows with rows=..., every row without; always one launch."""
    if (wx is None) != (bias is None) or (wx is None and relu):
        raise ValueError("three_nn_interpolate_pm: wx, bias (and relu) come together")
    if rows is not None:
        if not (isinstance(rows, (tuple, list)) and len(rows) == 2 and all(isinstance(t, torch.Tensor) for t in rows)):
            raise TypeError("three_nn_interpolate_pm: rows must be the (list, counts) pair of row_lists")
        if rows[0].dtype != torch.int32 or rows[1].dtype != torch.int32:
            raise TypeError("three_nn_interpolate_pm: rows must be int32 tensors")
        if tuple(rows[0].shape) != tuple(unknown.shape[:2]) or tuple(rows[1].shape) != (unknown.shape[0], 2):
            raise ValueError("three_nn_interpolate_pm: rows must be list (B,n) and counts (B,2)")
    B, n, _ = unknown.shape
    m, C = known.shape[1], points.shape[2]
    pp, ldp = _rows(points, "points", C)
    po, ldo = _rows(out, "out", C)
    f32 = torch.float32
    if rows is not None or wx is not None:
        if not (_lib.pn2x_three_nn_interpolate_pm_rows_supported(B, n, m, C, ldp, ldo) and pp % 16 == 0 and po % 16 == 0):
            raise ValueError("three_nn_interpolate_pm: rows / wx need 3 <= m <= 2048 known points, C and the row strides multiples "
                             "of 4 and 16-byte aligned points / out")
        if rows is not None and (rows[0].device != points.device or rows[1].device != points.device):
            raise ValueError("three_nn_interpolate_pm: rows on another device than points")
        if wx is not None:
            if not _lib.pn2x_three_nn_interpolate_pm_rows_act_supported(B, n, m, C, ldp, ldo):
                raise ValueError("three_nn_interpolate_pm: the wx / bias epilogue covers C <= 1024")
            pw, pb = _native._ptr(wx, "wx", f32, C * 3), _native._ptr(bias, "bias", f32, C)
            if tuple(wx.shape) != (C, 3) or tuple(bias.shape) != (C,) or pw % 16 or pb % 16:
                raise ValueError("three_nn_interpolate_pm: wx must be (C,3) and bias (C,), both 16-byte aligned")
            pl = None if rows is None else _native._ptr(rows[0], "rows list", torch.int32, B * n)
            pc = None if rows is None else _native._ptr(rows[1], "rows counts", torch.int32, B * 2)
            with torch.cuda.device(points.device):
                _native._check(_native._call(_lib.pn2x_three_nn_interpolate_pm_rows_act, "three_nn_interp_act_kernel", None, B, n, m, C,
                                             _native._ptr(unknown, "unknown", f32, B * n * 3), _native._ptr(known, "known", f32, B * m * 3),
                                             pp, ldp, po, ldo, pl, pc, pw, pb, 1 if relu else 0, _native._stream(points)),
                               "three_nn_interpolate_pm")
            return out
        with torch.cuda.device(points.device):
            _native._check(_native._call(_lib.pn2x_three_nn_interpolate_pm_rows, "three_nn_interp_kernel", None, B, n, m, C,
                                         _native._ptr(unknown, "unknown", f32, B * n * 3), _native._ptr(known, "known", f32, B * m * 3),
                                         pp, ldp, po, ldo, _native._ptr(rows[0], "rows list", torch.int32, B * n),
                                         _native._ptr(rows[1], "rows counts", torch.int32, B * 2), _native._stream(points)),
                           "three_nn_interpolate_pm")
        return out
    if _lib.pn2x_three_nn_interpolate_pm_supported(B, n, m, C, ldp, ldo) and pp % 16 == 0 and po % 16 == 0:
        with torch.cuda.device(points.device):
            _native._check(_native._call(_lib.pn2x_three_nn_interpolate_pm, "three_nn_interp_kernel", None, B, n, m, C,
                                         _native._ptr(unknown, "unknown", f32, B * n * 3), _native._ptr(known, "known", f32, B * m * 3),
                                         pp, ldp, po, ldo, _native._stream(points)), "three_nn_interpolate_pm")
        return out
    w, i3 = three_nn_weights(unknown, known)
    return three_interpolate_pm(points, i3, w, out)


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """src (B,N,C) contiguous, idx (B,M) int32 -> (B,M,C)."""
    B, N, C = src.shape
    M = idx.shape[1]
    out = torch.empty((B, M, C), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _native._check(_lib.pn2x_gather_rows(B, N, M, C, _native._ptr(src, "src", torch.float32, B * N * C),
                                             _native._ptr(idx, "idx", torch.int32, B * M), out.data_ptr(),
                                             _native._stream(src)), "gather_rows")
    return out


def bias_act_pm_(y: torch.Tensor, bias: torch.Tensor, rows_per_bias: int, relu: bool = True) -> torch.Tensor:
    """In place on point-major y (B,R,C): y[b,r,:] = act(y[b,r,:] + bias[(b*R+r)//rows_per_bias, :])."""
    B, R, C = y.shape
    py, ldy = _rows(y, "y", C)
    with torch.cuda.device(y.device):
        _native._check(_lib.pn2x_bias_act_pm(B * R, C, py, ldy, _native._ptr(bias.contiguous(), "bias", torch.float32, bias.numel()),
                                             rows_per_bias, 1 if relu else 0, _native._stream(y)), "bias_act_pm")
    return y


_lib.pn2x_bias_act.argtypes = [_ci, _ci, _ci, _vp, _vp, _ci, _vp]
_lib.pn2x_bias_act.restype = _ci


def bias_act_(y: torch.Tensor, bias: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """In place y[b,c,n] = act(y + bias[c]); y (B,C,N) contiguous fp32."""
    B, C, N = y.shape
    py = _native._ptr(y, "y", torch.float32, B * C * N)
    pb = _native._ptr(bias, "bias", torch.float32, C)
    with torch.cuda.device(y.device):
        _native._check(_lib.pn2x_bias_act(B, C, N, py, pb, 1 if relu else 0, _native._stream(y)), "bias_act")
    return y


_lib.pn2x_max_rows.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp]
_lib.pn2x_max_rows.restype = _ci


def max_rows(x: torch.Tensor) -> torch.Tensor:
    """x (B,R,C) contiguous -> (B,C) max over the R rows."""
    B, R, C = x.shape
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _native._check(_lib.pn2x_max_rows(B, R, C, _native._ptr(x, "x", torch.float32, B * R * C), out.data_ptr(),
                                          _native._stream(x)), "max_rows")
    return out


_lib.pn2x_hand_frame.argtypes = [_ci] * 5 + [_vp] * 4 + [ctypes.c_float] + [_vp] * 5 + [_ci, _vp, _vp]
_lib.pn2x_hand_frame.restype = _ci


def _xyz_cols(t: torch.Tensor, name: str, B: int, R: int):
    """A (B, R, 3) column block of a wider fp32 row buffer -> (data_ptr, row stride)."""
    if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (B, R, 3) or t.stride(2) != 1 or \
            (B > 1 and t.stride(0) != R * t.stride(1)):
        raise ValueError(f"{name}: expected a (B,{R},3) float32 column block with uniform row stride, got {tuple(t.shape)} {t.stride()}")
    return t.data_ptr(), t.stride(1)


def hand_frame(palm_template: torch.Tensor, kp: torch.Tensor, palm_idx: torch.Tensor, points: torch.Tensor, scale: float,
               xyz2_copy: torch.Tensor = None, nonfinite: torch.Tensor = None):
    """Kabsch(palm_template -> kp[:, palm_idx]) + canonicalisation in one launch.
    Returns R (B,3,3), t (B,3,1), xyz2 (B,N,3), xyz1 (B,J,3).  xyz2_copy: a (B,N,3) column block of a consumer's row
    buffer that receives a second copy of xyz2.  nonfinite: (B,) int32 that receives 1 for frames with a NaN / Inf input."""
    if palm_template.dim() == 2:
        palm_template = palm_template.unsqueeze(0)
    palm_template, kp, points = palm_template.float().contiguous(), kp.float().contiguous(), points.float().contiguous()
    B, N, _ = points.shape
    J = kp.shape[1]
    xb, num = palm_template.shape[0], palm_template.shape[1]
    f32 = torch.float32
    R = torch.empty((B, 3, 3), dtype=f32, device=points.device)
    t = torch.empty((B, 3, 1), dtype=f32, device=points.device)
    xyz2 = torch.empty((B, N, 3), dtype=f32, device=points.device)
    xyz1 = torch.empty((B, J, 3), dtype=f32, device=points.device)
    pc, ldc = (None, 0) if xyz2_copy is None else _xyz_cols(xyz2_copy, "xyz2_copy", B, N)
    with torch.cuda.device(points.device):
        _native._check(_lib.pn2x_hand_frame(B, xb, num, N, J, _native._ptr(palm_template, "palm_template", f32, xb * num * 3),
                                             _native._ptr(kp, "kp", f32, B * J * 3), _native._ptr(palm_idx, "palm_idx", torch.int32, num),
                                             _native._ptr(points, "points", f32, B * N * 3), float(scale), R.data_ptr(), t.data_ptr(),
                                             xyz2.data_ptr(), xyz1.data_ptr(), pc, ldc,
                                             None if nonfinite is None else _native._ptr(nonfinite, "nonfinite", torch.int32, B),
                                             _native._stream(points)), "hand_frame")
    return R, t, xyz2, xyz1


_cf = ctypes.c_float
_lib.pn2x_add_layernorm.argtypes = [_cl, _ci, _vp, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _cf, _vp, _vp]
_lib.pn2x_add_layernorm.restype = _ci
_lib.pn2x_pose_head.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _vp, _vp]
_lib.pn2x_pose_head.restype = _ci


def add_layernorm(x: torch.Tensor, ln1, y: torch.Tensor = None, bias: torch.Tensor = None, ln2=None) -> torch.Tensor:
    """LN2(LN1(x + y + bias)) over the last dim of row-major x (rows, C); ln1 / ln2 are nn.LayerNorm modules
    (ln2 optional), y (rows, C) and bias (C,) optional.  One launch (include/pn2_ext.h: pn2x_add_layernorm)."""
    rows, C = x.shape
    f32 = torch.float32
    px = _native._ptr(x, "x", f32, rows * C)
    py = None if y is None else _native._ptr(y, "y", f32, rows * C)
    pb = None if bias is None else _native._ptr(bias, "bias", f32, C)
    for ln in (ln1, ln2):
        if ln is not None and (tuple(ln.normalized_shape) != (C,) or ln.weight is None or ln.bias is None):
            raise ValueError("add_layernorm: LayerNorm over the last dimension with affine parameters expected")
    g1, b1 = _native._ptr(ln1.weight, "ln1.weight", f32, C), _native._ptr(ln1.bias, "ln1.bias", f32, C)
    g2 = b2 = None
    eps2 = 0.0
    if ln2 is not None:
        g2, b2, eps2 = _native._ptr(ln2.weight, "ln2.weight", f32, C), _native._ptr(ln2.bias, "ln2.bias", f32, C), ln2.eps
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _native._check(_lib.pn2x_add_layernorm(rows, C, px, py, pb, g1, b1, ln1.eps, g2, b2, eps2, out.data_ptr(), _native._stream(x)),
                       "add_layernorm")
    return out


_lib.pn2x_perm_sum_rows.argtypes = [_ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp, _vp]
_lib.pn2x_perm_sum_rows.restype = _ci
_lib.pn2x_add_layernorm_perm.argtypes = [_ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _cf, _vp, _vp]
_lib.pn2x_add_layernorm_perm.restype = _ci
_lib.pn2x_add_layernorm_perm_any_slots.argtypes = _lib.pn2x_add_layernorm_perm.argtypes  # the run-time-slot kernel at every re
_lib.pn2x_add_layernorm_perm_any_slots.restype = _ci


def _perm_args(z: torch.Tensor, perm: torch.Tensor, c: int, name: str):
    """z (B*J, >= re*c) product rows (last dim contiguous) and the HOST (J, re) int32 table -> (B, J, re, ldz)."""
    if not z.is_cuda or z.dtype != torch.float32 or z.dim() != 2 or z.stride(1) != 1:
        raise TypeError(f"{name}: z must be 2-D float32 GPU rows with a contiguous last dimension")
    if perm.is_cuda or perm.dtype != torch.int32 or perm.dim() != 2 or not perm.is_contiguous():
        raise TypeError(f"{name}: perm must be a contiguous (J, re) int32 CPU tensor (the library reads it on the host)")
    J, re = perm.shape
    if z.shape[0] % J or z.shape[1] < re * c:
        raise ValueError(f"{name}: z {tuple(z.shape)} does not hold whole groups of {J} tokens with {re} slots of {c} channels")
    return z.shape[0] // J, J, re, z.stride(0)


def perm_sum_rows(z: torch.Tensor, perm: torch.Tensor, c: int) -> torch.Tensor:
    """out[b,t,:] = sum_r z[b*J + perm[t,r], r*c:(r+1)*c] -> (B, J, c): rearrange_module's slot sum taken after the product
    with the stacked slot weights (include/pn2_ext.h: pn2x_perm_sum_rows).  perm: (J, re) int32 on the CPU."""
    B, J, re, ldz = _perm_args(z, perm, c, "perm_sum_rows")
    out = torch.empty((B, J, c), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _native._check(_lib.pn2x_perm_sum_rows(B, J, re, c, z.data_ptr(), ldz, perm.data_ptr(), out.data_ptr(), _native._stream(z)),
                       "perm_sum_rows")
    return out


def add_layernorm_perm(z: torch.Tensor, perm: torch.Tensor, ln1, bias: torch.Tensor = None, ln2=None, fixed_slots: bool = True) -> torch.Tensor:
    """LN2(LN1(perm_sum_rows(z, perm, C) + bias)) -> (B*J, C) in one launch (include/pn2_ext.h: pn2x_add_layernorm_perm);
    C is the LayerNorms' width, ln2 and bias optional.  fixed_slots = False: the run-time-slot kernel even at re = 5
    (pn2x_add_layernorm_perm_any_slots: same bits, for comparison)."""
    C = int(ln1.normalized_shape[-1])
    f32 = torch.float32
    for ln in (ln1, ln2):
        if ln is not None and (tuple(ln.normalized_shape) != (C,) or ln.weight is None or ln.bias is None):
            raise ValueError("add_layernorm_perm: LayerNorm over the last dimension with affine parameters expected")
    B, J, re, ldz = _perm_args(z, perm, C, "add_layernorm_perm")
    pb = None if bias is None else _native._ptr(bias, "bias", f32, C)
    g1, b1 = _native._ptr(ln1.weight, "ln1.weight", f32, C), _native._ptr(ln1.bias, "ln1.bias", f32, C)
    g2 = b2 = None
    eps2 = 0.0
    if ln2 is not None:
        g2, b2, eps2 = _native._ptr(ln2.weight, "ln2.weight", f32, C), _native._ptr(ln2.bias, "ln2.bias", f32, C), ln2.eps
    out = torch.empty((B * J, C), dtype=f32, device=z.device)
    with torch.cuda.device(z.device):
        args = (B, J, re, C, z.data_ptr(), ldz, perm.data_ptr(), pb, g1, b1, ln1.eps, g2, b2, eps2, out.data_ptr(), _native._stream(z))
        _native._check(_lib.pn2x_add_layernorm_perm(*args) if fixed_slots else _lib.pn2x_add_layernorm_perm_any_slots(*args),
                       "add_layernorm_perm")
    return out


def pose_head(h: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, xyz1: torch.Tensor, R: torch.Tensor, t: torch.Tensor, scale: float,
              nonfinite: torch.Tensor = None):
    """h (B*J, C), w (3, C), bias (3,), xyz1 (B,J,3), R (B,3,3), t (B,3,1) -> (kp_hand (B,J,3), kp_cam (B,J,3)):
    kp_hand = h w^T + bias + xyz1;  kp_cam = (kp_hand R^T) * scale + t  (include/pn2_ext.h: pn2x_pose_head)."""
    B, J, _ = xyz1.shape
    C = h.shape[1]
    f32 = torch.float32
    ptrs = (_native._ptr(h, "h", f32, B * J * C), _native._ptr(w, "w", f32, 3 * C), _native._ptr(bias, "bias", f32, 3),
            _native._ptr(xyz1, "xyz1", f32, B * J * 3), _native._ptr(R, "R", f32, B * 9), _native._ptr(t, "t", f32, B * 3))
    kp_hand = torch.empty((B, J, 3), dtype=f32, device=h.device)
    kp_cam = torch.empty((B, J, 3), dtype=f32, device=h.device)
    with torch.cuda.device(h.device):
        _native._check(_lib.pn2x_pose_head(B, J, C, *ptrs, float(scale), kp_hand.data_ptr(), kp_cam.data_ptr(),
                                            None if nonfinite is None else _native._ptr(nonfinite, "nonfinite", torch.int32, B),
                                            _native._stream(h)), "pose_head")
    return kp_hand, kp_cam


_lib.pn2x_linear_small.argtypes = [_ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp]
_lib.pn2x_linear_small.restype = _ci
# where pn2x_linear_small beats the library's best recorded solution (scripts/probes/linear_small_bench.py, profiles/
# r03_linear_small.json): 2 ... 512 rows, reductions up to 384 deep, up to 512 outputs -- e.g. 128 x 128 -> 256: 4.7 vs 20 us,
# 128 x 131 -> 128: 7.0 vs 12.8; it loses on one row, on deep reductions (21 x 1024 -> 384: 17 vs 5.9) and from ~1000 rows
LINEAR_SMALL_MAX_ROWS = 512
LINEAR_SMALL_MAX_K, LINEAR_SMALL_MAX_N = 384, 512


def linear(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor = None, relu: bool = False) -> torch.Tensor:
    """act(x w^T + bias) for x (M, K) rows, w (N, K): small problems (the B = 1 / B = 8 tracking loop; bounds above) through
    pn2x_linear_small (one workgroup per 32 x 32 output block), everything else through the BLAS library (torch, with its fused bias + ReLU epilogue).  Inference only."""
    M, K = x.shape
    N = w.shape[0]
    if (M > LINEAR_SMALL_MAX_ROWS or M < 2 or K > LINEAR_SMALL_MAX_K or N > LINEAR_SMALL_MAX_N or not x.is_cuda or x.dtype != torch.float32 or w.dtype != torch.float32 or x.stride(1) != 1
            or w.stride(1) != 1 or (bias is not None and not bias.is_contiguous()) or torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)):
        if relu and bias is not None:
            return torch._addmm_activation(bias, x, w.t())
        y = torch.nn.functional.linear(x, w, bias)
        return torch.relu_(y) if relu else y
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _native._check(_lib.pn2x_linear_small(M, K, N, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0),
                                              None if bias is None else bias.data_ptr(), 1 if relu else 0, y.data_ptr(), N,
                                              _native._stream(x)), "linear_small")
    return y


_lib.pn2x_ln_linear_small.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _cf, _vp, _vp, _ci, _vp, _ci, _vp, _ci, _vp]
_lib.pn2x_ln_linear_small.restype = _ci
LN_LINEAR_MAX_ROWS = 256  # 0: always the two launches (B = 8: 0.419 -> 0.410 ms with 168 rows through it)


def ln_linear_supported(rows: int, c: int) -> bool:
    """The LayerNorm launch in front of a small Linear folded into it (pn2x_ln_linear_small): few rows, c <= 384."""
    return 0 < rows <= LN_LINEAR_MAX_ROWS and c <= 384


def ln_linear(x: torch.Tensor, ln1, w: torch.Tensor, bias: torch.Tensor = None, relu: bool = False, y: torch.Tensor = None,
              ybias: torch.Tensor = None, ln2=None):
    """(xn, act(xn w^T + bias)) with xn = ln2(ln1(x + y + ybias)) over the last dimension of x (rows, C) -- add_layernorm and
    linear in one launch (include/pn2_ext.h: pn2x_ln_linear_small; same bits as the two).  Inference only."""
    rows, C = x.shape
    N = w.shape[0]
    f32 = torch.float32
    for ln in (ln1, ln2):
        if ln is not None and (tuple(ln.normalized_shape) != (C,) or ln.weight is None or ln.bias is None):
            raise ValueError("ln_linear: LayerNorm over the last dimension with affine parameters expected")
    if x.dtype != f32 or not x.is_cuda or not x.is_contiguous() or w.dtype != f32 or w.stride(1) != 1 or w.shape[1] != C:
        raise TypeError("ln_linear: contiguous float32 GPU rows and a (N, C) float32 weight expected")
    if y is not None and (y.shape != x.shape or not y.is_contiguous() or y.dtype != f32):
        raise TypeError("ln_linear: y must match x")
    xn = torch.empty_like(x)
    out = torch.empty((rows, N), dtype=f32, device=x.device)
    with torch.cuda.device(x.device):
        _native._check(_lib.pn2x_ln_linear_small(
            rows, C, N, x.data_ptr(), None if y is None else y.data_ptr(), None if ybias is None else _native._ptr(ybias, "ybias", f32, C),
            _native._ptr(ln1.weight, "ln1.weight", f32, C), _native._ptr(ln1.bias, "ln1.bias", f32, C), ln1.eps,
            None if ln2 is None else _native._ptr(ln2.weight, "ln2.weight", f32, C), None if ln2 is None else _native._ptr(ln2.bias, "ln2.bias", f32, C),
            0.0 if ln2 is None else ln2.eps, xn.data_ptr(), w.data_ptr(), w.stride(0), None if bias is None else _native._ptr(bias, "bias", f32, N),
            1 if relu else 0, out.data_ptr(), N, _native._stream(x)), "ln_linear_small")
    return xn, out


_lib.pn2x_knn_indices.argtypes = [_ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_knn_indices.restype = _ci


def knn_indices(k: int, unknown: torch.Tensor, known: torch.Tensor, k2: int = 0):
    """Indices (B,n,k) int32 of the k nearest `known` points of every `unknown` point, sorted by (distance, index) --
    pointnet2_utils.knn without the sqrt / distance output the caller would discard.  k2 > 0: also the first k2 of
    every list as a second contiguous (B,n,k2) tensor (returns a pair)."""
    B, n, _ = unknown.shape
    m = known.shape[1]
    pu, pk = _native._ptr(unknown, "unknown", torch.float32, B * n * 3), _native._ptr(known, "known", torch.float32, B * m * 3)
    idx = torch.empty((B, n, k), dtype=torch.int32, device=unknown.device)
    idx2 = torch.empty((B, n, k2), dtype=torch.int32, device=unknown.device) if k2 else None
    with torch.cuda.device(unknown.device):
        _native._check(_lib.pn2x_knn_indices(B, n, m, k, k2, pu, pk, idx.data_ptr(), None if idx2 is None else idx2.data_ptr(),
                                             _native._stream(unknown)), "knn_indices")
    return (idx, idx2) if k2 else idx


_lib.pn2x_furthest_point_sampling_radii.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _vp]
_lib.pn2x_furthest_point_sampling_radii.restype = _ci
_lib.pn2x_fps_radii_knn.argtypes = [_ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp]
_lib.pn2x_fps_radii_knn.restype = _ci
_lib.pn2x_fps_radii_knn_supported.argtypes = [_ci, _ci, _ci]
_lib.pn2x_fps_radii_knn_supported.restype = _ci
_lib.pn2x_fps_prefix_ties.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_fps_prefix_ties.restype = _ci
_lib.pn2x_fps_prefix_flags.argtypes = [_ci]
_lib.pn2x_fps_prefix_flags.restype = _ci
_lib.pn2x_furthest_point_sampling_prefix.argtypes = [_ci, _ci, _ci, _vp, _vp, _ci, _vp, _vp]
_lib.pn2x_furthest_point_sampling_prefix.restype = _ci


_lib.pn2x_ball_query_picks.argtypes = [_ci, _ci, _ci, ctypes.c_float, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp]
_lib.pn2x_ball_query_picks.restype = _ci
_lib.pn2x_ball_query_picks_counts.argtypes = [_ci, _ci, _ci, ctypes.c_float, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp]
_lib.pn2x_ball_query_picks_counts.restype = _ci


def ball_query_picks(radius: float, nsample: int, xyz: torch.Tensor, picks: torch.Tensor, xyz_copy: torch.Tensor = None,
                     counts: bool = False):
    """Ball query around the centroids xyz[picks] (picks (B,S) int32 from FPS) -> (idx (B,S,nsample) int32,
    new_xyz (B,S,3) = the centroids' coordinates): pointnet2_utils.ball_query + the gather before it, one launch.
    xyz_copy: a (B,S,3) column block of a consumer's row buffer that receives a second copy of new_xyz.
    counts=True: a third value, (B,S) int32 = min(hits, nsample) per centroid, 1 where nothing was hit (same launch)."""
    B, N, _ = xyz.shape
    S = picks.shape[1]
    px = _native._ptr(xyz, "xyz", torch.float32, B * N * 3)
    pp = _native._ptr(picks, "picks", torch.int32, B * S)
    idx = torch.empty((B, S, nsample), dtype=torch.int32, device=xyz.device)
    new_xyz = torch.empty((B, S, 3), dtype=torch.float32, device=xyz.device)
    pc, ldc = (None, 0) if xyz_copy is None else _xyz_cols(xyz_copy, "xyz_copy", B, S)
    with torch.cuda.device(xyz.device):
        if counts:
            cnt = torch.empty((B, S), dtype=torch.int32, device=xyz.device)
            _native._check(_lib.pn2x_ball_query_picks_counts(B, N, S, float(radius), nsample, px, pp, new_xyz.data_ptr(), idx.data_ptr(),
                                                              pc, ldc, cnt.data_ptr(), _native._stream(xyz)), "ball_query_picks")
            return idx, new_xyz, cnt
        _native._check(_lib.pn2x_ball_query_picks(B, N, S, float(radius), nsample, px, pp, new_xyz.data_ptr(), idx.data_ptr(),
                                                   pc, ldc, _native._stream(xyz)), "ball_query_picks")
    return idx, new_xyz


FPS_KNN_COLAUNCH = True  # (module attributes: tests compare the co-launches with the separate launches)
BALL_TIE_COLAUNCH = True
_lib.pn2x_ball_query_picks_ties.argtypes = [_ci, _ci, _ci, ctypes.c_float, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp]
_lib.pn2x_ball_query_picks_ties.restype = _ci
_lib.pn2x_ball_query_picks_ties_counts.argtypes = [_ci, _ci, _ci, ctypes.c_float, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp]
_lib.pn2x_ball_query_picks_ties_counts.restype = _ci
_lib.pn2x_ball_query_picks_ties_supported.argtypes = [_ci] * 4
_lib.pn2x_ball_query_picks_ties_supported.restype = _ci


def fps_two_level(xyz: torch.Tensor, m1: int, m2: int, query=None, knn=None, query_counts: bool = False):
    """The reference's two chained samplings  i1 = FPS(xyz, m1); l1 = xyz[i1]; i2 = FPS(l1, m2)  (backbones.py:98-104)
    -> (i1 (B,m1), l1 (B,m1,3), i2 (B,m2)) int32/float32, bit-identical to running both.  The second pass is
    skipped per cloud when level 1 had no tied arg-max among its first m2 picks (include/pn2_ext.h).
    query=(radius, nsample): level 1's ball query is done by the launch that produces l1 (ball_query_picks) and its
    index tensor (B,m1,nsample) is returned as a fourth value; with query_counts=True its hit counts (B,m1) int32 (min(hits,
    nsample), 1 where nothing was hit; written by the same launch) follow as a fifth.
    knn=(points (B,nq,3), k, k2): also knn_indices(k, points, xyz, k2) -- appended to the result as one more value, the pair
    (idx (B,nq,k), idx2 (B,nq,k2) | None) -- in the launch of the first sampling level when the kernels cover the sizes
    (include/pn2_ext.h: pn2x_fps_radii_knn), as its own launch otherwise."""
    from . import pointnet2_utils as ops
    B, N, _ = xyz.shape
    if not 1 <= m2 <= m1:
        raise ValueError("fps_two_level: need 1 <= m2 <= m1")
    xyz = xyz.contiguous()

    def knn_alone():
        r = knn_indices(knn[1], knn[0], xyz, k2=knn[2])
        return r if knn[2] else (r, None)
    if m2 > 1024 or N > 16384:  # beyond the shortcut's kernels: two plain passes
        i1 = ops.furthest_point_sample(xyz, m1)
        l1 = gather_rows(xyz, i1)
        i2 = ops.furthest_point_sample(l1, m2)
        if query is not None and query_counts:
            raise ValueError("fps_two_level: query_counts needs m2 <= 1024 and N <= 16384")
        res = (i1, l1, i2) if query is None else (i1, l1, i2, ops.ball_query(query[0], query[1], xyz, l1))
        return res if knn is None else res + (knn_alone(),)
    px = _native._ptr(xyz, "xyz", torch.float32, B * N * 3)
    nf = _lib.pn2x_fps_prefix_flags(N)
    i1 = torch.empty((B, m1), dtype=torch.int32, device=xyz.device)
    radii = torch.empty((B, m1), dtype=torch.float32, device=xyz.device)
    flags = torch.empty((B, nf), dtype=torch.int32, device=xyz.device)
    i2 = torch.empty((B, m2), dtype=torch.int32, device=xyz.device)
    if query_counts and query is None:
        raise ValueError("fps_two_level: query_counts without query")
    cnt1 = torch.empty((B, m1), dtype=torch.int32, device=xyz.device) if query_counts else None
    with torch.cuda.device(xyz.device):
        st = _native._stream(xyz)
        lists = None
        if knn is not None and FPS_KNN_COLAUNCH and _lib.pn2x_fps_radii_knn_supported(N, knn[0].shape[1], knn[1]):
            pts, k, k2 = knn
            nq = pts.shape[1]
            gi = torch.empty((B, nq, k), dtype=torch.int32, device=xyz.device)
            gi2 = torch.empty((B, nq, k2), dtype=torch.int32, device=xyz.device) if k2 else None
            _native._check(_native._call(_lib.pn2x_fps_radii_knn, "fps_knn_kernel", None, B, N, m1, px, i1.data_ptr(), radii.data_ptr(),
                                         nq, k, k2, _native._ptr(pts, "knn points", torch.float32, B * nq * 3), gi.data_ptr(),
                                         None if gi2 is None else gi2.data_ptr(), st), "fps_two_level/1+knn")
            lists = (gi, gi2)
        else:
            _native._check(_native._call(_lib.pn2x_furthest_point_sampling_radii, "fps_kernel", None, B, N, m1, px, i1.data_ptr(),
                                         radii.data_ptr(), st), "fps_two_level/1")
        if query is not None and BALL_TIE_COLAUNCH and _lib.pn2x_ball_query_picks_ties_supported(B, N, m1, m2):
            # level 1's ball query and the tie check of the sampling run both start from the picks: one launch
            idx1 = torch.empty((B, m1, query[1]), dtype=torch.int32, device=xyz.device)
            l1 = torch.empty((B, m1, 3), dtype=torch.float32, device=xyz.device)
            if query_counts:
                _native._check(_native._call(_lib.pn2x_ball_query_picks_ties_counts, "ball_tie_kernel", None, B, N, m1, float(query[0]), query[1],
                                             px, i1.data_ptr(), l1.data_ptr(), idx1.data_ptr(), None, 0, m2, radii.data_ptr(),
                                             flags.data_ptr(), cnt1.data_ptr(), st), "fps_two_level/query+ties")
            else:
                _native._check(_native._call(_lib.pn2x_ball_query_picks_ties, "ball_tie_kernel", None, B, N, m1, float(query[0]), query[1], px,
                                             i1.data_ptr(), l1.data_ptr(), idx1.data_ptr(), None, 0, m2, radii.data_ptr(), flags.data_ptr(), st),
                               "fps_two_level/query+ties")
        else:
            if query is None:
                l1 = gather_rows(xyz, i1)
            elif query_counts:
                idx1, l1, cnt1 = ball_query_picks(query[0], query[1], xyz, i1, counts=True)
            else:
                idx1, l1 = ball_query_picks(query[0], query[1], xyz, i1)
            _native._check(_lib.pn2x_fps_prefix_ties(B, N, m1, m2, px, i1.data_ptr(), radii.data_ptr(), flags.data_ptr(), st), "fps_two_level/ties")
        _native._check(_native._call(_lib.pn2x_furthest_point_sampling_prefix, "fps_prefix_kernel", None, B, m1, m2, l1.data_ptr(),
                                     flags.data_ptr(), nf, i2.data_ptr(), st), "fps_two_level/2")
    res = (i1, l1, i2) if query is None else (i1, l1, i2, idx1)
    if query_counts:
        res = res + (cnt1,)
    if knn is None:
        return res
    return res + (lists if lists is not None else knn_alone(),)


_lib.pn2x_hand_losses.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_hand_losses.restype = _ci
_lib.pn2x_hand_losses_backward.argtypes = [_ci, _ci, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_hand_losses_backward.restype = _ci
HAND_LOSS_NAMES = ("hand_pred_kp_loss", "hand_pred_r_loss", "hand_pred_t_loss", "hand_pred_kp_diff", "hand_init_kp_diff",
                   "hand_init_r_diff", "hand_init_t_diff", "hand_pred_r_diff", "hand_pred_t_diff")


class HandLosses(torch.autograd.Function):
    """The nine entries of HandTrackNet.compute_loss's dictionary (include/pn2_ext.h: pn2x_hand_losses) as a (9,) tensor;
    differentiable with respect to pred_hf through the first three (keypoint L1, rotation L1 and translation L1 of the palm
    fit -- the closed-form Kabsch gradient), the rest are metrics."""

    @staticmethod
    def forward(ctx, pred_hf, init_hf, gt_kp, pred_kp, R, t, scale, palm, weights=None):
        # weights (9,) on the device: also returns sum_i weights[i] out[i] as a second (0-dim) output (the trainer's weighted
        # total, trainer.py:157-165) -- no multiply / sum launches, and its gradient goes straight into the backward kernel
        f32 = torch.float32
        B = pred_hf.shape[0]
        ctx.set_materialize_grads(False)
        pred_hf = pred_hf.contiguous()
        palm = palm.contiguous().float()
        if palm.dim() == 2:
            palm = palm.unsqueeze(0)
        args = [x.detach().contiguous().float() for x in (init_hf, gt_kp, pred_kp, R, t)]
        out = torch.empty(10, dtype=f32, device=pred_hf.device)
        saved = torch.empty((B, 87), dtype=f32, device=pred_hf.device)
        wptr = None if weights is None else _native._ptr(weights, "weights", f32, 9)
        with torch.cuda.device(pred_hf.device):
            _native._check(_lib.pn2x_hand_losses(B, palm.shape[0], _native._ptr(pred_hf, "pred_hf", f32, B * 63), _native._ptr(args[0], "init_hf", f32, B * 63),
                                                  _native._ptr(args[1], "gt_kp", f32, B * 63), _native._ptr(args[2], "pred_kp", f32, B * 63),
                                                  _native._ptr(args[3], "R", f32, B * 9), _native._ptr(args[4], "t", f32, B * 3), float(scale),
                                                  _native._ptr(palm, "palm", f32, palm.shape[0] * 18), out.data_ptr(), saved.data_ptr(), wptr,
                                                  _native._stream(pred_hf)), "hand_losses")
        ctx.save_for_backward(pred_hf, palm, saved, *([weights] if weights is not None else []))
        ctx.scale = float(scale)
        ctx.set_materialize_grads(False)  # (backward handles None: no zero-fill launch for the output nobody differentiates)
        if weights is None:
            return out[:9]
        return out[:9], out[9]

    @staticmethod
    def backward(ctx, grad, grad_total=None):
        pred_hf, palm, saved = ctx.saved_tensors[:3]
        weights = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        B = pred_hf.shape[0]
        if grad is None and grad_total is None:
            return (None,) * 9
        g3 = None if grad is None else grad[:3].contiguous().float()
        gt = None if grad_total is None else grad_total.contiguous().float()
        d = torch.empty_like(pred_hf)
        with torch.cuda.device(pred_hf.device):
            _native._check(_lib.pn2x_hand_losses_backward(B, palm.shape[0], pred_hf.data_ptr(), ctx.scale, palm.data_ptr(), saved.data_ptr(),
                                                           None if g3 is None else g3.data_ptr(), None if gt is None else gt.data_ptr(),
                                                           None if weights is None else weights.data_ptr(), d.data_ptr(),
                                                           _native._stream(pred_hf)), "hand_losses_backward")
        return d, None, None, None, None, None, None, None, None


_lib.pn2x_copy_multi_max.argtypes = []
_lib.pn2x_copy_multi_max.restype = _ci
_lib.pn2x_copy_multi.argtypes = [_ci, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_long), _vp]
_lib.pn2x_copy_multi.restype = _ci


def copy_multi(dsts, srcs) -> None:
    """dsts[i].copy_(srcs[i]) for same-shaped, same-dtype contiguous tensors on ONE GPU as one launch (pn2x_copy_multi)."""
    n = len(dsts)
    if n == 0:
        return
    cap = int(_lib.pn2x_copy_multi_max())
    dev = dsts[0].device
    for d, s_ in zip(dsts, srcs):
        if (not d.is_cuda or d.device != dev or s_.device != dev or d.dtype != s_.dtype or d.shape != s_.shape
                or not d.is_contiguous() or not s_.is_contiguous()):
            raise ValueError("copy_multi: same-shaped contiguous tensors of one dtype on one GPU")
    with torch.cuda.device(dev):
        for i0 in range(0, n, cap):
            k = min(cap, n - i0)
            D, S, Bn = (_vp * k)(), (_vp * k)(), (ctypes.c_long * k)()
            for j in range(k):
                D[j], S[j], Bn[j] = dsts[i0 + j].data_ptr(), srcs[i0 + j].data_ptr(), dsts[i0 + j].numel() * dsts[i0 + j].element_size()
            _native._check(_lib.pn2x_copy_multi(k, D, S, Bn, _native._stream(dsts[0])), "copy_multi")


# ---- the per-point chain fp1 -> conv1 -> q layer-1 over the rows the kNN lists name (include/pn2_ext.h: pn2x_row_chain) ----
_lib.pn2x_row_lists.argtypes = [_ci] * 5 + [_vp] * 5
_lib.pn2x_row_lists.restype = _ci
_lib.pn2x_row_chain_supported.argtypes = [_ci] * 4
_lib.pn2x_row_chain_supported.restype = _ci
_lib.pn2x_row_chain.argtypes = [_ci, _ci, _vp, _ci, _vp, _vp] + [_vp] * 7 + [_vp, _ci, _ci, _vp]
_lib.pn2x_row_chain.restype = _ci
_lib.pn2x_row_chain3_supported.argtypes = [_ci] * 3
_lib.pn2x_row_chain3_supported.restype = _ci
_lib.pn2x_row_chain3.argtypes = [_ci, _ci, _vp, _ci, _vp, _vp] + [_vp] * 5 + [_vp, _ci, _ci, _vp]
_lib.pn2x_row_chain3.restype = _ci
ROW_CHAIN_MAX_B = 1024


def row_lists(gi: torch.Tensor, gi_small, n: int):
    """Per-cloud lists of the distinct points the kNN index lists name: gi (B,J,KL) int32, gi_small (B,J,KS) int32 (or None: every
    row of gi counts as small).  -> list (B,n) int32 (rows named by gi_small ascending, then the rest of
    gi's rows ascending; entries past the count are not written) and counts (B,2) int32 [small, all]."""
    if gi.dim() != 3 or gi.dtype != torch.int32 or not gi.is_cuda:
        raise TypeError("row_lists: gi must be a (B,J,K) int32 GPU tensor")
    gi = gi.contiguous()
    B, J, KL = gi.shape
    if gi_small is not None:
        if gi_small.dim() != 3 or gi_small.shape[:2] != (B, J) or gi_small.dtype != torch.int32 or gi_small.device != gi.device:
            raise ValueError("row_lists: gi_small must be (B,J,K2) int32 on gi's device")
        gi_small = gi_small.contiguous()
    KS = gi_small.shape[2] if gi_small is not None else KL
    lst = torch.empty((B, n), dtype=torch.int32, device=gi.device)
    counts = torch.empty((B, 2), dtype=torch.int32, device=gi.device)
    with torch.cuda.device(gi.device):
        _native._check(_native._call(_lib.pn2x_row_lists, "row_lists_kernel", None, B, n, J, KL, KS, gi.data_ptr(),
                                     None if gi_small is None else gi_small.data_ptr(), lst.data_ptr(), counts.data_ptr(),
                                     _native._stream(gi)), "row_lists")
    return lst, counts


def row_chain_supported(c_in: int, c_h: int, c_conv: int, c_q: int) -> bool:
    return bool(_lib.pn2x_row_chain_supported(c_in, c_h, c_conv, c_q))


def row_chain_pack(W: torch.Tensor) -> torch.Tensor:
    """(n_out, k) weights -> the kernel's operand layout: k zero-padded to a multiple of 16, then [n-tile][k-group][lane][4] with
    lane = 16 * (k quad inside the group) + (row inside the n-tile) (include/pn2_ext.h: pn2x_row_chain)."""
    n_out, k = W.shape
    kp = (k + 15) // 16 * 16
    Wp = torch.zeros((n_out, kp), dtype=torch.float32, device=W.device)
    Wp[:, :k] = W
    return Wp.view(n_out // 16, 16, kp // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


def row_chain(x: torch.Tensor, lst: torch.Tensor, counts: torch.Tensor, wa, ba, wb, bb, wc, bc, wq, out: torch.Tensor = None,
              grid: int = 0) -> torch.Tensor:
    """out[b, p, :512] for every listed point p of cloud b (pn2x_row_chain): x (B,N,>=132) [interp | xyz | pad] rows (last dim
    contiguous, row stride a multiple of 4), lst / counts from row_lists, the four weight matrices packed by row_chain_pack
    (wa: fp1 layer 1 as (128, 131) [features | xyz]; wb (128,128); wc (384,128); wq (512,384)) and the biases of the first three.
    Rows / columns no list asks for are left as they are in `out` (B,N,>=512).
    wa = ba = None: x (B,N,>=128) already holds h1 = relu(fp1 layer 1) and the chain starts at its second layer (pn2x_row_chain3)."""
    if x.dim() != 3 or not x.is_cuda or x.dtype != torch.float32 or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        raise TypeError("row_chain: x must be a (B,N,C) float32 GPU tensor with contiguous rows")
    if (wa is None) != (ba is None):
        raise ValueError("row_chain: wa and ba come together")
    if wa is None and x.shape[2] < 128:
        raise ValueError("row_chain: without wa / ba the rows of x hold h1, 128 floats")
    B, N, _ = x.shape
    f32 = torch.float32
    if out is None:
        out = torch.empty((B, N, 512), dtype=f32, device=x.device)
    if out.shape[:2] != (B, N) or out.shape[2] < 512 or out.stride(2) != 1 or out.stride(0) != N * out.stride(1) or out.dtype != f32:
        raise ValueError("row_chain: out must be (B,N,>=512) float32 with contiguous rows")
    if lst.shape != (B, N) or counts.shape != (B, 2) or lst.dtype != torch.int32 or counts.dtype != torch.int32:
        raise ValueError("row_chain: list (B,N) / counts (B,2) int32 from row_lists")
    if wa is None:
        with torch.cuda.device(x.device):
            _native._check(_native._call(_lib.pn2x_row_chain3, "row_chain3_kernel", None, B, N, x.data_ptr(), x.stride(1), lst.data_ptr(),
                                         counts.data_ptr(), _native._ptr(wb, "wb", f32, 128 * 128), _native._ptr(bb, "bb", f32, 128),
                                         _native._ptr(wc, "wc", f32, 384 * 128), _native._ptr(bc, "bc", f32, 384),
                                         _native._ptr(wq, "wq", f32, 512 * 384), out.data_ptr(), out.stride(1), int(grid),
                                         _native._stream(x)), "row_chain")
        return out
    with torch.cuda.device(x.device):
        _native._check(_native._call(_lib.pn2x_row_chain, "row_chain_kernel", None, B, N, x.data_ptr(), x.stride(1), lst.data_ptr(),
                                     counts.data_ptr(), _native._ptr(wa, "wa", f32, 128 * 144), _native._ptr(ba, "ba", f32, 128),
                                     _native._ptr(wb, "wb", f32, 128 * 128), _native._ptr(bb, "bb", f32, 128),
                                     _native._ptr(wc, "wc", f32, 384 * 128), _native._ptr(bc, "bc", f32, 384),
                                     _native._ptr(wq, "wq", f32, 512 * 384), out.data_ptr(), out.stride(1), int(grid),
                                     _native._stream(x)), "row_chain")
    return out


def row_chain3_supported(c_h: int, c_conv: int, c_q: int) -> bool:
    return bool(_lib.pn2x_row_chain3_supported(c_h, c_conv, c_q))


def row_chain3(h1: torch.Tensor, lst: torch.Tensor, counts: torch.Tensor, wb, bb, wc, bc, wq, out: torch.Tensor = None,
               grid: int = 0) -> torch.Tensor:
    """row_chain from its second layer on (pn2x_row_chain3): h1 (B,N,>=128) rows that already hold relu(fp1 layer 1); lists, packed
    weights, biases and `out` as in row_chain, which this is without its first layer."""
    return row_chain(h1, lst, counts, None, None, wb, bb, wc, bc, wq, out=out, grid=grid)


# ---- sa3 and fp3 as row-tiled layer chains on the large-batch route (include/pn2_ext.h: pn2x_sa3_chain, pn2x_fp3_chain) ----
_lib.pn2x_sa3_chain_supported.argtypes = [_ci] * 5
_lib.pn2x_sa3_chain_supported.restype = _ci
_lib.pn2x_sa3_chain.argtypes = [_ci, _ci, _vp, _ci] + [_vp] * 7 + [_vp]
_lib.pn2x_sa3_chain.restype = _ci
_lib.pn2x_fp3_chain_supported.argtypes = [_ci] * 5
_lib.pn2x_fp3_chain_supported.restype = _ci
_lib.pn2x_fp3_chain.argtypes = [_ci, _ci, _vp, _ci] + [_vp] * 6 + [_vp, _ci, _vp]
_lib.pn2x_fp3_chain.restype = _ci
MID_CHAIN_TILE = 32  # rows per tile of pn2x_sa3_chain / pn2x_fp3_chain; each tile writes one partial maximum row


def sa3_chain_supported(s: int, c_in: int, c1: int, c2: int, c3: int) -> bool:
    return bool(_lib.pn2x_sa3_chain_supported(s, c_in, c1, c2, c3))


def fp3_chain_supported(s: int, c_l2: int, c_l3: int, c1: int, c2: int) -> bool:
    return bool(_lib.pn2x_fp3_chain_supported(s, c_l2, c_l3, c1, c2))


def _chain_rows(x: torch.Tensor, name: str, min_cols: int):
    if x.dim() != 3 or not x.is_cuda or x.dtype != torch.float32 or x.stride(2) != 1 or x.shape[2] < min_cols or \
            x.stride(0) != x.shape[1] * x.stride(1):
        raise TypeError(f"{name}: expected a (B,S,>={min_cols}) float32 GPU tensor with contiguous rows, got {tuple(x.shape)} {x.stride()}")
    return x.shape[0], x.shape[1]


def sa3_chain(x: torch.Tensor, w1, b1, w2, b2, w3, b3, part: torch.Tensor = None) -> torch.Tensor:
    """Per-tile maxima of sa3 (pn2x_sa3_chain): x (B,S,>=132) [l2_feat | l2_xyz | pad] rows, weights packed by row_chain_pack
    (w1: (128, 131) [features | xyz]; w2 (128,128); w3 (512,128)) with their biases.  -> part (B, S/32, 512); the max over
    its last-but-one axis is sa3's output."""
    B, S = _chain_rows(x, "sa3_chain", 132)
    T = MID_CHAIN_TILE
    if S % T:
        raise ValueError(f"sa3_chain: S = {S} is not a multiple of {T}")
    f32 = torch.float32
    if part is None:
        part = torch.empty((B, S // T, 512), dtype=f32, device=x.device)
    if tuple(part.shape) != (B, S // T, 512) or not part.is_contiguous() or part.dtype != f32:
        raise ValueError(f"sa3_chain: part must be a contiguous (B, S/{T}, 512) float32 tensor")
    with torch.cuda.device(x.device):
        _native._check(_native._call(_lib.pn2x_sa3_chain, "sa3_chain_kernel", None, B, S, x.data_ptr(), x.stride(1),
                                     _native._ptr(w1, "w1", f32, 128 * 144), _native._ptr(b1, "b1", f32, 128),
                                     _native._ptr(w2, "w2", f32, 128 * 128), _native._ptr(b2, "b2", f32, 128),
                                     _native._ptr(w3, "w3", f32, 512 * 128), _native._ptr(b3, "b3", f32, 512), part.data_ptr(),
                                     _native._stream(x)), "sa3_chain")
    return part


def fp3_chain(x: torch.Tensor, part: torch.Tensor, wgt, bg, wa, wf, bf, out: torch.Tensor = None) -> torch.Tensor:
    """fp3 over the level-2 rows (pn2x_fp3_chain): out[b, r] = relu(Wf relu(Wa x[b, r, :128] + Wg l3[b] + bg) + bf) with
    l3[b] = part[b].max(0) (part from sa3_chain).  x (B,S,>=128) rows with contiguous columns; wgt = Wg^T (512, 256)
    contiguous; wa (256, 128) and wf (256, 256) packed by row_chain_pack.  out (B,S,>=256)."""
    B, S = _chain_rows(x, "fp3_chain", 128)
    T = MID_CHAIN_TILE
    if S % T:
        raise ValueError(f"fp3_chain: S = {S} is not a multiple of {T}")
    f32 = torch.float32
    if out is None:
        out = torch.empty((B, S, 256), dtype=f32, device=x.device)
    _chain_rows(out, "fp3_chain: out", 256)
    if out.shape[:2] != (B, S):
        raise ValueError("fp3_chain: out must be (B,S,>=256)")
    if tuple(part.shape) != (B, S // T, 512) or not part.is_contiguous() or part.dtype != f32:
        raise ValueError(f"fp3_chain: part must be a contiguous (B, S/{T}, 512) float32 tensor")
    if tuple(wgt.shape) != (512, 256):
        raise ValueError("fp3_chain: wgt must be Wg^T, (512, 256)")
    with torch.cuda.device(x.device):
        _native._check(_native._call(_lib.pn2x_fp3_chain, "fp3_chain_kernel", None, B, S, x.data_ptr(), x.stride(1), part.data_ptr(),
                                     _native._ptr(wgt, "wgt", f32, 512 * 256), _native._ptr(bg, "bg", f32, 256),
                                     _native._ptr(wa, "wa", f32, 256 * 128), _native._ptr(wf, "wf", f32, 256 * 256),
                                     _native._ptr(bf, "bf", f32, 256), out.data_ptr(), out.stride(1), _native._stream(x)), "fp3_chain")
    return out


# ---- hand shape-code search in one launch (include/pn2_ext.h: pn2x_hand_shape_opt) ---------------------------------------
_lib.pn2x_hand_shape_opt_supported.argtypes = [_ci] * 3
_lib.pn2x_hand_shape_opt_supported.restype = _ci
_lib.pn2x_hand_shape_opt.argtypes = [_ci] * 4 + [_vp] * 5 + [ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]
_lib.pn2x_hand_shape_opt.restype = _ci


def hand_shape_opt_supported(p: int, d: int, t: int) -> bool:
    return bool(_lib.pn2x_hand_shape_opt_supported(p, d, t))


def hand_shape_opt(k0: torch.Tensor, k: torch.Tensor, pre: torch.Tensor, targets: torch.Tensor, initial_scale: torch.Tensor,
                   scaling_coefficient2: float, beta: float, iterations: int, out: torch.Tensor = None, trace: bool = False):
    """The whole shape-code search of gf_optimize_hand_shape.optimize in one launch (pn2x_hand_shape_opt).  k0 (21,3) and
    k (D,21,3): keypoints affine in the shape code (HandModel.shape_keypoint_basis); pre (P,D) pre-sampled particles, row 0
    zero; targets (T,15) bone lengths; initial_scale (D).  -> (shape code (D,), trace (iterations, 3 + D) or None).  With iterations = 0 the code is zero, in a
    caller's `out` too."""
    P, D = pre.shape
    T = targets.shape[0]
    f32 = torch.float32
    if tuple(k.shape) != (D, 21, 3) or tuple(k0.shape) != (21, 3) or targets.dim() != 2 or targets.shape[1] != 15:
        raise ValueError(f"hand_shape_opt: k0 {tuple(k0.shape)}, k {tuple(k.shape)}, pre {tuple(pre.shape)}, targets "
                         f"{tuple(targets.shape)} do not fit together")
    if not hand_shape_opt_supported(P, D, T):
        raise ValueError(f"hand_shape_opt: P = {P}, D = {D}, T = {T} outside 1..8192, 1..16, 1..1024")
    if out is None:
        out = (torch.empty if iterations > 0 else torch.zeros)(D, dtype=f32, device=pre.device)
    tr = torch.empty((iterations, 3 + D), dtype=f32, device=pre.device) if trace else None
    with torch.cuda.device(pre.device):
        _native._check(_native._call(_lib.pn2x_hand_shape_opt, "hand_shape_kernel", None, P, D, T, int(iterations),
                                     _native._ptr(k0, "k0", f32, 63), _native._ptr(k, "k", f32, D * 63),
                                     _native._ptr(pre, "pre", f32, P * D), _native._ptr(targets, "targets", f32, T * 15),
                                     _native._ptr(initial_scale, "initial_scale", f32, D), float(scaling_coefficient2), float(beta),
                                     _native._ptr(out, "out", f32, D), None if tr is None else tr.data_ptr(),
                                     _native._stream(pre)), "hand_shape_opt")
        if iterations == 0:  # no launch: the C entry leaves `out` alone, and the code after no iterations is the zero code
            out.zero_()
    return out, tr


# ---- IKNet eval forward for up to 16 rows (include/pn2_ext.h: pn2x_iknet_forward) -------------------------------------------
_lib.pn2x_iknet_supported.argtypes = [_ci] * 5
_lib.pn2x_iknet_supported.restype = _ci
_lib.pn2x_iknet_work_floats.argtypes = []
_lib.pn2x_iknet_work_floats.restype = _cl
_lib.pn2x_iknet_forward.argtypes = [_ci, _ci] + [_vp] * 14
_lib.pn2x_iknet_forward.restype = _ci
IKNET_MAX_ROWS = 16


def iknet_supported(m: int, k_in: int = 126, hidden: int = 1024, layers: int = 6, n_out: int = 60) -> bool:
    return bool(_lib.pn2x_iknet_supported(m, k_in, hidden, layers, n_out))


def iknet_forward(kp: torch.Tensor, R: torch.Tensor, t: torch.Tensor, w1, b1, wh, bh, wo, bo, camera: bool = False):
    """The eval-mode IKNet forward (pn2x_iknet_forward): kp (M,21,3), R (M,3,3), t (M,3,1) of the palm fit; BatchNorm-folded
    weights w1 (1024,128) (columns 126, 127 zero), b1 (1024), wh (5,1024,1024), bh (5,1024), wo (60,1024), bo (60).
    -> (raw_quat (M,60), theta (M,45), kp_hf (M,3,21)).  camera: the 'camera' frame (kp * 5; R, t unused)."""
    M = kp.shape[0]
    if not iknet_supported(M):
        raise ValueError(f"iknet_forward: {M} rows outside 1..{IKNET_MAX_ROWS}")
    f32 = torch.float32
    dev = kp.device
    work = torch.empty(int(_lib.pn2x_iknet_work_floats()), dtype=f32, device=dev)
    raw = torch.empty((M, 60), dtype=f32, device=dev)
    theta = torch.empty((M, 45), dtype=f32, device=dev)
    kp_hf = torch.empty((M, 3, 21), dtype=f32, device=dev)
    with torch.cuda.device(dev):
        _native._check(_native._call(_lib.pn2x_iknet_forward, "iknet_forward", None, M, 1 if camera else 0,
                                     _native._ptr(kp, "kp", f32, M * 63), _native._ptr(R, "R", f32, M * 9),
                                     _native._ptr(t, "t", f32, M * 3), _native._ptr(w1, "w1", f32, 1024 * 128),
                                     _native._ptr(b1, "b1", f32, 1024), _native._ptr(wh, "wh", f32, 5 * 1024 * 1024),
                                     _native._ptr(bh, "bh", f32, 5 * 1024), _native._ptr(wo, "wo", f32, 60 * 1024),
                                     _native._ptr(bo, "bo", f32, 60), work.data_ptr(), kp_hf.data_ptr(), raw.data_ptr(),
                                     theta.data_ptr(), _native._stream(kp)), "iknet_forward")
    return raw, theta, kp_hf


# ---- hand-pose particle optimiser on the device (include/pn2_ext.h: pn2x_hand_pose_energy / _opt / _opt_batch) -----------------
_cf, _cd = ctypes.c_float, ctypes.c_double
HAND_POSE_STATE_FLOATS = 90   # curr_r (9), curr_t (3), curr_theta (45), search (16), previous search (16), previous success
HAND_POSE_TRACE_FLOATS = 19   # E[0], mean_E, success, search after the update (16)
HAND_POSE_WEIGHTS = ("sil_loss", "penetrate_sum_loss", "vis_regu_loss", "invis_regu_loss", "temporal_smooth", "attraction_loss")
HAND_POSE_MANO_ENTRIES = ("posedirs", "pose_mean", "kp_vertex", "centre_root")  # skinning_tables()' optional entries


class _HandPoseSetup(ctypes.Structure):
    """pn2x_hand_pose_setup (136 bytes): what the problems of a batch share."""
    _WEIGHTS = ("w_sil", "w_pen", "w_vis", "w_invis", "w_temporal", "w_attr")   # in HAND_POSE_WEIGHTS' order
    _fields_ = ([(n, _vp) for n in ("parents", "pose_block", "skin_pack", "skin_w", "comps", "pre", "posedirs", "pose_mean", "kp_vertex")] +
                [(n, _ci) for n in ("p", "v", "j", "k", "vol_f16", "res", "centre_root", "reserved")] +
                [(n, _cf) for n in ("theta_scale", "voxel_scale") + _WEIGHTS])


class _HandPoseProblem(ctypes.Structure):
    """pn2x_hand_pose_problem (128 bytes): one problem's frame."""
    _fields_ = ([(n, _vp) for n in ("state", "work", "rest_joints", "rest_verts", "pred_kp", "last_kp", "vis_mask", "obj_r", "obj_t",
                                    "vol", "mask", "trace")] +
                [("h", _ci), ("w", _ci), ("fx", _cf), ("fy", _cf), ("cx", _cf), ("cy", _cf), ("active", _ci), ("reserved", _ci)])


_HP_SETUP, _HP_PROBLEM = ctypes.POINTER(_HandPoseSetup), ctypes.POINTER(_HandPoseProblem)
_lib.pn2x_hand_pose_opt_supported.argtypes = [_ci] * 6
_lib.pn2x_hand_pose_opt_supported.restype = _ci
_lib.pn2x_hand_pose_opt_work_floats.argtypes = [_ci]
_lib.pn2x_hand_pose_opt_work_floats.restype = _cl
_lib.pn2x_hand_pose_mano_work_floats.argtypes = [_ci, _ci]
_lib.pn2x_hand_pose_mano_work_floats.restype = _cl
_lib.pn2x_hand_pose_opt_batch_work_floats.argtypes = [_ci, _ci]
_lib.pn2x_hand_pose_opt_batch_work_floats.restype = _cl
_lib.pn2x_hand_pose_energy.argtypes = [_HP_SETUP, _HP_PROBLEM, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_hand_pose_energy.restype = _ci
_lib.pn2x_hand_pose_opt.argtypes = [_HP_SETUP, _HP_PROBLEM, _vp, _ci, _cd, _cd, _vp]
_lib.pn2x_hand_pose_opt.restype = _ci
_lib.pn2x_hand_pose_problems_fill.argtypes = [_vp, _ci, _HP_PROBLEM, _vp]
_lib.pn2x_hand_pose_problems_fill.restype = _ci
_lib.pn2x_hand_pose_opt_batch.argtypes = [_HP_SETUP, _ci, _ci, _vp, _ci, _cd, _cd, _vp]
_lib.pn2x_hand_pose_opt_batch.restype = _ci
_lib.pn2x_hand_pose_mano_batch_work_floats.argtypes = [_ci, _ci, _ci]
_lib.pn2x_hand_pose_mano_batch_work_floats.restype = _cl
_lib.pn2x_hand_pose_mano_opt_batch.argtypes = [_HP_SETUP, _ci, _ci, _vp, _vp, _ci, _cd, _cd, _vp]
_lib.pn2x_hand_pose_mano_opt_batch.restype = _ci


def hand_pose_opt_supported(p: int, v: int, j: int, k: int, d_pose: int = 10, res: int = 151) -> bool:
    return bool(_lib.pn2x_hand_pose_opt_supported(int(p), int(v), int(j), int(k), int(d_pose), int(res)))


def hand_pose_model(tables: dict, device) -> dict:
    """HandModel.skinning_tables() as the device arrays the hand-pose kernels read (built once per model and device):
    int32 parents / pose_block, float32 rest and shape tables, skin_w, comps, and skin_pack = the K joint indices of a vertex
    (5 bits each) with, from bit 20, the tip regions (fingers 0..4 of tips / finger_offsets) the vertex belongs to.
    Tables with a MANO entry (posedirs, pose_mean, kp_vertex, centre_root) set m["mano"] and add what the MANO
    kernels read: posedirs_pack (ceil16(3 V), 136) = posedirs as rows 3 v + coordinate, zero-padded; pose_mean (45); kp_vertex
    (J) int32; centre_root 0 / 1; and in skin_pack bits 25..29 of a keypoint vertex the table joint it is (mano_ok: no vertex
    serves two keypoints).  hand_pose_energy / hand_pose_opt run such a model on the MANO kernels, hand_pose_mano_opt_batch in lockstep;
    hand_pose_opt_batch refuses it."""
    f32, i32 = torch.float32, torch.int32
    idx = tables["skin_idx"].long()
    V, K = idx.shape
    pack = torch.zeros(V, dtype=torch.long)
    for k in range(K):
        pack |= idx[:, k] << (5 * k)
    offs = [int(o) for o in tables["finger_offsets"]]
    for f in range(5):
        pack[tables["tips"][offs[f]:offs[f + 1]].long().unique()] |= 1 << (20 + f)
    m = {"V": V, "K": K, "J": int(tables["parents"].numel()),
         "parents": tables["parents"].to(device, i32).contiguous(), "pose_block": tables["pose_block"].to(device, i32).contiguous(),
         "rest_joints": tables["rest_joints"].to(device, f32).contiguous(), "rest_verts": tables["rest_verts"].to(device, f32).contiguous(),
         "skin_pack": pack.to(device, i32).contiguous(), "skin_w": tables["skin_w"].to(device, f32).contiguous(),
         "comps": tables["comps"].to(device, f32).contiguous(), "fingers_ok": all(offs[f + 1] > offs[f] for f in range(5))}
    m["mano"] = any(k in tables for k in HAND_POSE_MANO_ENTRIES)
    if m["mano"]:
        J = m["J"]
        kpv = tables["kp_vertex"].long() if "kp_vertex" in tables else torch.full((J,), -1, dtype=torch.long)
        owners = [(j, int(v)) for j, v in enumerate(kpv) if int(v) >= 0]
        m["mano_ok"] = len({v for _, v in owners}) == len(owners) and all(0 < j < 32 and v < V for j, v in owners)
        if m["mano_ok"]:
            for j, v in owners:
                pack[v] |= j << 25
            m["skin_pack"] = pack.to(device, i32).contiguous()
        rows = (3 * V + 15) // 16 * 16
        pd = torch.zeros(rows, 136, dtype=f32)
        if "posedirs" in tables:
            pd[:3 * V, :135] = tables["posedirs"].to(f32).reshape(3 * V, 135)
        m["posedirs_pack"] = pd.to(device).contiguous()
        m["pose_mean"] = (tables["pose_mean"].to(f32) if "pose_mean" in tables else torch.zeros(45)).to(device).contiguous()
        m["kp_vertex"] = kpv.to(device, i32).contiguous()
        m["centre_root"] = 1 if tables.get("centre_root", False) else 0
    if "shape_joints" in tables:
        D = tables["shape_joints"].shape[0]
        m["shape_joints"] = tables["shape_joints"].to(device, f32).reshape(D, -1).contiguous()
        m["shape_verts"] = tables["shape_verts"].to(device, f32).reshape(D, -1).contiguous()
    return m


def hand_pose_rest(model: dict, beta: torch.Tensor = None):
    """The frame's shaped rest joints (J,3) and vertices (V,3): rest + beta @ shape_* (device ops, no host read)."""
    if beta is None or "shape_joints" not in model:
        return model["rest_joints"], model["rest_verts"]
    b = beta.to(model["rest_joints"]).reshape(1, -1)
    return ((model["rest_joints"] + (b @ model["shape_joints"]).view(-1, 3)).contiguous(),
            (model["rest_verts"] + (b @ model["shape_verts"]).view(-1, 3)).contiguous())


def _hand_pose_setup(model, pre, theta_scale, volume, voxel_scale, weights, posedirs=None) -> _HandPoseSetup:
    """The pn2x_hand_pose_setup record of a call: the model's tables, the candidates, the volumes' type and the weights; for a
    model with MANO entries also its MANO part (posedirs: a packed table in place of the model's posedirs_pack).  pre / weights
    None: the record of an entry that reads the model alone (hand_interaction_metrics) -- p = 0, no candidates, zero weights."""
    f32, i32 = torch.float32, torch.int32
    mano = bool(model.get("mano", False))
    if mano and not model.get("mano_ok", False):
        raise ValueError("hand_pose_mano: one vertex serves two keypoints (kp_vertex)")
    V, K, J = model["V"], model["K"], model["J"]
    if pre is not None and (pre.dim() != 2 or pre.shape[1] != 16):
        raise ValueError(f"hand_pose: pre {tuple(pre.shape)} is not (P, 16)")
    P = 0 if pre is None else pre.shape[0]
    if volume.dim() != 3 or len(set(volume.shape)) != 1 or volume.dtype not in (torch.float16, f32):
        raise ValueError(f"hand_pose: volume {tuple(volume.shape)} {volume.dtype} is not a cubic fp16 / fp32 volume")
    res = volume.shape[0]
    if not hand_pose_opt_supported(1 if pre is None else P, V, J, K, 10, res):
        raise ValueError(f"hand_pose: P = {P}, V = {V}, J = {J}, K = {K}, res = {res} outside 1..8192, 1..1024, 21, 1..4, odd <= 1024")
    s = _HandPoseSetup(p=P, v=V, j=J, k=K, vol_f16=1 if volume.dtype == torch.float16 else 0, res=res,
                       theta_scale=float(theta_scale), voxel_scale=float(voxel_scale))
    s.parents, s.pose_block = _native._ptr(model["parents"], "parents", i32, J), _native._ptr(model["pose_block"], "pose_block", i32, J)
    s.skin_pack, s.skin_w = _native._ptr(model["skin_pack"], "skin_pack", i32, V), _native._ptr(model["skin_w"], "skin_w", f32, V * K)
    s.comps, s.pre = _native._ptr(model["comps"], "comps", f32, 45 * 45), None if pre is None else _native._ptr(pre, "pre", f32, P * 16)
    for field, key in zip(_HandPoseSetup._WEIGHTS, HAND_POSE_WEIGHTS) if weights is not None else ():
        setattr(s, field, float(weights[key]))
    if mano:
        s.posedirs = _native._ptr(model["posedirs_pack"] if posedirs is None else posedirs, "posedirs", f32, (3 * V + 15) // 16 * 16 * 136)
        s.pose_mean, s.kp_vertex = _native._ptr(model["pose_mean"], "pose_mean", f32, 45), _native._ptr(model["kp_vertex"], "kp_vertex", i32, J)
        s.centre_root = int(model["centre_root"])
    return s


def _hand_pose_frame(model, state, work, trace, rest, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, mask, proj) -> _HandPoseProblem:
    """A pn2x_hand_pose_problem record from the per-frame tensors; state, work and trace (or None) are device addresses."""
    f32, u8 = torch.float32, torch.uint8
    V, J = model["V"], model["J"]
    if mask.dim() != 2:
        raise ValueError(f"hand_pose: mask {tuple(mask.shape)} is not (h, w)")
    h, w = mask.shape
    rest_j, rest_v = rest
    r = _HandPoseProblem(state=state, work=work, trace=trace, h=h, w=w, fx=float(proj["fx"]), fy=float(proj["fy"]), cx=float(proj["cx"]),
                         cy=float(proj["cy"]), active=1)
    r.rest_joints, r.rest_verts = _native._ptr(rest_j, "rest_joints", f32, J * 3), _native._ptr(rest_v, "rest_verts", f32, V * 3)
    r.pred_kp = _native._ptr(pred_kp, "pred_kp", f32, J * 3)
    r.last_kp = None if last_kp is None else _native._ptr(last_kp, "last_kp", f32, J * 3)
    r.vis_mask, r.obj_r, r.obj_t = _native._ptr(vis_mask, "vis_mask", u8, J), _native._ptr(obj_r, "obj_r", f32, 9), _native._ptr(obj_t, "obj_t", f32, 3)
    r.vol, r.mask = _native._ptr(volume, "volume", volume.dtype, volume.shape[0] ** 3), _native._ptr(mask, "mask", u8, h * w)
    return r


def hand_pose_mano_workspace(p: int, v: int, device) -> torch.Tensor:
    """The pose-blend offsets of p candidates of a v-vertex hand (pn2x_hand_pose_mano_work_floats floats), to be reused."""
    return torch.empty(int(_lib.pn2x_hand_pose_mano_work_floats(int(p), int(v))), dtype=torch.float32, device=device)


def _hand_pose_single(setup, model, offsets, state, trace, rest, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, mask, proj):
    """What a single-problem call hands over beside the setup: (frame record, offsets address or None, the tensors they point into).
    A model with MANO entries needs `offsets` (hand_pose_mano_workspace, allocated here when None)."""
    f32, dev = torch.float32, model["rest_joints"].device
    work = torch.empty(int(_lib.pn2x_hand_pose_opt_work_floats(setup.p)), dtype=f32, device=dev)
    off_ptr = None
    if model.get("mano", False):
        if offsets is None:
            offsets = hand_pose_mano_workspace(setup.p, setup.v, dev)
        off_ptr = _native._ptr(offsets, "offsets", f32, int(_lib.pn2x_hand_pose_mano_work_floats(setup.p, setup.v)))
    frame = _hand_pose_frame(model, _native._ptr(state, "state", f32, HAND_POSE_STATE_FLOATS), work.data_ptr(),
                             None if trace is None else trace.data_ptr(), rest, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, mask, proj)
    return frame, off_ptr, (work, offsets)


def hand_pose_energy(model, rest, theta_scale, pre, state, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, voxel_scale, mask, proj,
                     weights, with_geometry: bool = False, *, offsets: torch.Tensor = None, posedirs: torch.Tensor = None):
    """One evaluation of all candidates at `state` (pn2x_hand_pose_energy): model = hand_pose_model(...), rest = hand_pose_rest(...),
    pre (P,16), state (90,), pred_kp / last_kp (21,3) (last_kp may be None), vis_mask (21,) uint8, obj_r (3,3), obj_t (3,), volume
    (res,res,res) fp16 / fp32, mask (h,w) uint8 (non-zero = background), proj {fx, fy, cx, cy}, weights {energy_weight names}.
    A model with MANO entries runs the pose-offset pre-pass and the MANO evaluation.  offsets: hand_pose_mano_workspace(P, V) to
    reuse (else allocated); posedirs: a packed table to use in place of the model's posedirs_pack (tests).
    -> (energy (P,), vertices (P,V,3) or None, keypoints (P,21,3) or None)."""
    setup = _hand_pose_setup(model, pre, theta_scale, volume, voxel_scale, weights, posedirs)
    frame, off_ptr, keep = _hand_pose_single(setup, model, offsets, state, None, rest, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, mask, proj)
    f32, dev, P = torch.float32, pre.device, setup.p
    energy = torch.empty(P, dtype=f32, device=dev)
    verts = torch.empty((P, model["V"], 3), dtype=f32, device=dev) if with_geometry else None
    kp = torch.empty((P, model["J"], 3), dtype=f32, device=dev) if with_geometry else None
    with torch.cuda.device(dev):
        _native._check(_native._call(_lib.pn2x_hand_pose_energy, "hand_pose_energy", None, ctypes.byref(setup), ctypes.byref(frame), off_ptr,
                                     energy.data_ptr(), None if verts is None else verts.data_ptr(),
                                     None if kp is None else kp.data_ptr(), _native._stream(pre)), "hand_pose_energy")
    return energy, verts, kp


def hand_pose_opt(model, rest, theta_scale, pre, state, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, voxel_scale, mask, proj,
                  weights, iterations: int, scaling_coefficient2: float, beta: float, trace: bool = False, *,
                  offsets: torch.Tensor = None):
    """`iterations` x (evaluate, update) of gf_optimize_hand_pose.optimize on the device (pn2x_hand_pose_opt), arguments as
    hand_pose_energy; `state` (90,) is updated in place.  -> trace (iterations, 19) or None."""
    setup = _hand_pose_setup(model, pre, theta_scale, volume, voxel_scale, weights)
    tr = torch.empty((int(iterations), HAND_POSE_TRACE_FLOATS), dtype=torch.float32, device=pre.device) if trace else None
    frame, off_ptr, keep = _hand_pose_single(setup, model, offsets, state, tr, rest, pred_kp, last_kp, vis_mask, obj_r, obj_t, volume, mask, proj)
    with torch.cuda.device(pre.device):
        _native._check(_native._call(_lib.pn2x_hand_pose_opt, "hand_pose_opt", None, ctypes.byref(setup), ctypes.byref(frame), off_ptr,
                                     int(iterations), float(scaling_coefficient2), float(beta), _native._stream(pre)), "hand_pose_opt")
    return tr


# ---- the same loop for S problems per launch (pn2x_hand_pose_opt_batch / pn2x_hand_pose_mano_opt_batch) ------------------------
_HAND_POSE_FRAME_KEYS = ("rest", "theta_scale", "pre", "pred_kp", "last_kp", "vis_mask", "obj_r", "obj_t", "volume", "voxel_scale", "mask",
                         "proj", "weights")
# how hand_pose_opt_batch names the setup fields in which two frames of a batch may differ (the model's tables are one object)
_HAND_POSE_SHARED = {"pre": "pre", "p": "pre", "res": "volume resolution", "vol_f16": "volume dtype", "voxel_scale": "voxel_scale",
                     "theta_scale": "theta_scale", **{w: "weights" for w in _HandPoseSetup._WEIGHTS}}


def hand_pose_opt_batch(model, frames, states, iterations: int, scaling_coefficient2: float, beta: float, trace: bool = False):
    """hand_pose_opt for S independent problems with ONE set of launches (pn2x_hand_pose_opt_batch): every problem's state and
    trace are bit-for-bit what hand_pose_opt gives for it alone.
    frames: a list of S entries, each a dict of hand_pose_opt's per-frame arguments (rest, theta_scale, pre, pred_kp, last_kp,
      vis_mask, obj_r, obj_t, volume, voxel_scale, mask, proj, weights; a 'model' key is ignored) or None for a problem that
      sits out.  rest, pred_kp, last_kp (None or a tensor), vis_mask, the object pose, the volume (problems may share one), the
      mask with its size and proj differ per problem; pre (one tensor), theta_scale, weights and the volumes' resolution, dtype
      and voxel_scale are shared, and a batch that mixes them is refused.  So is a model with MANO entries: it goes to
      hand_pose_mano_opt_batch.
    states (S, 90): updated in place; the rows of problems that sit out are not touched.
    Every tensor is read in place by the launches, and the record table is written by launches that carry the records as
    arguments: no upload, no host read -- a captured call replays on whatever its buffers hold then.
    -> trace (S, iterations, 19) (zero rows for problems that sit out) or None."""
    return _hand_pose_batch(False, model, frames, states, iterations, scaling_coefficient2, beta, trace, None)


def hand_pose_mano_batch_workspace(p: int, v: int, s: int, device) -> torch.Tensor:
    """The pose-blend offsets of s problems of p candidates of a v-vertex hand, one allocation of
    pn2x_hand_pose_mano_batch_work_floats floats (problem q uses slice q), to be reused."""
    return torch.empty(int(_lib.pn2x_hand_pose_mano_batch_work_floats(int(p), int(v), int(s))), dtype=torch.float32, device=device)


def hand_pose_mano_opt_batch(model, frames, states, iterations: int, scaling_coefficient2: float, beta: float, trace: bool = False,
                             offsets: torch.Tensor = None):
    """hand_pose_opt_batch for a model with MANO entries (pn2x_hand_pose_mano_opt_batch): per iteration the pose-offset pre-pass
    over all problems, the MANO evaluation over (candidates, problem) and the shared update -- every problem's state and trace
    are bit-for-bit what hand_pose_opt gives for it alone on the MANO kernels.  frames, states, the shared fields, the record
    table and the result are hand_pose_opt_batch's.  A plain model is refused (it goes to hand_pose_opt_batch), and so is a
    model whose mano_ok is false.
    offsets: hand_pose_mano_batch_workspace(P, V, S) to reuse (else allocated): S times the single route's workspace."""
    return _hand_pose_batch(True, model, frames, states, iterations, scaling_coefficient2, beta, trace, offsets)


def _hand_pose_batch(mano, model, frames, states, iterations, scaling_coefficient2, beta, trace, offsets):
    """The two batched bindings: `mano` names the kind of model the entry takes."""
    f32 = torch.float32
    what = "hand_pose_mano_opt_batch" if mano else "hand_pose_opt_batch"
    S, iterations = len(frames), int(iterations)
    if S < 1:
        raise ValueError(f"{what}: frames is empty")
    if not mano and model.get("mano", False):  # the lockstep kernels would drop the model's MANO terms without a word
        raise ValueError("hand_pose_opt_batch: a model with MANO entries goes to hand_pose_mano_opt_batch (or, one problem at a "
                         "time, to hand_pose_energy / hand_pose_opt)")
    if mano and not model.get("mano", False):
        raise ValueError("hand_pose_mano_opt_batch: a model without MANO entries goes to hand_pose_opt_batch")
    if mano and not model.get("mano_ok", False):
        raise ValueError("hand_pose_mano: one vertex serves two keypoints (kp_vertex)")
    if states.dim() != 2 or tuple(states.shape) != (S, HAND_POSE_STATE_FLOATS):
        raise ValueError(f"{what}: states {tuple(states.shape)} is not ({S}, {HAND_POSE_STATE_FLOATS})")
    _native._ptr(states, "states", f32, S * HAND_POSE_STATE_FLOATS)
    dev = states.device
    tr = torch.zeros((S, iterations, HAND_POSE_TRACE_FLOATS), dtype=f32, device=dev) if trace else None
    sstride, tstride = HAND_POSE_STATE_FLOATS * 4, iterations * HAND_POSE_TRACE_FLOATS * 4
    first, shared, per = None, None, [None] * S
    for q, fr in enumerate(frames):
        if fr is None:
            continue
        missing = [k for k in _HAND_POSE_FRAME_KEYS if k not in fr]
        if missing:
            raise ValueError(f"{what}: frames[{q}] lacks {missing}")
        mine = _hand_pose_setup(model, fr["pre"], fr["theta_scale"], fr["volume"], fr["voxel_scale"], fr["weights"])
        for name, t in (("pre", fr["pre"]), ("pred_kp", fr["pred_kp"]), ("mask", fr["mask"]), ("rest_joints", fr["rest"][0]),
                        ("volume", fr["volume"])):
            if t.device != dev:
                raise RuntimeError(f"{what}: frames[{q}]['{name}'] is on {t.device}, states on {dev}")
        if first is None:
            first, shared = q, mine
        for field, name in _HAND_POSE_SHARED.items() if bytes(mine) != bytes(shared) else ():
            a, b = getattr(shared, field), getattr(mine, field)
            if a != b:
                kind = "one tensor of candidates" if name == "pre" else f"{a} and {b}"
                raise ValueError(f"{what}: frames[{first}] and frames[{q}] differ in {name} ({kind}): a batch "
                                 "shares it; run them in separate batches")
        per[q] = _hand_pose_frame(model, states.data_ptr() + q * sstride, None, None if tr is None else tr.data_ptr() + q * tstride,
                                  fr["rest"], fr["pred_kp"], fr["last_kp"], fr["vis_mask"], fr["obj_r"], fr["obj_t"], fr["volume"],
                                  fr["mask"], fr["proj"])
    if first is None or iterations == 0:
        if iterations < 0:
            raise ValueError(f"{what}: iterations = {iterations}")
        return tr
    need = _lib.pn2x_hand_pose_opt_batch_work_floats(shared.p, S)
    work = torch.empty((S, need // S), dtype=f32, device=dev)
    table = torch.empty((S, ctypes.sizeof(_HandPoseProblem) // 8), dtype=torch.int64, device=dev)
    recs = (_HandPoseProblem * S)()   # (a zeroed record: active == 0, every pointer NULL)
    for q, r in enumerate(per):
        if r is not None:
            r.work = work.data_ptr() + q * work.stride(0) * 4
            recs[q] = r
    n_active = sum(r is not None for r in per)
    tail = (iterations, float(scaling_coefficient2), float(beta))
    if mano:
        if offsets is None:
            offsets = hand_pose_mano_batch_workspace(shared.p, shared.v, S, dev)
        if offsets.device != dev:
            raise RuntimeError(f"{what}: offsets is on {offsets.device}, states on {dev}")
        off_ptr = _native._ptr(offsets, "offsets", f32, int(_lib.pn2x_hand_pose_mano_batch_work_floats(shared.p, shared.v, S)))
        entry, args = _lib.pn2x_hand_pose_mano_opt_batch, (table.data_ptr(), off_ptr) + tail
    else:
        entry, args = _lib.pn2x_hand_pose_opt_batch, (table.data_ptr(),) + tail
    with torch.cuda.device(dev):
        st = _native._stream(states)
        _native._check(_native._call(_lib.pn2x_hand_pose_problems_fill, "hand_pose_problems_fill", None, table.data_ptr(), S, recs, st),
                       "hand_pose_problems_fill")
        _native._check(_native._call(entry, what, None, ctypes.byref(shared), S, n_active, *args, st), what)
    return tr


_lib.pn2x_posed_chamfer_partial_floats.argtypes = [_ci, _ci, _ci]
_lib.pn2x_posed_chamfer_partial_floats.restype = ctypes.c_long
_lib.pn2x_posed_chamfer.argtypes = [_ci, _ci, _ci] + [_vp] * 7 + [ctypes.c_long, _vp, _vp]
_lib.pn2x_posed_chamfer.restype = _ci
_lib.pn2x_obj_pose_metrics.argtypes = [_ci, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp]
_lib.pn2x_obj_pose_metrics.restype = _ci


def posed_chamfer(A: torch.Tensor, B: torch.Tensor, Ra: torch.Tensor, ta: torch.Tensor, Rb: torch.Tensor, tb: torch.Tensor) -> torch.Tensor:
    """Per-frame chamfer distance of two posed clouds (pn2x_posed_chamfer): A (N,3), B (M,3) in their model frames, Ra / Rb
    (T,3,3), ta / tb (T,3) -> (T,) with out[f] = mean_i min_j |Ra_f a_i + ta_f - (Rb_f b_j + tb_f)| + mean_j min_i |...|.
    Two launches for the whole sequence, no host sync (capturable)."""
    f32 = torch.float32
    N, M, T = A.shape[0], B.shape[0], Ra.shape[0]
    if T > 0 and (N == 0 or M == 0):
        raise ValueError(f"posed_chamfer: empty cloud (N = {N}, M = {M})")
    args = [_native._ptr(A, "A", f32, N * 3), _native._ptr(B, "B", f32, M * 3), _native._ptr(Ra, "Ra", f32, T * 9),
            _native._ptr(ta, "ta", f32, T * 3), _native._ptr(Rb, "Rb", f32, T * 9), _native._ptr(tb, "tb", f32, T * 3)]
    need = int(_lib.pn2x_posed_chamfer_partial_floats(N, M, T))
    partial = torch.empty(max(need, 1), dtype=f32, device=A.device)
    out = torch.empty(T, dtype=f32, device=A.device)
    with torch.cuda.device(A.device):
        _native._check(_native._call(_lib.pn2x_posed_chamfer, "posed_chamfer", None, N, M, T, *args, partial.data_ptr(), need,
                                     out.data_ptr(), _native._stream(A)), "posed_chamfer")
    return out


def obj_pose_metrics(gt_R: torch.Tensor, gt_t: torch.Tensor, pred_R: torch.Tensor, pred_t: torch.Tensor, axis: int,
                     up_and_down_sym: bool) -> torch.Tensor:
    """eval_part_full's per-frame terms (pn2x_obj_pose_metrics): rotations (T,3,3), translations (T,3) ->
    (T,4) = [tdiff (m), rdiff (degrees), 5deg5cm, 10deg10cm].  One launch, no host sync."""
    f32 = torch.float32
    T = gt_R.shape[0]
    out = torch.empty((T, 4), dtype=f32, device=gt_R.device)
    with torch.cuda.device(gt_R.device):
        _native._check(_native._call(_lib.pn2x_obj_pose_metrics, "obj_pose_metrics", None, T, _native._ptr(gt_R, "gt_R", f32, T * 9),
                                     _native._ptr(gt_t, "gt_t", f32, T * 3), _native._ptr(pred_R, "pred_R", f32, T * 9),
                                     _native._ptr(pred_t, "pred_t", f32, T * 3), int(axis), 1 if up_and_down_sym else 0,
                                     out.data_ptr(), _native._stream(gt_R)), "obj_pose_metrics")
    return out


_lib.pn2x_hand_seq_metrics.argtypes = [_ci] * 4 + [_vp] * 18
_lib.pn2x_hand_seq_metrics.restype = _ci
HAND_SEQ_COLS = 12


def hand_seq_metrics(pred_hf: torch.Tensor, init_hf: torch.Tensor, gt_kp: torch.Tensor, pred_kp: torch.Tensor, Rc: torch.Tensor,
                     tc: torch.Tensor, scale: torch.Tensor, offsets, palm=None, pose_R=None, pose_t=None, gt_R=None, gt_t=None,
                     theta=None, theta_gt=None, seq_off=None):
    """The tracked-hand evaluation of F frames in S sequences (pn2x_hand_seq_metrics): pred_hf / init_hf (F,3,21), gt_kp / pred_kp
    (F,21,3), Rc (F,3,3), tc (F,3), scale (F,) -> rows (F,12), seq (S,12), mask (bit c: column c is valid).  offsets: the HOST
    list of S + 1 frame offsets (non-decreasing, offsets[0] = 0, offsets[-1] = F); seq_off: the same offsets as an int32 device
    tensor when the caller already holds one (a captured graph must: building it is a host-to-device copy), else it is built
    here.  palm (S,6,3) selects the Kabsch mode, pose_R (F,3,3) / pose_t (F,3) with gt_R / gt_t the pose mode; gt_R / gt_t
    (F,3,3) / (F,3) are optional in the Kabsch mode, theta / theta_gt (F,45) in both.  Two launches, no host sync."""
    f32 = torch.float32
    offsets = [int(o) for o in offsets]
    F, S = pred_hf.shape[0], len(offsets) - 1
    if S < 0 or offsets[0] != 0 or offsets[-1] != F or any(b < a for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"hand_seq_metrics: offsets must be non-decreasing from 0 to F = {F}, got {offsets}")
    if (palm is None) == (pose_R is None):
        raise ValueError("hand_seq_metrics: give either the palm templates (Kabsch mode) or the global pose (pose mode)")
    mode = 0 if palm is not None else 1
    if (gt_R is None) != (gt_t is None) or (theta is None) != (theta_gt is None) or (mode == 1 and (pose_t is None or gt_R is None)):
        raise ValueError("hand_seq_metrics: gt_R / gt_t and theta / theta_gt come in pairs; the pose mode needs pose_t, gt_R and gt_t")
    if pred_hf.dim() != 3 or tuple(pred_hf.shape[1:]) != (3, 21):
        raise ValueError(f"hand_seq_metrics: pred_hf must be (F,3,21), got {tuple(pred_hf.shape)}")
    dev = pred_hf.device
    if seq_off is None:
        seq_off = torch.tensor(offsets, dtype=torch.int32, device=dev)
    opt = lambda t, name, n: None if t is None else _native._ptr(t, name, f32, n)
    args = [_native._ptr(pred_hf, "pred_hf", f32, F * 63), _native._ptr(init_hf, "init_hf", f32, F * 63),
            _native._ptr(gt_kp, "gt_kp", f32, F * 63), _native._ptr(pred_kp, "pred_kp", f32, F * 63),
            _native._ptr(Rc, "Rc", f32, F * 9), _native._ptr(tc, "tc", f32, F * 3), _native._ptr(scale, "scale", f32, F),
            opt(palm, "palm", S * 18), _native._ptr(seq_off, "seq_off", torch.int32, S + 1),
            opt(pose_R, "pose_R", F * 9), opt(pose_t, "pose_t", F * 3), opt(gt_R, "gt_R", F * 9), opt(gt_t, "gt_t", F * 3),
            opt(theta, "theta", F * 45), opt(theta_gt, "theta_gt", F * 45)]
    for t in (init_hf, gt_kp, pred_kp, Rc, tc, scale, palm, seq_off, pose_R, pose_t, gt_R, gt_t, theta, theta_gt):
        if t is not None and t.device != dev:
            raise ValueError(f"hand_seq_metrics: tensors on {dev} and {t.device}")
    rows = torch.empty((F, HAND_SEQ_COLS), dtype=f32, device=dev)
    seq = torch.empty((S, HAND_SEQ_COLS), dtype=f32, device=dev)
    if F == 0:  # nothing to launch (an empty tensor has no address to tell a given input from an absent one): zero rows per sequence
        return rows, seq.zero_(), 0x19f | (0x60 if mode == 0 else 0) | (0x600 if gt_R is not None else 0) | (0x800 if theta is not None else 0)
    with torch.cuda.device(dev):
        rc = _native._call(_lib.pn2x_hand_seq_metrics, "hand_seq_metrics", None, F, S, 21, mode, *args, rows.data_ptr(), seq.data_ptr(),
                           _native._stream(pred_hf))
    if rc < 0:
        _native._check(rc, "hand_seq_metrics")
    return rows, seq, int(rc)


# ---- hand-object penetration and contact of tracked hand sequences (include/pn2_ext.h: pn2x_hand_interaction_metrics) -----------
_lib.pn2x_hand_interaction_metrics.argtypes = [_HP_SETUP, _ci, _ci, _ci] + [_vp] * 11 + [_cf] + [_vp] * 5
_lib.pn2x_hand_interaction_metrics.restype = _ci
HAND_INTERACTION_COLS = 8


def hand_interaction_metrics(model, global_r: torch.Tensor, global_t: torch.Tensor, theta: torch.Tensor, obj_r: torch.Tensor,
                             obj_t: torch.Tensor, rest, rest_of: torch.Tensor, volumes, voxel_scale: float, offsets,
                             contact_threshold: float = 0.005, pred_kp: torch.Tensor = None, seq_off: torch.Tensor = None,
                             vol_table: torch.Tensor = None, with_geometry: bool = False):
    """Penetration and contact of F posed hands in S sequences against the sequences' SDF volumes (pn2x_hand_interaction_metrics):
    model = hand_pose_model(...); global_r (F,3,3), global_t (F,3), theta (F,45), obj_r (F,3,3), obj_t (F,3), pred_kp (F,21,3) or
    None; rest = (rest_joints (G,21,3), rest_verts (G,V,3)), the G shape tables (hand_pose_rest, stacked), rest_of (F,) int32 the
    table of each frame; volumes: the S sequences' (res,res,res) fp16 / fp32 volumes (one resolution and dtype; None for a
    sequence without frames); offsets: the HOST list of S + 1 frame offsets.  seq_off / vol_table: the offsets as an int32 and
    the volumes' addresses as an int64 device tensor when the caller holds them (a captured graph must: building them is a
    host-to-device copy).  -> (rows (F,8) and seq (S,8) in metres, mask (bit c: column c is valid), vertices (F,V,3) or None,
    keypoints (F,21,3) or None).  Two launches, no host sync."""
    f32, i32 = torch.float32, torch.int32
    offsets = [int(o) for o in offsets]
    F, S = global_r.shape[0], len(offsets) - 1
    if S < 0 or offsets[0] != 0 or offsets[-1] != F or any(b < a for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"hand_interaction_metrics: offsets must be non-decreasing from 0 to F = {F}, got {offsets}")
    if len(volumes) != S:
        raise ValueError(f"hand_interaction_metrics: {len(volumes)} volumes for {S} sequences")
    if not float(contact_threshold) >= 0:
        raise ValueError(f"hand_interaction_metrics: contact_threshold = {contact_threshold}")
    given = [v for v in volumes if v is not None]
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b > a and volumes[q] is None:
            raise ValueError(f"hand_interaction_metrics: sequence {q} has frames and no volume")
    if not given:
        raise ValueError("hand_interaction_metrics: volumes holds no volume")
    for v in given:
        if v.shape != given[0].shape or v.dtype != given[0].dtype:
            raise ValueError(f"hand_interaction_metrics: volumes {tuple(given[0].shape)} {given[0].dtype} and {tuple(v.shape)} {v.dtype} "
                             "differ: a call shares one resolution and dtype")
    setup = _hand_pose_setup(model, None, 0.0, given[0], voxel_scale, None)
    dev, V, J = global_r.device, model["V"], model["J"]
    rest_j, rest_v = rest
    G = rest_j.shape[0] if rest_j.dim() == 3 else 1
    # (rest_of is device memory and is not read here: the kernel clamps an index outside [0, G) into it)
    if seq_off is None:
        seq_off = torch.tensor(offsets, dtype=i32, device=dev)
    if vol_table is None:
        vol_table = torch.tensor([0 if v is None else _native._ptr(v, "volume", v.dtype, setup.res ** 3) for v in volumes],
                                 dtype=torch.int64, device=dev)
    args = [_native._ptr(global_r, "global_r", f32, F * 9), _native._ptr(global_t, "global_t", f32, F * 3),
            _native._ptr(theta, "theta", f32, F * 45), _native._ptr(obj_r, "obj_r", f32, F * 9), _native._ptr(obj_t, "obj_t", f32, F * 3),
            None if pred_kp is None else _native._ptr(pred_kp, "pred_kp", f32, F * J * 3),
            _native._ptr(rest_j, "rest_joints", f32, G * J * 3), _native._ptr(rest_v, "rest_verts", f32, G * V * 3),
            _native._ptr(rest_of, "rest_of", i32, F), _native._ptr(vol_table, "vol_table", torch.int64, S),
            _native._ptr(seq_off, "seq_off", i32, S + 1)]
    for t in (global_t, theta, obj_r, obj_t, pred_kp, rest_j, rest_v, rest_of, vol_table, seq_off, *given):
        if t is not None and t.device != dev:
            raise ValueError(f"hand_interaction_metrics: tensors on {dev} and {t.device}")
    rows = torch.empty((F, HAND_INTERACTION_COLS), dtype=f32, device=dev)
    seq = torch.empty((S, HAND_INTERACTION_COLS), dtype=f32, device=dev)
    verts = torch.empty((F, V, 3), dtype=f32, device=dev) if with_geometry else None
    kp = torch.empty((F, J, 3), dtype=f32, device=dev) if with_geometry else None
    if F == 0 or S == 0:  # nothing to launch (an empty tensor has no address): zero rows per sequence
        return rows, seq.zero_(), 0xbf | (0x40 if pred_kp is not None else 0), verts, kp
    with torch.cuda.device(dev):
        rc = _native._call(_lib.pn2x_hand_interaction_metrics, "hand_interaction_metrics", None, ctypes.byref(setup), F, S, G, *args,
                           float(contact_threshold), rows.data_ptr(), seq.data_ptr(), None if verts is None else verts.data_ptr(),
                           None if kp is None else kp.data_ptr(), _native._stream(global_r))
    if rc < 0:
        _native._check(rc, "hand_interaction_metrics")
    return rows, seq, int(rc), verts, kp


# ---- hand and object clouds from depth frames (include/pn2_ext.h: pn2x_depth_frame_clouds) --------------------------------------
class _DepthFrame(ctypes.Structure):
    """pn2x_depth_frame (144 bytes)."""
    _fields_ = ([(n, _vp) for n in ("depth", "seg", "intrinsics")] + [("centre", _vp * 2)] +
                [(n, _vp) for n in ("clouds", "counts", "background", "work")] + [("depth_scale", _cd)] +
                [(n, _ci) for n in ("b", "h", "w", "hs", "ws", "c", "cap", "depth_u16", "flip_yz", "reserved")] +
                [("channel", _ci * 2), ("value", _ci * 2), ("radius", _cf * 2)])


_lib.pn2x_depth_frame_supported.argtypes = [_ci] * 6
_lib.pn2x_depth_frame_supported.restype = _ci
_lib.pn2x_depth_frame_work_ints.argtypes = [_ci] * 3
_lib.pn2x_depth_frame_work_ints.restype = _cl
_lib.pn2x_depth_frame_clouds.argtypes = [ctypes.POINTER(_DepthFrame), _vp]
_lib.pn2x_depth_frame_clouds.restype = _ci
DEPTH_FRAME_MAX_CAP = 16384   # the register-resident FPS range
DEPTH_FRAME_CALLS = 0         # calls of depth_frame_clouds so far (tests: a frame that has its clouds never gets here)


def depth_frame_supported(h: int, w: int, hs: int, ws: int, c: int, cap: int) -> bool:
    return bool(_lib.pn2x_depth_frame_supported(int(h), int(w), int(hs), int(ws), int(c), int(cap)))


def depth_frame_workspace(b: int, h: int, w: int, cap: int, device):
    """What a depth_frame_clouds call writes, to be reused: (tile counts, clouds (b,2,cap,3), counts (b,2), background (b,h,w)).
    Nothing in it needs a value: every element is written on every call."""
    ints = int(_lib.pn2x_depth_frame_work_ints(int(b), int(h), int(w)))
    if ints < 0:
        raise ValueError(f"depth_frame_workspace: b = {b}, h = {h}, w = {w}")
    return (torch.empty(max(ints, 1), dtype=torch.int32, device=device), torch.empty((b, 2, cap, 3), dtype=torch.float32, device=device),
            torch.empty((b, 2), dtype=torch.int32, device=device), torch.empty((b, h, w), dtype=torch.uint8, device=device))


def depth_frame_clouds(depth: torch.Tensor, seg: torch.Tensor, intrinsics: torch.Tensor, hand, obj, cap: int, flip_yz: bool = False,
                       depth_scale: float = None, work=None):
    """Back-projection, split by segment and crop to a ball of B depth frames in two launches (pn2x_depth_frame_clouds).
    depth (B,H,W) fp32 metres, or uint16 / int16 raw counts with depth_scale;  seg (B,Hs,Ws,C) uint8, C 1 or 3, H = f Hs and
    W = f Ws;  intrinsics (B,4) fp32 on the device: fx, fy, cx, cy;  hand / obj = (channel, value, centre (B,3) fp32 on the device,
    radius);  cap: slots per cloud, 1..16384;  work: depth_frame_workspace(B, H, W, cap) to write into, else allocated.
    -> (clouds (B,2,cap,3), counts (B,2) int32, background (B,H,W) uint8), as pn2_ext.h describes them.  No host sync."""
    global DEPTH_FRAME_CALLS
    f32, u8 = torch.float32, torch.uint8
    for name, t in (("depth", depth), ("seg", seg), ("intrinsics", intrinsics), ("hand centre", hand[2]), ("obj centre", obj[2])):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"depth_frame_clouds: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"depth_frame_clouds: {name} must be a GPU (HIP) tensor -- hotrack_amd has no CPU path (got device {t.device})")
    if depth.dim() != 3 or seg.dim() != 4 or seg.shape[0] != depth.shape[0]:
        raise ValueError(f"depth_frame_clouds: depth {tuple(depth.shape)} is not (B,H,W) or seg {tuple(seg.shape)} not (B,Hs,Ws,C)")
    B, H, W = depth.shape
    _, Hs, Ws, C = seg.shape
    cap = int(cap)
    raw = depth.dtype in (torch.uint16, torch.int16)   # (int16: the same 16 bits, for a torch without uint16 arithmetic)
    if raw == (depth_scale is None) or (not raw and depth.dtype != f32):
        raise TypeError(f"depth_frame_clouds: depth is fp32 metres, or uint16 counts with a depth_scale (got {depth.dtype}, "
                        f"depth_scale = {depth_scale})")
    if not depth_frame_supported(H, W, Hs, Ws, C, cap):
        raise ValueError(f"depth_frame_clouds: depth {H} x {W}, seg {Hs} x {Ws} x {C}, cap {cap}: one integer factor between the "
                         f"two images, C 1 or 3, H W < 2^29 and 1 <= cap <= {DEPTH_FRAME_MAX_CAP}")
    if work is None:
        work = depth_frame_workspace(B, H, W, cap, depth.device)
    tiles, clouds, counts, background = work
    r = _DepthFrame(b=B, h=H, w=W, hs=Hs, ws=Ws, c=C, cap=cap, depth_u16=int(raw), flip_yz=int(bool(flip_yz)),
                    depth_scale=0.0 if depth_scale is None else float(depth_scale))
    r.depth, r.seg = _native._ptr(depth, "depth", depth.dtype, B * H * W), _native._ptr(seg, "seg", u8, B * Hs * Ws * C)
    r.intrinsics = _native._ptr(intrinsics, "intrinsics", f32, B * 4)
    for k, (channel, value, centre, radius) in enumerate((hand, obj)):
        r.channel[k], r.value[k], r.radius[k] = int(channel), int(value), float(radius)
        r.centre[k] = _native._ptr(centre, "centre", f32, B * 3)
    r.clouds, r.counts = _native._ptr(clouds, "clouds", f32, B * 2 * cap * 3), _native._ptr(counts, "counts", torch.int32, B * 2)
    r.background = _native._ptr(background, "background", u8, B * H * W)
    r.work = _native._ptr(tiles, "work", torch.int32, max(int(_lib.pn2x_depth_frame_work_ints(B, H, W)), 1))
    for t in (seg, intrinsics, hand[2], obj[2], tiles, clouds, counts, background):
        if t.device != depth.device:
            raise ValueError(f"depth_frame_clouds: tensors on {depth.device} and {t.device}")
    DEPTH_FRAME_CALLS += 1
    with torch.cuda.device(depth.device):
        _native._check(_native._call(_lib.pn2x_depth_frame_clouds, "depth_frame_kernels", None, ctypes.byref(r), _native._stream(depth)),
                       "depth_frame_clouds")
    return clouds, counts, background


_lib.pn2x_cloud_normals.argtypes = [_ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.pn2x_cloud_normals.restype = _ci
_lib.pn2x_cloud_normals_limits.argtypes = [ctypes.POINTER(_ci)] * 3
_lib.pn2x_cloud_normals_limits.restype = None


def _cloud_normals_limits():
    b, n, k = _ci(), _ci(), _ci()
    _lib.pn2x_cloud_normals_limits(ctypes.byref(b), ctypes.byref(n), ctypes.byref(k))
    return b.value, n.value, k.value


# PN2X_CLOUD_NORMALS_MAX_B / _MAX_N / _MAX_K, as the library was built with them
CLOUD_NORMALS_MAX_B, CLOUD_NORMALS_MAX_N, CLOUD_NORMALS_MAX_K = _cloud_normals_limits()
CLOUD_NORMALS_ORIENT = {"none": 0, "view": 1, "reference": 2}


def cloud_normals(points: torch.Tensor, k: int = 30, viewpoint=None, valid=None, orient: str = "view"):
    """Oriented normals of B point clouds in one launch, one wave per query (pn2x_cloud_normals): points (B,N,3) fp32 ->
    (normals (B,N,3), variation (B,N)).  For every usable query -- `valid` (B,N) bool / uint8 not 0 (None: all) and finite
    coordinates -- the k nearest usable points of its own cloud, itself included (open3d's estimate_normals convention, whose
    default k is 30; all of them when fewer than k are usable), their covariance in two fp32 passes, the unit eigenvector of the
    smallest eigenvalue by cyclic Jacobi sweeps, and variation = lambda0 / (lambda0 + lambda1 + lambda2).  Zeros for a query that
    is not usable, for fewer than 3 usable points and for neighbours that all coincide.
    viewpoint (B,3) or (3,), None = the origin (the camera in the camera frame).  orient:
      "none"       the component of largest magnitude is positive (a deterministic sign, no geometry);
      "view"       n . (viewpoint - p) >= 0;
      "reference"  the reference's (2 (n (viewpoint - p) > 0) - 1) n, optimization_obj.py:342: a sign per COMPONENT.  It is NOT a
                   geometric orientation (the result need not even be +-n); it is what the reference feeds its shape refit.
    Range: 3 <= N <= CLOUD_NORMALS_MAX_N = 2048 (the register-resident selection), 3 <= k <= CLOUD_NORMALS_MAX_K = 64 (one lane per
    neighbour), B <= CLOUD_NORMALS_MAX_B = 65535.  No host sync."""
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"cloud_normals: points must be a torch.Tensor, got {type(points).__name__}")
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError(f"cloud_normals: points must be (B,N,3), got {tuple(points.shape)}")
    B, N, _ = points.shape
    k = int(k)
    if orient not in CLOUD_NORMALS_ORIENT:
        raise ValueError(f"cloud_normals: orient must be one of {sorted(CLOUD_NORMALS_ORIENT)}, got {orient!r}")
    if B < 1 or not 3 <= N <= CLOUD_NORMALS_MAX_N:
        raise ValueError(f"cloud_normals: {B} clouds of {N} points: at least one cloud of 3 to {CLOUD_NORMALS_MAX_N} points (the "
                         "selection keeps a cloud's distances in one wave's registers)")
    if B > CLOUD_NORMALS_MAX_B:
        raise ValueError(f"cloud_normals: {B} clouds: at most {CLOUD_NORMALS_MAX_B} clouds per call (one row of the launch grid each)")
    if not 3 <= k <= CLOUD_NORMALS_MAX_K:
        raise ValueError(f"cloud_normals: k = {k}: 3 to {CLOUD_NORMALS_MAX_K} neighbours (one lane of the wave per neighbour)")
    f32 = torch.float32
    if points.dtype != f32:
        raise TypeError(f"cloud_normals: points must be {f32}, got {points.dtype}")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError("cloud_normals: valid must be a bool or uint8 tensor")
        if tuple(valid.shape) != (B, N):
            raise ValueError(f"cloud_normals: valid must be ({B},{N}), got {tuple(valid.shape)}")
        if valid.device != points.device:
            raise ValueError(f"cloud_normals: tensors on {points.device} and {valid.device}")
        if valid.dtype == torch.bool:
            valid = valid.contiguous().view(torch.uint8) if valid.is_contiguous() else valid.to(torch.uint8)
    if viewpoint is None:
        viewpoint = torch.zeros((B, 3), dtype=f32, device=points.device)
    else:
        if not isinstance(viewpoint, torch.Tensor) or viewpoint.dtype != f32:
            raise TypeError(f"cloud_normals: viewpoint must be a {f32} tensor")
        if viewpoint.device != points.device:
            raise ValueError(f"cloud_normals: tensors on {points.device} and {viewpoint.device}")
        if tuple(viewpoint.shape) == (3,):
            viewpoint = viewpoint.expand(B, 3).contiguous()
        elif tuple(viewpoint.shape) != (B, 3):
            raise ValueError(f"cloud_normals: viewpoint must be ({B},3) or (3,), got {tuple(viewpoint.shape)}")
    pp = _native._ptr(points, "points", f32, B * N * 3)
    pv = None if valid is None else _native._ptr(valid, "valid", torch.uint8, B * N)
    pc = _native._ptr(viewpoint, "viewpoint", f32, B * 3)
    normals = torch.empty((B, N, 3), dtype=f32, device=points.device)
    variation = torch.empty((B, N), dtype=f32, device=points.device)
    with torch.cuda.device(points.device):
        _native._check(_native._call(_lib.pn2x_cloud_normals, "cloud_normals", None, B, N, k, CLOUD_NORMALS_ORIENT[orient], pp, pv, pc,
                                     normals.data_ptr(), variation.data_ptr(), _native._stream(points)), "cloud_normals")
    return normals, variation
