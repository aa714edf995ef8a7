"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol the headers declare
(no compute calls -- there is no GPU here), and the Python boundary validates its arguments."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pn2[xs]?_[a-z0-9_]+)\s*\(", src)))


def _prototypes():
    """{name: [parameter declarations]} of every entry the three headers declare (comments stripped)."""
    out = {}
    for header in ("pn2_hip.h", "pn2_ext.h", "pn2_sdf.h"):
        src = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
        for m in re.finditer(r"\b(pn2[xs]?_\w+)\s*\(([^()]*)\)\s*;", src):
            params = [p.strip() for p in m.group(2).split(",")]
            out[m.group(1)] = [] if params in ([""], ["void"]) else params
    return out


def _called_entries():
    """Entries the Python bindings call: `lib.<name>(...)` directly, or `lib.<name>` handed to pointnet2_hip._call."""
    called = set()
    for base in ("hotrack_amd", "network"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith(".py"):
                    called |= set(re.findall(r"lib\.(pn2[xs]?_\w+)\s*[(,]", open(os.path.join(dp, f)).read()))
    return called


def test_every_extension_entry_has_a_caller():
    """An entry that nothing calls is dead ABI surface: every pn2x_* the extension header declares is called by the bindings."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2_ext.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2x_\w+)\s*\(", src))
    assert declared
    assert sorted(declared - _called_entries()) == []


def test_bound_argtypes_match_the_header_prototypes():
    """Every entry the bindings call has argtypes, and each list matches the header prototype element by element (int, long,
    float, double or pointer) -- a renamed or re-signatured entry cannot slip through with a stale table."""
    import importlib
    for m in ("pointnet2_hip", "ext", "train_ops", "train_stack", "linear_dw", "tail_train", "optim", "sdf"):
        importlib.import_module("hotrack_amd." + m)
    from hotrack_amd.pointnet2_hip import _lib
    c = ctypes

    def c_kind(param):
        if "*" in param:
            return "pointer"
        words = re.sub(r"\b(const|unsigned)\b", "", param).split()[:-1]  # type words without the parameter name
        return {"int": "int", "long": "long", "float": "float", "double": "double"}[words[0]]

    def py_kind(t):
        if t in (c.c_int, c.c_int32):
            return "int"
        if t in (c.c_long, c.c_longlong, c.c_int64):
            return "long"
        if t in (c.c_float, c.c_double):
            return {c.c_float: "float", c.c_double: "double"}[t]
        if t in (c.c_void_p, c.c_char_p) or issubclass(t, c._Pointer):
            return "pointer"
        raise AssertionError(t)

    protos = _prototypes()
    bad = []
    for name in sorted(_called_entries()):
        assert name in protos, f"{name} is called but no header declares it"
        at = getattr(_lib, name).argtypes
        if at is None:
            bad.append(f"{name}: no argtypes")
            continue
        want, got = [c_kind(p) for p in protos[name]], [py_kind(t) for t in at]
        if want != got:
            bad.append(f"{name}: header {want} != argtypes {got}")
    assert not bad, "\n".join(bad)


def test_headers_declare_the_reference_surface():
    names = _declared("pn2_hip.h")
    for n in ("pn2_ball_query", "pn2_group_points", "pn2_group_points_grad", "pn2_gather_points", "pn2_gather_points_grad",
              "pn2_furthest_point_sampling", "pn2_knn", "pn2_three_nn", "pn2_three_interpolate", "pn2_three_interpolate_grad"):
        assert n in names  # one per m.def of pointnet2_api.cpp:11-24


def test_library_exports_every_declared_symbol(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    for header in ("pn2_hip.h", "pn2_ext.h", "pn2_sdf.h"):
        for name in _declared(header):
            assert hasattr(lib, name), f"{name} declared in {header} but not exported"
    lib.pn2_abi_version.restype = ctypes.c_int
    assert lib.pn2_abi_version() == 4  # 4: the hand-pose entries take a setup and a problem record, the _mano_ entries removed
    lib.pn2_strerror.restype = ctypes.c_char_p
    assert b"NULL" in lib.pn2_strerror(-2)


def test_argument_validation_without_gpu(hip_lib_path):
    """Invalid arguments are rejected before anything touches the device."""
    lib = ctypes.CDLL(hip_lib_path)
    vp = ctypes.c_void_p
    lib.pn2_knn.argtypes = [ctypes.c_int] * 4 + [vp] * 5
    assert lib.pn2_knn(1, 4, 16, 0, None, None, None, None, None) == -1      # k < 1
    assert lib.pn2_knn(1, 4, 16, 201, None, None, None, None, None) == -3    # k > 200 (reference array bound)
    assert lib.pn2_knn(1, 4, 16, 8, None, None, None, None, None) == -2      # NULL pointers
    lib.pn2_furthest_point_sampling.argtypes = [ctypes.c_int] * 3 + [vp] * 4
    assert lib.pn2_furthest_point_sampling(1, 0, 4, None, None, None, None) == -1   # n < 1
    assert lib.pn2_furthest_point_sampling(0, 16, 4, None, None, None, None) == 0   # empty batch is a no-op
    lib.pn2_ball_query.argtypes = [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int] + [vp] * 4
    assert lib.pn2_ball_query(1, 16, 4, 0.1, 0, None, None, None, None) == -1       # nsample < 1
    lib.pn2_group_points.argtypes = [ctypes.c_int] * 5 + [vp] * 4
    assert lib.pn2_group_points(2, 0, 16, 4, 4, None, None, None, None) == 0        # C == 0 is legal (sa1)
    cf, ci = ctypes.c_float, ctypes.c_int
    lib.pn2s_nearest.argtypes = [ci, ci, vp, vp, vp, vp, ci, ci, cf, vp, vp, vp, vp]
    assert lib.pn2s_nearest(4, 8, None, None, None, None, 1, 150, 0.003, None, None, None, None) == -1   # even res
    assert lib.pn2s_nearest(4, 8, None, None, None, None, 1, 151, 0.003, None, None, None, None) == -2   # NULL pointers
    lib.pn2s_trilinear.argtypes = [ci, vp, vp, ci, ci, cf, cf, cf, cf, vp, vp]
    assert lib.pn2s_trilinear(8, None, None, 1, 201, -0.2, 0.0, -0.05, 0.05, None, None) == -1           # stride <= 0
    assert lib.pn2s_trilinear(0, None, None, 1, 201, -0.2, 0.002, -0.05, 0.05, None, None) == 0          # empty is a no-op
    cl = ctypes.c_long
    lib.pn2x_mlp2_rows.argtypes = [cl, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp]
    assert lib.pn2x_mlp2_rows(-1, 128, 128, 128, None, 128, None, None, None, None, None, None, 128, None) == -1  # rows < 0
    assert lib.pn2x_mlp2_rows(8, 128, 128, 128, None, 126, None, None, None, None, None, None, 128, None) == -1   # ldx < c1
    assert lib.pn2x_mlp2_rows(0, 128, 128, 128, None, 128, None, None, None, None, None, None, 128, None) == 0    # no rows: no-op
    assert lib.pn2x_mlp2_rows(8, 128, 128, 128, None, 128, None, None, None, None, None, None, 130, None) == -1   # ldo not a multiple of 4
    assert lib.pn2x_mlp2_rows(8, 128, 128, 128, None, 128, None, None, None, None, None, None, 128, None) == -2   # NULL pointers
    assert lib.pn2x_mlp2_rows_supported(128, 128, 128) == 1 and lib.pn2x_mlp2_rows_supported(96, 96, 96) == 0
    lib.pn2x_ln_linear_small.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, cf, vp, vp, cf, vp, vp, ci, vp, ci, vp, ci, vp]
    assert lib.pn2x_ln_linear_small(21, 385, 64, None, None, None, None, None, 1e-5, None, None, 0.0, None, None, 385, None, 0, None, 64, None) == -1  # k > 384
    assert lib.pn2x_ln_linear_small(21, 192, 64, None, None, None, None, None, 1e-5, None, None, 0.0, None, None, 192, None, 0, None, 64, None) == -2  # NULL
    assert lib.pn2x_ln_linear_small(0, 192, 64, None, None, None, None, None, 1e-5, None, None, 0.0, None, None, 192, None, 0, None, 64, None) == 0   # no rows
    lib.pn2x_kabsch_backward.argtypes = [ci, ci, ci] + [vp] * 7
    assert lib.pn2x_kabsch_backward(4, 2, 6, None, None, None, None, None, None, None) == -1   # x batch neither 1 nor b
    assert lib.pn2x_kabsch_backward(4, 1, 6, None, None, None, None, None, None, None) == -2   # NULL pointers
    assert lib.pn2x_kabsch_backward(0, 1, 6, None, None, None, None, None, None, None) == 0    # empty batch
    assert lib.pn2x_sa_set_compute_units(-3) == -1 and lib.pn2x_sa_set_compute_units(0) == 0
    lib.pn2x_sa_mlp_max.argtypes = [ci] * 7 + [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cl, ci, ci, vp]
    # a row stride whose byte offsets would not fit the 24-bit address multiplier of the gathers is refused, not mis-addressed
    one = ctypes.c_void_p(16)
    assert lib.pn2x_sa_mlp_max(1, 64, 4, 16, 128, 128, 192, one, 1 << 23, one, one, one, one, None, 0, one, one, one, one, one, one, 768, 192, 1, None) == -3


def test_sa_mlp_max_argument_validation_without_gpu(hip_lib_path):
    """pn2x_sa_mlp_max / pn2x_sa_mlp_max_pair refuse every invalid argument before any launch: non-null fake pointers and exactly
    one violation per call.  The *_supported queries answer 1 on exactly the combinations sa_fused.hip instantiates."""
    lib = ctypes.CDLL(hip_lib_path)
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.pn2x_sa_mlp_max.argtypes = [ci] * 7 + [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cl, ci, ci, vp]
    p = vp(16)
    good = dict(b=2, n=64, s=4, k=16, c1=128, c2=128, c3=192, a1f=p, a1f_ld=128, xyz=p, cxyz=p, wx=p, b1=p, cadd=p, cadd_ld=128, idx=p,
                w2=p, b2=p, w3=p, b3=p, out=p, out_b=768, out_s=192, out_c=1, stream=None)

    def call(**change):
        assert set(change) <= set(good)
        return lib.pn2x_sa_mlp_max(*{**good, **change}.values())

    assert call(b=-1) == -1
    assert call(k=0) == -1
    assert call(s=0) == 0                                  # nothing to do
    assert call(b=0) == 0
    assert call(idx=None) == -2
    assert call(a1f=None, xyz=None) == -2                  # layer 1 needs a per-point term
    assert call(cxyz=None) == -2                           # xyz without the centroids
    assert call(a1f_ld=124) == -1                          # a1f_ld < c1
    assert call(a1f_ld=130) == -1                          # rows are read as 16-byte quads
    assert call(cadd_ld=130) == -1
    assert call(k=8) == -3
    assert call(c1=64, c2=64, c3=64, out_b=256, out_s=64) == -3
    assert call(a1f=vp(20)) == -1                          # not 16-byte aligned
    for name in ("w2", "b2", "w3", "b3", "out", "wx"):
        assert call(**{name: None}) == -2, name
    for name in ("cadd", "b1", "w2", "w3"):
        assert call(**{name: vp(20)}) == -1, name
    assert call(n=0) == -1 and call(s=-1) == -1
    assert call(cadd_ld=124) == -1
    assert call(n=1 << 24) == -3 and call(cadd_ld=1 << 23) == -3 and call(out_c=-1) == -3

    class Problem(ctypes.Structure):                       # include/pn2_ext.h: pn2x_sa_problem
        _fields_ = [("n", ci), ("s", ci), ("k", ci), ("a1f", vp), ("a1f_ld", ci), ("xyz", vp), ("cxyz", vp), ("wx", vp), ("b1", vp),
                    ("cadd", vp), ("cadd_ld", ci), ("idx", vp), ("w2", vp), ("b2", vp), ("w3", vp), ("b3", vp), ("out", vp),
                    ("out_b", cl), ("out_s", ci), ("out_c", ci)]

    lib.pn2x_sa_mlp_max_pair.argtypes = [ci] * 4 + [ctypes.POINTER(Problem)] * 2 + [vp]

    def problem(k):
        return Problem(64, 21, k, 16, 128, 16, 16, 16, 16, 16, 128, 16, 16, 16, 16, 16, 16, 21 * 384, 384, 1)

    p16, p32, p64 = problem(16), problem(32), problem(64)
    assert lib.pn2x_sa_mlp_max_pair(2, 128, 128, 192, None, ctypes.byref(p64), None) == -2
    assert lib.pn2x_sa_mlp_max_pair(2, 128, 128, 192, ctypes.byref(p16), None, None) == -2
    assert lib.pn2x_sa_mlp_max_pair(-1, 128, 128, 192, ctypes.byref(p16), ctypes.byref(p64), None) == -1
    assert lib.pn2x_sa_mlp_max_pair(2, 128, 128, 192, ctypes.byref(p32), ctypes.byref(p64), None) == -3
    assert lib.pn2x_sa_mlp_max_pair(0, 128, 128, 192, ctypes.byref(p16), ctypes.byref(p64), None) == 0

    # every field of a record, one fault per call, in the first record and in the second: none reaches a launch
    def pair(first, **change):
        bad = problem(16 if first else 64)
        for name, value in change.items():
            assert name in dict(Problem._fields_)
            setattr(bad, name, value)
        recs = (bad, p64) if first else (p16, bad)
        return lib.pn2x_sa_mlp_max_pair(2, 128, 128, 192, ctypes.byref(recs[0]), ctypes.byref(recs[1]), None)

    for first in (True, False):
        for name in ("idx", "w2", "b2", "w3", "b3", "out", "cxyz", "wx"):
            assert pair(first, **{name: None}) == -2, name
        assert pair(first, a1f=None, xyz=None) == -2                 # layer 1 needs a per-point term
        for name in ("a1f_ld", "cadd_ld"):
            assert pair(first, **{name: 124}) == -1, name            # below c1
            assert pair(first, **{name: 130}) == -1, name            # rows are read as 16-byte quads
            assert pair(first, **{name: 1 << 23}) == -3, name        # a row stride past the 24-bit multiplier
        for name in ("a1f", "cadd", "b1", "w2", "w3"):
            assert pair(first, **{name: 20}) == -1, name             # not 16-byte aligned
        assert pair(first, n=0) == -1 and pair(first, s=0) == -1
        assert pair(first, k=0) == -3                                # (k0, k1) is tested first: not a supported pair
        assert pair(first, n=1 << 24) == -3 and pair(first, s=1 << 24) == -3   # row numbers past 24 bits
        assert pair(first, out_s=-384) == -3
        # the two records must name the same layer-1 operands, a1f + xyz (+ cadd)
        assert pair(first, cadd=None) == -3 and pair(first, a1f=None) == -3 and pair(first, xyz=None) == -3

    widths = {(32, 32, 64), (64, 64, 128), (128, 128, 192)}
    near = sorted(widths | {(32, 32, 32), (32, 64, 64), (64, 64, 64), (64, 64, 192), (64, 128, 128), (128, 128, 128), (128, 128, 256),
                            (128, 192, 192), (192, 192, 192), (16, 16, 32), (32, 32, 128), (64, 32, 128), (128, 64, 192), (0, 0, 0)})
    ks = (0, 1, 8, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 65, 128)
    for w in near:
        for k in ks:
            assert lib.pn2x_sa_mlp_max_supported(k, *w) == int(w in widths and k in (16, 32, 64)), (k, w)
        for k0 in ks:
            for k1 in ks:
                assert lib.pn2x_sa_mlp_max_pair_supported(k0, k1, *w) == int(w == (128, 128, 192) and (k0, k1) in ((16, 64), (64, 16))), (k0, k1, w)


def _header_records():
    """{record name: [(field name, kind)]} of every `typedef struct pn2x_* { ... }` the three headers declare, in declaration
    order; kind = pointer / int / long / float / double (comments stripped as in _prototypes)."""
    out = {}
    for header in ("pn2_hip.h", "pn2_ext.h", "pn2_sdf.h"):
        src = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
        for m in re.finditer(r"typedef\s+struct\s+(pn2x_\w+)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
            assert m.group(3) == m.group(1)
            fields = []
            for stmt in filter(None, (s.strip() for s in m.group(2).split(";"))):
                first, *more = [d.strip() for d in stmt.split(",")]
                words = re.sub(r"\b(const|unsigned)\b", "", first.replace("*", " * ")).split()
                base = {"int": "int", "long": "long", "float": "float", "double": "double"}.get(words[0], "other")
                for d in (first, *more):
                    kind = "pointer" if "*" in d else base
                    assert kind != "other", (m.group(1), stmt)
                    fields.append((re.findall(r"\w+", d)[-1], kind))
            out[m.group(1)] = fields
    return out


def test_bound_records_match_the_header_structs():
    """Every problem record of the headers has a ctypes.Structure in the bindings whose _fields_ match it field by field (name,
    order, kind) and whose size is the one the library asserts beside the entry (static_assert(sizeof(...) == N))."""
    from hotrack_amd import ext, train_ops, train_stack
    c = ctypes
    bound = {"pn2x_sa_problem": ext._SaProblem, "pn2x_hand_pose_problem": ext._HandPoseProblem,
             "pn2x_hand_pose_setup": ext._HandPoseSetup,
             "pn2x_sa_layer1_stats_problem": train_ops._SaLayer1StatsProblem,
             "pn2x_rows_segment_sum_problem": train_ops._RowsSegmentSumProblem,
             "pn2x_bn_relu_max_problem": train_ops._BnReluMaxProblem,
             "pn2x_bn_bwd_reduce_routed_problem": train_stack._BnBwdReduceRoutedProblem,
             "pn2x_bn_bwd_apply_rel_problem": train_stack._BnBwdApplyRelProblem,
             "pn2x_tg_fwd2_problem": train_stack._TgFwd2Problem, "pn2x_tg_bwd_slice_problem": train_stack._TgBwdSliceProblem}
    kinds = {c.c_void_p: "pointer", c.c_int: "int", c.c_long: "long", c.c_float: "float", c.c_double: "double"}
    records = _header_records()
    assert sorted(records) == sorted(bound)
    csrc = os.path.join(ROOT, "hotrack_amd", "csrc")
    asserted = {}
    for f in os.listdir(csrc):
        if f.endswith(".hip"):
            for name, size in re.findall(r"static_assert\(sizeof\((pn2x_\w+)\) == (\d+)", open(os.path.join(csrc, f)).read()):
                asserted[name] = int(size)
    for name, fields in records.items():
        assert [(n, kinds[t]) for n, t in bound[name]._fields_] == fields, name
        assert c.sizeof(bound[name]) == asserted[name], name
    # pointers, then 8-byte, then 4-byte scalars in the records of the training operators and the hand-pose setup: no implicit padding
    for name in sorted(set(records) - {"pn2x_sa_problem", "pn2x_hand_pose_problem"}):
        sizes = [c.sizeof(t) for _, t in bound[name]._fields_]
        assert sizes == sorted(sizes, reverse=True) and sum(sizes) == c.sizeof(bound[name]), name


def test_training_record_entries_validate_without_gpu(hip_lib_path):
    """The seven record entries of the training operators refuse an invalid record -- the first or the second of a pair -- with the
    code the rule has, before any launch: fake non-null pointers, one violation per call."""
    from hotrack_amd import train_ops as TO, train_stack as TS
    lib = TO._lib
    P = 16  # a fake, 16-byte aligned, non-null pointer
    EINVAL, ENULL, ESCRATCH = -1, -2, -4

    def rec(cls, **values):
        r = cls(**{n: P for n, t in cls._fields_ if t is ctypes.c_void_p})
        for n, v in values.items():
            setattr(r, n, v)
        return r

    def arr(*records):
        return (type(records[0]) * len(records))(*records)

    def cases(call, good, violations, other=None):
        """call(array, count) -> code.  violations: (field changes, code); each is tried alone and as the second of a pair whose
        first record (`other`, or the good one) is valid."""
        for change, code in violations:
            bad = good(**change)
            assert call(arr(bad), 1) == code, change
            assert call(arr((other or good)(), bad), 2) == code, change

    # pn2x_tg_fwd2
    fwd = lambda **ch: rec(TS._TgFwd2Problem, **{**dict(rows=640, k=128, n=128, ldx=128, ldw=128, ldy=128, eps=1e-5, momentum=0.1), **ch})
    call = lambda a, n: lib.pn2x_tg_fwd2(a, n, None)
    assert call(arr(fwd()), 0) == EINVAL and call(arr(fwd(), fwd(), fwd()), 3) == EINVAL and call(None, 1) == ENULL
    cases(call, fwd, [(dict(ldx=124), EINVAL), (dict(ldw=130), EINVAL), (dict(ldy=64), EINVAL), (dict(x=20), EINVAL), (dict(w=None), ENULL),
                      (dict(rows=0), EINVAL), (dict(k=96, ldx=96, ldw=96), EINVAL)])
    assert call(arr(fwd(), fwd(n=192, ldy=192)), 2) == EINVAL   # unequal layer shapes
    assert call(arr(fwd(), fwd(k=64)), 2) == EINVAL
    # pn2x_tg_bwd_slice
    bwd = lambda **ch: rec(TS._TgBwdSliceProblem, **{**dict(
        rows=640, partial_floats=1 << 40, n=128, k=128, gmode=0, ldg=128, ldarg=128, kmax=1, ldyi=128, sums_ld=128, ldw=128, ldyp=128,
        ldgp=128, ldga=128, raw_out=0), **ch})
    nparts = (ctypes.c_int * 2)()
    call = lambda a, n: lib.pn2x_tg_bwd_slice(a, n, nparts, None)
    assert call(arr(bwd()), 0) == EINVAL and call(arr(bwd(), bwd(), bwd()), 3) == EINVAL and call(None, 1) == ENULL
    assert lib.pn2x_tg_bwd_slice(arr(bwd(), bwd()), 2, None, None) == ENULL   # a pair reports both partial counts
    cases(call, bwd, [(dict(ldg=124), EINVAL), (dict(ldyp=130), EINVAL), (dict(sums_ld=64), EINVAL), (dict(gmode=3), EINVAL),
                      (dict(gmode=2, kmax=3), EINVAL), (dict(gmode=2, arg=None), ENULL), (dict(gp=24), EINVAL), (dict(dw=None), ENULL),
                      (dict(g_add=P, ldga=64), EINVAL), (dict(partial_floats=0), ESCRATCH)])
    assert call(arr(bwd(), bwd(n=192, ldg=192, ldyi=192, sums_ld=192)), 2) == EINVAL   # unequal layer shapes
    assert call(arr(bwd(), bwd(k=64)), 2) == EINVAL
    assert call(arr(bwd(), bwd(gmode=1)), 2) == EINVAL                                 # unequal gradient sources
    assert call(arr(bwd(partial_floats=0), bwd()), 2) == ESCRATCH
    # pn2x_bn_relu_max
    mx = lambda **ch: rec(TO._BnReluMaxProblem, **{**dict(groups=300, k=24, c=64, ldy=64, ldo=72, eps=1e-5, momentum=0.1), **ch})
    call = lambda a, n: lib.pn2x_bn_relu_max(a, n, None)
    assert call(arr(mx()), 0) == EINVAL and call(arr(mx(), mx(), mx()), 3) == EINVAL and call(None, 2) == ENULL
    cases(call, mx, [(dict(ldo=60), EINVAL), (dict(ldo=66), EINVAL), (dict(ldy=62), EINVAL), (dict(c=1028, ldy=1028, ldo=1028), EINVAL),
                     (dict(out=20), EINVAL), (dict(arg=None), ENULL), (dict(k=0), EINVAL)])
    # pn2x_bn_bwd_reduce_routed
    rt = lambda **ch: rec(TS._BnBwdReduceRoutedProblem, **{**dict(groups=300, k=24, c=64, ldd=128, lda=64, ldy=64), **ch})
    call = lambda a, n: lib.pn2x_bn_bwd_reduce_routed(a, n, None)
    assert call(arr(rt()), 0) == EINVAL and call(arr(rt(), rt(), rt()), 3) == EINVAL and call(None, 1) == ENULL
    cases(call, rt, [(dict(ldd=60), EINVAL), (dict(lda=32), EINVAL), (dict(ldy=32), EINVAL), (dict(c=6), EINVAL), (dict(sums=None), ENULL),
                     (dict(groups=1 << 30, k=64), EINVAL)])
    # pn2x_bn_bwd_apply_rel
    ar = lambda **ch: rec(TS._BnBwdApplyRelProblem, **{**dict(rows=7200, scratch_floats=1 << 40, c=64, ldg=64, ldy=64, relu=0, ldo=64), **ch})
    call = lambda a, n: lib.pn2x_bn_bwd_apply_rel(a, n, None)
    assert call(arr(ar()), 0) == EINVAL and call(arr(ar(), ar(), ar()), 3) == EINVAL and call(None, 1) == ENULL
    cases(call, ar, [(dict(ldg=60), EINVAL), (dict(ldo=66), EINVAL), (dict(c=260, ldg=260, ldy=260, ldo=260), EINVAL), (dict(dy=24), EINVAL),
                     (dict(rel=None), ENULL), (dict(dbias=None, dwx=None), ENULL), (dict(scratch_floats=3 * 64 - 1), ESCRATCH)])
    # pn2x_sa_layer1_stats (b, n, s, xyz, cxyz shared)
    sa = lambda **ch: rec(TO._SaLayer1StatsProblem, **{**dict(k=16, c1=32, a1f_ld=64, wx_ld=3, cadd_ld=64), **ch})
    call = lambda a, n, b=2, xyz=P, cxyz=P: lib.pn2x_sa_layer1_stats(a, n, b, 300, 37, xyz, cxyz, None)
    assert call(arr(sa()), 0) == EINVAL and call(arr(sa(), sa(), sa()), 3) == EINVAL and call(None, 1) == ENULL
    cases(call, sa, [(dict(a1f_ld=28), EINVAL), (dict(cadd_ld=34), EINVAL), (dict(wx_ld=2), EINVAL), (dict(a1f=24), EINVAL),
                     (dict(sums=None), ENULL), (dict(idx=None), ENULL), (dict(k=0), EINVAL), (dict(c1=6), EINVAL),
                     (dict(c1=12, a1f_ld=8), EINVAL)])        # (c1 = 12: the statistics cannot be taken in the launch)
    assert call(arr(sa(), sa()), 2, cxyz=None) == ENULL and call(arr(sa(), sa()), 2, b=-1) == EINVAL
    assert call(arr(sa(), sa(idx=None)), 2, b=0) == 0        # an empty batch: nothing is read
    # pn2x_rows_segment_sum (b, n_dst, accumulate shared)
    sg = lambda **ch: rec(TO._RowsSegmentSumProblem, **{**dict(m_src=96, t=1, c=8, ldo=8, ldi=16), **ch})
    call = lambda a, n, b=2, n_dst=64: lib.pn2x_rows_segment_sum(a, n, b, n_dst, 0, None)
    assert call(arr(sg()), 0) == EINVAL and call(arr(sg(), sg(), sg()), 3) == EINVAL and call(None, 1) == ENULL
    cases(call, sg, [(dict(ldo=4), EINVAL), (dict(ldi=18), EINVAL), (dict(t=2), EINVAL), (dict(c=6), EINVAL), (dict(din=20), EINVAL),
                     (dict(order=None), ENULL), (dict(t=3, weight=None), ENULL)])
    cases(call, sg, [(dict(ldo=4), EINVAL), (dict(t=3, weight=None), ENULL)], other=lambda: sg(t=3, m_src=40))   # beside a t == 3 problem
    assert call(arr(sg(), sg()), 2, n_dst=0) == EINVAL
    assert call(arr(sg(c=0, dout=None), sg(c=0)), 2) == 0    # no channels: nothing to do


def test_python_boundary_exports_reference_names():
    from hotrack_amd import pointnet2_hip, pointnet2_utils
    for n in pointnet2_hip.EXPORTED:
        assert callable(getattr(pointnet2_hip, n))
    for n in ("furthest_point_sample", "gather_operation", "knn", "three_nn", "three_interpolate", "grouping_operation",
              "ball_query", "QueryAndGroup", "GroupAll", "KNNAndGroup", "FurthestPointSampling", "GatherOperation", "KNN",
              "ThreeNN", "ThreeInterpolate", "GroupingOperation", "BallQuery"):
        assert hasattr(pointnet2_utils, n)


def test_cpu_tensors_fail_loudly():
    from hotrack_amd import pointnet2_utils as ops
    xyz = torch.rand(1, 32, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.furthest_point_sample(xyz, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ball_query(0.1, 4, xyz, xyz[:, :4].contiguous())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.three_nn(xyz, xyz)
    with pytest.raises(TypeError):
        ops.furthest_point_sample(xyz.double(), 8)


def test_product_code_never_imports_the_oracle():
    bad = []
    for base in ("hotrack_amd", "network", "configs", "datasets"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp")):
                    txt = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "pn2_oracle" in txt:
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_tuned_gemm_table_is_well_formed():
    from hotrack_amd import gemm_tuning
    rows = [l.strip().split(",") for l in open(gemm_tuning.RESULTS) if l.strip()]
    assert any(r[0] == "Validator" and r[1] == "GCN_ARCH_NAME" and r[2].startswith("gfx950") for r in rows)
    ops = [r for r in rows if r[0] != "Validator"]
    assert len(ops) > 50 and all(len(r) >= 3 and r[0].startswith("Gemm") for r in ops)
    rec = gemm_tuning.recorded_on()  # the library build the solution indices are valid for travels with the table
    assert rec.get("HIPBLASLT_VERSION") and rec.get("ROCBLAS_VERSION") and rec.get("PT_VERSION")
    if not torch.cuda.is_available():
        assert gemm_tuning.enable() is False  # no GPU: nothing is touched
        assert gemm_tuning.status()["gemm_table"] == "off"


def test_build_refuses_kernels_with_scratch_memory(tmp_path):
    """The build parses hipcc's kernel-resource-usage remarks and fails on any kernel that uses scratch (private) memory
    (hot tg_bwd / tg_dgrad instantiations kept a register array there unnoticed)."""
    import subprocess
    from hotrack_amd import _build
    sample = ("a.hip:1:1: remark: Function Name: _Z3foov [-Rpass-analysis=kernel-resource-usage]\n"
              "a.hip:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
              "a.hip:9:1: remark: Function Name: _Z3barv [-Rpass-analysis=kernel-resource-usage]\n"
              "a.hip:9:1: remark:     ScratchSize [bytes/lane]: 48 [-Rpass-analysis=kernel-resource-usage]\n")
    assert _build.scratch_kernels(sample) == {"_Z3barv": 48}
    # a real compile: a dynamically indexed private array must live in scratch memory
    src = tmp_path / "scr.hip"
    src.write_text('#include <hip/hip_runtime.h>\n__global__ void k(float *o, const int *i, int n) {\n  float a[64];\n'
                   '  for (int j = 0; j < 64; ++j) a[j] = o[j];\n  for (int j = 0; j < n; ++j) a[i[j] & 63] += 1.f;\n'
                   '  o[threadIdx.x] = a[i[threadIdx.x] & 63];\n}\n')
    p = subprocess.run([_build._hipcc(), *_build.HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o",
                        str(tmp_path / "scr.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-500:]
    assert list(_build.scratch_kernels(p.stderr).values())[0] >= 256


def test_streams_in_flight_warns_once_about_hardware_queues(monkeypatch):
    """several captured forwards in flight need GPU_MAX_HW_QUEUES >= streams + 1 before the runtime starts;
    hotrack_amd.streams_in_flight says so once instead of silently running the streams behind each other."""
    import warnings
    import hotrack_amd
    monkeypatch.setattr(hotrack_amd, "_hw_queue_warned", False)
    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert hotrack_amd.streams_in_flight(1) is True and not w
        assert hotrack_amd.streams_in_flight(4) is False and len(w) == 1 and "GPU_MAX_HW_QUEUES=8" in str(w[0].message)
        assert hotrack_amd.streams_in_flight(4) is False and len(w) == 1   # once
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")
    assert hotrack_amd.streams_in_flight(4) is True
