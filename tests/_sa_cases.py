"""Seeded cases and the plain reference for the fused set-abstraction kernel (hotrack_amd/csrc/sa_fused.hip: pn2x_sa_mlp_max and
pn2x_sa_mlp_max_pair) over every instantiation -- 3 width sets x 3 neighbourhood sizes x 4 operand modes -- and the index, tile and
grid edges of its persistent loop.  Everything here is CPU tensors; tests/test_sa_cases.py anchors the reference to the network's
own set-abstraction scale and checks every case's preconditions, tests/test_gpu_sa_mlp_max.py runs the kernels.

  reference_sa     h1 = relu(a1f[idx] + (xyz[idx] - c_s) Wx^T + b1 + cadd_s), two more layers, max over the K neighbours, in `dtype`
  get_case         a row of the table by name, built once from its seed (the cases are read-only)
  kernel_args      the case as the keyword arguments of ext.sa_mlp_max on a device (column blocks stay column blocks)
  ratio / compare  |got - ref64| / (ATOL + RTOL |ref64|), its maximum asserted <= 1

Weights are BatchNorm-folded-like (tests/test_gpu_mid_chain.py::_lin): randn / sqrt(fan-in) times a per-channel scale in
[0.5, 1.5), biases 0.1 randn, wx and b1 included; a1f and cadd are 0.5 randn, coordinates uniform in [0, 1)."""
from types import SimpleNamespace

import torch

# The bound the suite applies to same-depth fp32-MFMA chains with this weight scaling (test_gpu_mid_chain.py,
# test_mlp2_rows_matches_torch).  A float32 torch evaluation of reference_sa is within 0.1 of it (test_sa_cases.py asserts the
# bound itself for every case), a wrong neighbour, centroid or operand moves outputs by 1e-2 or more (test_sa_cases.py proves it).
ATOL, RTOL = 2e-5, 1e-5
WIDTHS = ((32, 32, 64), (64, 64, 128), (128, 128, 192))
KS = (16, 32, 64)
# layer-1 operand sets: a = a1f, x = xyz (with cxyz and wx), c = cadd.  The first three have a kernel instance of their own
# (MODE 0, 1, 2), the last three share the one that tests its operands at run time (MODE 3).
OPERANDS = ("x", "ax", "axc", "a", "ac", "xc")
FORMS = ("cm", "pm", "block")  # (B, C3, S) | point_major=True | out= a column block of a wider (B, S, C3 + 8) buffer
SENTINEL = -7.0
OUT_PAD, OUT_OFF = 8, 4      # the output block: columns [4, 4 + C3) of C3 + 8
A1F_PAD, A1F_OFF = 8, 4      # a1f as columns [4, 4 + C1) of C1 + 8 (block form), NaN around it
CADD_PAD, CADD_OFF = 12, 8   # cadd as columns [8, 8 + C1) of C1 + 12


def _lin(g, o, i):
    scale = 0.5 + torch.rand(o, 1, generator=g)
    return (torch.randn(o, i, generator=g) / i ** 0.5 * scale).contiguous(), torch.randn(o, generator=g) * 0.1


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _rows(t, idx):
    """t (B, R, C), idx (B, ...) -> (B, ..., C)."""
    B = t.shape[0]
    batch = torch.arange(B).view([B] + [1] * (idx.dim() - 1)).expand_as(idx)
    return t[batch, idx.long()]


def reference_sa(dtype, idx, a1f, xyz, cxyz, wx, b1, cadd, w2, b2, w3, b3):
    """One set-abstraction scale in `dtype`, (B, S, C3).  idx (B, S, K) any K; a1f (B, N, C1) | None; xyz (B, N, 3) with cxyz
    (B, S, 3) and wx (C1, 3) | None; b1 (C1) | None; cadd (B, S, C1) | None.  An absent operand contributes 0."""
    def d(t):
        return None if t is None else t.to(dtype)

    B, S, K = idx.shape
    h1 = torch.zeros(B, S, K, w2.shape[1], dtype=dtype)
    if a1f is not None:
        h1 = h1 + _rows(d(a1f), idx)
    if xyz is not None:
        h1 = h1 + (_rows(d(xyz), idx) - d(cxyz)[:, :, None, :]) @ d(wx).t()
    if b1 is not None:
        h1 = h1 + d(b1)
    if cadd is not None:
        h1 = h1 + d(cadd)[:, :, None, :]
    h1 = torch.relu(h1)
    h2 = torch.relu(h1 @ d(w2).t() + d(b2))
    h3 = torch.relu(h2 @ d(w3).t() + d(b3))
    return h3.amax(dim=2)


def reference_of(case, dtype=torch.float64, **override):
    """reference_sa on the case's tensors, any of them replaced by keyword (the perturbations of test_sa_cases.py)."""
    a = dict(idx=case.idx, a1f=case.a1f, xyz=case.xyz, cxyz=case.cxyz, wx=case.wx, b1=case.b1, cadd=case.cadd, w2=case.w2, b2=case.b2,
             w3=case.w3, b3=case.b3)
    a.update(override)
    return reference_sa(dtype, **a)


def ref64(case):
    """The case's float64 reference, computed once and left unchanged."""
    if case._ref64 is None:
        case._ref64 = reference_of(case)
    return case._ref64


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def ratio(got, ref):
    """max |got - ref| / (ATOL + RTOL |ref|); nan if anything in `got` is not finite."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def compare(got, ref, what):
    r = ratio(got, ref)
    print(f"{what}: worst |got - ref64| / (atol + rtol |ref64|) = {r:.4f}")
    assert r <= 1.0, f"{what}: {r:.4g} times the bound atol={ATOL:g} rtol={RTOL:g}"
    return r


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _indices(g, kind, B, N, S, K):
    idx = torch.randint(0, N, (B, S, K), generator=g, dtype=torch.int32)
    if kind == "ends":      # the last point of the last cloud everywhere (its 16-byte coordinate read ends past the tensor), point 0 of the first
        idx[B - 1] = N - 1
        idx[0] = 0
    elif kind == "last":    # one cloud: the descriptor of xyz ends where the tensor ends, and every second centroid reads only its last point
        idx[B - 1, ::2] = N - 1
    elif kind == "padded":  # ball-query lists: 1 + s % K distinct neighbours, the rest repeat the first
        assert N >= K
        for b in range(B):
            for s in range(S):
                n = 1 + s % K
                idx[b, s, :n] = torch.randperm(N, generator=g)[:n].int()
                idx[b, s, n:] = idx[b, s, 0]
    elif kind == "dup":     # the second half of every list names the copies (points N/2 ...) of the first half's points
        assert N % 2 == 0
        idx[:, :, :K // 2] %= N // 2
        idx[:, :, K // 2:] = idx[:, :, :K // 2] + N // 2
    else:
        assert kind == "random"
    return idx


def forced_channels(C3):
    """(channels b3 forces to zero, channels b3 keeps positive) of the "b3" cases: every third channel each, so both kinds fall
    into every 16-channel tile and every lane group of the max-pool's store."""
    c = torch.arange(C3)
    return c % 3 == 0, c % 3 == 1


def make_case(name, widths, K, B, N, S, ops, has_b1, form, seed, index_kind="random", b3_kind=None, cus=0):
    """Every input of ext.sa_mlp_max from a seed, on the CPU.  form "block": the output is a column block, and so are a1f and
    cadd (of buffers that hold NaN elsewhere); `cus`: the compute-unit cap the GPU test also runs the case under (0 = none)."""
    C1, C2, C3 = widths
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(name=name, widths=tuple(widths), K=K, B=B, N=N, S=S, ops=ops, form=form, cus=cus, index_kind=index_kind,
                        b3_kind=b3_kind, _ref64=None)
    c.wx, b1 = _lin(g, C1, 3)
    c.w2, c.b2 = _lin(g, C2, C1)
    c.w3, c.b3 = _lin(g, C3, C2)
    a1f, cadd = 0.5 * torch.randn(B, N, C1, generator=g), 0.5 * torch.randn(B, S, C1, generator=g)
    c.xyz, c.cxyz = torch.rand(B, N, 3, generator=g), torch.rand(B, S, 3, generator=g)
    c.idx = _indices(g, index_kind, B, N, S, K)
    if index_kind == "dup":
        a1f[:, N // 2:] = a1f[:, :N // 2]
        c.xyz[:, N // 2:] = c.xyz[:, :N // 2]
    if b3_kind == "forced":
        zero, pos = forced_channels(C3)
        c.b3[zero], c.b3[pos] = -100.0, 5.0
    c.b1 = b1 if has_b1 else None
    if "x" not in ops:
        c.xyz = c.cxyz = c.wx = None
    pad_a, off_a = (A1F_PAD, A1F_OFF) if form == "block" else (0, 0)
    pad_c, off_c = (CADD_PAD, CADD_OFF) if form == "block" else (0, 0)
    c.a1f_wide, c.a1f_off, c.cadd_wide, c.cadd_off = None, off_a, None, off_c
    if "a" in ops:
        c.a1f_wide = torch.full((B, N, C1 + pad_a), float("nan"))
        c.a1f_wide[:, :, off_a:off_a + C1] = a1f
    if "c" in ops:
        c.cadd_wide = torch.full((B, S, C1 + pad_c), float("nan"))
        c.cadd_wide[:, :, off_c:off_c + C1] = cadd
    _views(c)
    return c


def _views(c):
    C1 = c.widths[0]
    c.a1f = None if c.a1f_wide is None else c.a1f_wide[:, :, c.a1f_off:c.a1f_off + C1]
    c.cadd = None if c.cadd_wide is None else c.cadd_wide[:, :, c.cadd_off:c.cadd_off + C1]


def kernel_args(case, device="cpu"):
    """The keyword arguments of ext.sa_mlp_max (without out / point_major) on `device`; a1f and cadd are views of their wide
    buffers there, as they are here."""
    def d(t):
        return None if t is None else t.to(device).contiguous()

    C1 = case.widths[0]
    a, cd = d(case.a1f_wide), d(case.cadd_wide)
    return dict(idx=d(case.idx), w2=d(case.w2), b2=d(case.b2), w3=d(case.w3), b3=d(case.b3),
                a1f=None if a is None else a[:, :, case.a1f_off:case.a1f_off + C1], xyz=d(case.xyz), cxyz=d(case.cxyz), wx=d(case.wx),
                b1=d(case.b1), cadd=None if cd is None else cd[:, :, case.cadd_off:case.cadd_off + C1])


# ---- the table of tests/test_gpu_sa_mlp_max.py -------------------------------------------------------------------------------------
W32, W128 = WIDTHS[0], WIDTHS[2]
EDGE_CONFIGS = ((W128, 16), (W128, 64), (W32, 32))   # index edges
GRID_CONFIGS = ((W128, 16), (W32, 64))               # tile and grid edges


def case_specs():
    """name -> make_case arguments."""
    s = {}

    def add(name, widths, K, B, N, S, ops, has_b1, form, **kw):
        s[name] = dict(widths=widths, K=K, B=B, N=N, S=S, ops=ops, has_b1=has_b1, form=form, seed=1000 + len(s), **kw)

    # 1. every instantiation: S K = 176, 352, 704 -- every cloud ends in a partial tile of 64 or 128 positions at K = 16 and 32.
    #    b1 is absent in every second case; the output form rotates so that every operand set meets every form at every width.
    for wi, widths in enumerate(WIDTHS):
        for ki, K in enumerate(KS):
            for oi, ops in enumerate(OPERANDS):
                add(f"inst-{widths[0]}-K{K}-{ops}", widths, K, 3, 50, 11, ops, (oi + ki) % 2 == 0, FORMS[(oi + ki + wi) % 3])
    # 2. index edges, all three operands.  S = 67 > K: the padded lists reach both 1 and K distinct entries.
    for ci, (widths, K) in enumerate(EDGE_CONFIGS):
        for ei, (edge, kw) in enumerate((("ends", dict(index_kind="ends")), ("padded", dict(index_kind="padded")),
                                         ("dup", dict(index_kind="dup")), ("b3", dict(b3_kind="forced")))):
            add(f"edge-{edge}-{widths[0]}-K{K}", widths, K, 3, 70, 67, "axc", True, FORMS[(ci + ei) % 3], **kw)
        add(f"edge-last-1cloud-{widths[0]}-K{K}", widths, K, 1, 70, 67, "axc", True, FORMS[ci % 3], index_kind="last")
    # 3. tile and grid edges.  A tile is 64 positions at 128-128-192 and 128 at 32-32-64.
    for ci, (widths, K) in enumerate(GRID_CONFIGS):
        tag = f"{widths[0]}-K{K}"
        add(f"grid-1x1-{tag}", widths, K, 1, 50, 1, "axc", True, FORMS[ci % 3])
        add(f"grid-2x8-{tag}", widths, K, 2, 50, 8, "axc", True, FORMS[(ci + 1) % 3])          # S K = 128 (K = 16) / 512: whole tiles only
        # several tiles per workgroup, the (cloud, tile) cursor crossing clouds: 3 CUs give 3 workgroups over 5 x 6 tiles at
        # 128-128-192 (the grid divides a cloud's tiles) and 6 over 5 x 11 at 32-32-64 (it does not); 4 CUs give 4 over 5 x 6
        add(f"grid-5x21-cu3-{tag}", widths, K, 5, 64, 21, "axc", True, FORMS[(ci + 2) % 3], cus=3)
    add("grid-2x2-32-K64", W32, 64, 2, 50, 2, "axc", True, "pm")                                 # S K = 128: exactly one tile of 128
    add("grid-5x21-cu4-128-K16", W128, 16, 5, 64, 21, "axc", True, "cm", cus=4)
    add("production-33x1024x21-128-K64", W128, 64, 33, 1024, 21, "axc", True, "pm")             # 693 tiles: three rounds of 231 workgroups
    return s


CASES = tuple(case_specs())
_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = make_case(name=name, **case_specs()[name])
    return _CASES[name]


# ---- the pair kernel --------------------------------------------------------------------------------------------------------------
PAIR_ORDERS = ((16, 64), (64, 16))
PAIR_B, PAIR_N, PAIR_J = 2, 64, 21
_PAIRS = {}


def get_pair(order, with_cadd):
    """Both scales of a keypoint-query module as two cases (widths 128-128-192, their own weights and index lists) over the same
    points and keypoints, a1f (and cadd) the two column halves of one (B, N, 2 C1) buffer as the inference path lays them out."""
    key = (tuple(order), bool(with_cadd))
    if key in _PAIRS:
        return _PAIRS[key]
    C1 = W128[0]
    ops = "axc" if with_cadd else "ax"
    cases = [make_case(f"pair-{order[0]}-{order[1]}-{ops}-p{i}", W128, K, PAIR_B, PAIR_N, PAIR_J, ops, True, "cm",
                       seed=5000 + 10 * order[0] + 2 * int(with_cadd) + i) for i, K in enumerate(order)]
    a_all = torch.cat([c.a1f for c in cases], dim=2).contiguous()
    c_all = torch.cat([c.cadd for c in cases], dim=2).contiguous() if with_cadd else None
    for i, c in enumerate(cases):
        c.xyz, c.cxyz = cases[0].xyz, cases[0].cxyz
        c.a1f_wide, c.a1f_off = a_all, i * C1
        if with_cadd:
            c.cadd_wide, c.cadd_off = c_all, i * C1
        _views(c)
    _PAIRS[key] = cases
    return cases
