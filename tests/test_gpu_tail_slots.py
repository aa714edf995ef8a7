"""GPU: pn2x_add_layernorm_perm (hotrack_amd/csrc/tail.hip) with the slot count as a compile-time value (re = 5: every load of
a row in flight at once) and as a run-time value (every other re, and pn2x_add_layernorm_perm_any_slots at re = 5).

Against float64 at the bound of tests/test_gpu_tail_perm.py (atol = rtol = 2e-5), over the widths at which the entry changes its
instance (c <= 128, <= 256, <= 512, above; each with a partly filled last 64-channel group), re = 1, 5, 6, row counts that are no
multiple of the four rows of a workgroup (B * 21 with B = 1, 3, and j = 5), ldz > re * c with NaN in the columns past re * c
(never to be read), with and without bias and the second LayerNorm, a table with repeated and identity entries.

Same bits: both kernels add ((((0 + z_0) + z_1) + ..) + z_4) + bias, so at re = 5 the two entries must agree with torch.equal;
and tests/golden/tail_slots_parent.npz holds what the kernel before this change (commit ca6fb1e) returned for inputs made of
exact integer arithmetic (tests/golden/make_golden_tail_slots.py), which both entries must still return bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = -12345.0
PAD = 8
CS = (4, 128, 132, 384, 512, 516)
RES = (1, 5, 6)
EPS1, EPS2 = 1e-5, 1e-6


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def table(j, re):
    """(j, re) int32: slot 0 the token itself, slot 1 the token again (a repeat), then token 0, the last token, and strides."""
    cols = [[t, t, 0, j - 1][r] if r < 4 else (7 * t + r) % j for t in range(j) for r in range(re)]
    return torch.tensor(cols, dtype=torch.int32).view(j, re)


def exact_inputs(B, j, re, c, pad):
    """Inputs that every machine forms with the same bits: multiples of 1/512 from integer arithmetic.  z (B*j, re*c + pad) with NaN
    in the pad columns, bias, and the two LayerNorms' (weight, bias), all float32 on the CPU."""
    def grid(n, m, a, b, mod):
        i = np.arange(n, dtype=np.int64)[:, None]
        k = np.arange(m, dtype=np.int64)[None, :]
        return torch.from_numpy((((i * a + k * b + (i * k) % 13) % mod - mod // 2) / 512.0).astype(np.float32))
    z = torch.full((B * j, re * c + pad), float("nan"))
    z[:, :re * c] = grid(B * j, re * c, 7919, 104729, 2003)
    bias = grid(1, c, 1, 31, 1021)[0]
    aff = [grid(1, c, 1, a, 1531)[0] for a in (17, 29, 43, 59)]
    return z, bias, aff


def _run(ext, entry, B, j, re, c, z, perm, bias, aff, use_ln2):
    """One launch of `entry` into a buffer with two sentinel rows behind the last token; returns the (B*j, c) result."""
    out = torch.full((B * j + 2, c), SENTINEL, device="cuda")
    g1, b1, g2, b2 = aff
    with torch.cuda.device(0):
        rc = getattr(ext._lib, entry)(B, j, re, c, _p(z), z.stride(0), _p(perm), _p(bias), _p(g1), _p(b1), EPS1,
                                      _p(g2 if use_ln2 else None), _p(b2 if use_ln2 else None), EPS2 if use_ln2 else 0.0, _p(out), None)
    assert rc == 0
    assert bool((out[B * j:] == SENTINEL).all()), "rows past the last token were written"
    return out[:B * j]


def _ref64(z, perm, B, j, re, c, bias, aff, use_ln2):
    z3 = z[:, :re * c].double().view(B, j, re * c)
    u = sum(z3[:, perm[:, r].long(), r * c:(r + 1) * c] for r in range(re)).reshape(B * j, c)
    if bias is not None:
        u = u + bias.double()
    u = F.layer_norm(u, (c,), aff[0].double(), aff[1].double(), EPS1)
    return F.layer_norm(u, (c,), aff[2].double(), aff[3].double(), EPS2) if use_ln2 else u


@pytest.mark.parametrize("re", RES)
@pytest.mark.parametrize("c", CS)
def test_add_layernorm_perm_matches_fp64(c, re):
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(1000 * re + c)
    worst = 0.0
    for B, j in ((1, 21), (3, 21), (2, 5)):
        perm = table(j, re)
        for pad in (0, PAD):
            z = torch.full((B * j, re * c + pad), float("nan"))
            z[:, :re * c] = torch.randn(B * j, re * c, generator=g) * 1.3 + 0.45
            bias = torch.randn(c, generator=g)
            aff = [torch.randn(c, generator=g) for _ in range(4)]
            dz, dbias, daff = z.cuda(), bias.cuda(), [a.cuda() for a in aff]
            for use_ln2 in (False, True):
                for use_bias in (False, True):
                    ref = _ref64(z, perm, B, j, re, c, bias if use_bias else None, aff, use_ln2)
                    got = _run(ext, "pn2x_add_layernorm_perm", B, j, re, c, dz, perm, dbias if use_bias else None, daff, use_ln2)
                    got = got.cpu().double()
                    assert bool(torch.isfinite(got).all()), f"c={c} re={re} B={B} j={j} pad={pad}: a pad column was read"
                    r = float(((got - ref).abs() / (2e-5 + 2e-5 * ref.abs())).max())
                    worst = max(worst, r)
                    assert r <= 1.0, (f"c={c} re={re} B={B} j={j} pad={pad} ln2={use_ln2} bias={use_bias}: {r:.3g} times the bound "
                                      "atol = rtol = 2e-5")
    print(f"add_layernorm_perm c={c} re={re}: worst |got - ref64| / (2e-5 + 2e-5 |ref64|) = {worst:.4f}")


@pytest.mark.parametrize("c", CS)
def test_compile_time_and_run_time_slots_give_the_same_bits(c):
    from hotrack_amd import ext
    re = 5
    g = torch.Generator().manual_seed(77 + c)
    for B, j in ((3, 21), (2, 5)):
        perm = table(j, re)
        z = torch.full((B * j, re * c + PAD), float("nan"))
        z[:, :re * c] = torch.randn(B * j, re * c, generator=g) * 1.3 + 0.45
        z[0, :re * c:3] = -0.0  # signed zeros keep their sign through 0 + z_0 in both
        dz, dbias = z.cuda(), torch.randn(c, generator=g).cuda()
        daff = [torch.randn(c, generator=g).cuda() for _ in range(4)]
        for use_ln2 in (False, True):
            for bias in (None, dbias):
                fast = _run(ext, "pn2x_add_layernorm_perm", B, j, re, c, dz, perm, bias, daff, use_ln2)
                slow = _run(ext, "pn2x_add_layernorm_perm_any_slots", B, j, re, c, dz, perm, bias, daff, use_ln2)
                assert bool(torch.isfinite(fast).all())
                assert torch.equal(fast, slow), (c, B, j, use_ln2, bias is not None, float((fast - slow).abs().max()))
        # the binding's switch reaches the same two entries
        lns = [torch.nn.LayerNorm(c, eps=eps).cuda().requires_grad_(False) for eps in (EPS1, EPS2)]
        with torch.no_grad():
            for ln, (w, b) in zip(lns, (daff[:2], daff[2:])):
                ln.weight.copy_(w)
                ln.bias.copy_(b)
        for fixed in (True, False):
            via = ext.add_layernorm_perm(dz[:, :re * c], perm, lns[0], bias=dbias, ln2=lns[1], fixed_slots=fixed)
            assert torch.equal(via, fast)


def test_both_entries_return_the_bits_of_the_kernel_before_this_change():
    from hotrack_amd import ext
    rec = np.load(os.path.join(G, "tail_slots_parent.npz"))
    B, j, re, c, pad = (int(rec[k]) for k in ("B", "j", "re", "c", "pad"))
    z, bias, aff = exact_inputs(B, j, re, c, pad)
    perm = table(j, re)
    dz, dbias, daff = z.cuda(), bias.cuda(), [a.cuda() for a in aff]
    for use_ln2 in (False, True):
        for use_bias in (False, True):
            want = torch.from_numpy(rec[f"out_ln2{int(use_ln2)}_bias{int(use_bias)}"])
            for entry in ("pn2x_add_layernorm_perm", "pn2x_add_layernorm_perm_any_slots"):
                got = _run(ext, entry, B, j, re, c, dz, perm, dbias if use_bias else None, daff, use_ln2).cpu()
                assert torch.equal(got, want), (entry, use_ln2, use_bias, float((got - want).abs().max()))
