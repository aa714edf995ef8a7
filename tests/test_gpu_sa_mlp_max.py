"""GPU: the fused set-abstraction kernel (ext.sa_mlp_max / ext.sa_mlp_max_pair, hotrack_amd/csrc/sa_fused.hip) against a plain
float64 evaluation of its own formula, in every instantiation -- 3 width sets x K in {16, 32, 64} x the four operand modes (six
operand sets: xyz, a1f+xyz, a1f+xyz+cadd and the run-time-tested a1f, a1f+cadd, xyz+cadd) -- with and without b1, in every
output layout, with a1f / cadd / out as column blocks of wider buffers, at the index edges (the last point of the last cloud,
padded ball-query lists, duplicated points, pooled rows that are exactly zero) and the tile and grid edges of the persistent loop
(one centroid, whole tiles only, several rounds under a compute-unit cap with the cursor crossing clouds, a production shape).
Cases, reference and comparison: tests/_sa_cases.py (checked on the CPU by tests/test_sa_cases.py).

Bound: atol 2e-5, rtol 1e-5 against float64, as for the other fp32-MFMA chains of this depth.  Every test prints the largest
|got - ref64| / (atol + rtol |ref64|) it saw; on an MI355X the maxima per width set were

    32-32-64     0.034   (the 54 instantiations 0.016, index edges 0.034, tile and grid edges 0.016)
    64-64-128    0.023   (the 54 instantiations)
    128-128-192  0.062   (the 54 instantiations 0.024, index edges 0.062 -- the forced-bias cases, whose outputs reach 8 --,
                          tile and grid edges 0.029, the production shape 0.035)
    pair kernel  0.031   (both K orders, with and without cadd, on all and on 5 compute units)

(a float32 torch evaluation of the same cases stays below 0.1; a wrong neighbour, centroid or operand is beyond 100)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sa_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(ext, case, kw):
    """One launch in the case's output form -> (B, S, C3) view of what the kernel wrote."""
    C3 = case.widths[2]
    if case.form == "block":
        buf = torch.full((case.B, case.S, C3 + C.OUT_PAD), C.SENTINEL, device="cuda")
        ext.sa_mlp_max(out=buf[:, :, C.OUT_OFF:C.OUT_OFF + C3], **kw)
        keep = torch.ones(C3 + C.OUT_PAD, dtype=torch.bool, device="cuda")
        keep[C.OUT_OFF:C.OUT_OFF + C3] = False
        assert bool((buf[:, :, keep] == C.SENTINEL).all()), f"{case.name}: columns around the output block were written"
        return buf[:, :, C.OUT_OFF:C.OUT_OFF + C3]
    if case.form == "pm":
        out = ext.sa_mlp_max(point_major=True, **kw)
        assert out.shape == (case.B, case.S, C3)
        return out
    out = ext.sa_mlp_max(**kw)
    assert out.shape == (case.B, C3, case.S)
    return out.transpose(1, 2)


def _run(ext, case):
    """Two launches (bit-identical), the comparison with float64 -> (output, worst ratio)."""
    kw = C.kernel_args(case, "cuda")
    got = _launch(ext, case, kw)
    again = _launch(ext, case, kw)
    assert torch.equal(got, again), f"{case.name}: a second launch differs"
    return got, C.compare(got, C.ref64(case), case.name)


@pytest.mark.parametrize("name", C.CASES)
def test_sa_mlp_max_matches_fp64(name):
    from hotrack_amd import ext
    case = C.get_case(name)
    assert ext.sa_mlp_max_supported(case.K, *case.widths)
    got, _ = _run(ext, case)
    if case.b3_kind == "forced":  # pooled rows that are zero everywhere come out as exact zeros
        zero, _ = C.forced_channels(case.widths[2])
        assert bool((got[:, :, zero.cuda()] == 0).all())
    if case.cus:
        # fewer workgroups walk the same tiles, each several of them, the (cloud, tile) cursor crossing clouds
        try:
            ext.sa_set_compute_units(case.cus)
            capped, _ = _run(ext, case)
        finally:
            ext.sa_set_compute_units(0)
        assert torch.equal(capped, got), f"{name}: the output under a cap of {case.cus} compute units differs"


@pytest.mark.parametrize("cus", [0, 5])
@pytest.mark.parametrize("with_cadd", [False, True])
@pytest.mark.parametrize("order", C.PAIR_ORDERS)
def test_sa_mlp_max_pair_matches_fp64(order, with_cadd, cus):
    """Both scales of a keypoint-query module in one launch, in either K order, written into the two halves of one
    (B, J, 2 C3) buffer; uncapped and with both shares running several rounds on 5 compute units."""
    from hotrack_amd import ext
    cases = C.get_pair(order, with_cadd)
    C3 = cases[0].widths[2]
    assert ext._lib.pn2x_sa_mlp_max_pair_supported(order[0], order[1], *cases[0].widths) == 1
    kws = [C.kernel_args(c, "cuda") for c in cases]
    outs = []
    try:
        ext.sa_set_compute_units(cus)
        for _ in range(2):
            buf = torch.full((C.PAIR_B, C.PAIR_J, 2 * C3), C.SENTINEL, device="cuda")
            ext.sa_mlp_max_pair(*(dict(kw, out=buf[:, :, i * C3:(i + 1) * C3]) for i, kw in enumerate(kws)))
            outs.append(buf)
    finally:
        ext.sa_set_compute_units(0)
    assert torch.equal(outs[0], outs[1])
    for i, c in enumerate(cases):
        C.compare(outs[0][:, :, i * C3:(i + 1) * C3], C.ref64(c), f"{c.name}, {cus or 'all'} compute units")
