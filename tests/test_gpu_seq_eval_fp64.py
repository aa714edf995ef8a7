"""GPU: obj_pose_metrics_kernel and posed_chamfer_kernel (hotrack_amd/csrc/seq_eval.hip) through hotrack_amd.ext, against
float64 from the float32 inputs (tests/_pose_metric_cases.py) in all nine symmetry modes at T in {1, 63, 64, 65, 257}.

  tdiff   within 4 x 2^-24 x tdiff of float64;
  rdiff   inside [acos(min(c + d, 1)), acos(max(c - d, -1))] in degrees, c the float64 cosine and d the derived bound on the
          float32 cosine, widened by the error of the device's acosf and the conversion to degrees; also within that error of
          the float64 acos of the RESTATED float32 cosine (the kernel's sum order in numpy float32);
  flags   exactly the float64 flags;
  tiling  a frame's four outputs are the same bits wherever it lands.

The acosf figure: no accuracy table for the device library's acosf is installed with ROCm (no document under its share/ or
llvm/ trees states one), so it was measured: over this case list, max |rdiff - degrees(acos64(restated float32 cosine))| was
2.18 float32 ulps of the result (MEASURED_ULPS) on the MI355X (acosf, the division by pi and the multiplication by 180 together);
the tests hold the kernel to 4 x that."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pose_metric_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = [tuple(int(v) for v in m) for m in np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))["modes"]]
MEASURED_ULPS = 2.18
ACOS_ULPS = 4 * MEASURED_ULPS
_REF = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def metrics(fr, axis, sym):
    """Through the C entry, with one spare frame behind the inputs and a sentinel row behind the output: the launch writes T rows
    and nothing past them."""
    from hotrack_amd import ext
    T = fr["gR"].shape[0]
    gR, gt, pR, pt = (dev(np.concatenate([fr[k], fr[k][-1:]])) for k in ("gR", "gt", "pR", "pt"))
    out = torch.full((T + 1, 4), -7.0, dtype=torch.float32, device="cuda")
    rc = ext._lib.pn2x_obj_pose_metrics(T, gR.data_ptr(), gt.data_ptr(), pR.data_ptr(), pt.data_ptr(), int(axis), int(sym),
                                        out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    out = out.cpu().numpy()
    assert (out[T] == -7.0).all(), f"T {T}: the row behind the last frame was written"
    return np.ascontiguousarray(out[:T])


def case(axis, sym):
    if (axis, sym) not in _REF:
        fr = P.frames(axis, sym)
        _REF[(axis, sym)] = (fr, P.reference(fr, axis, sym))
    return _REF[(axis, sym)]


@pytest.mark.parametrize("axis,sym", MODES)
def test_pose_metrics_against_fp64(axis, sym):
    from hotrack_amd import ext
    fr, ref = case(axis, sym)
    F = len(fr["kind"])
    canon = None   # the frame list's outputs from the first launch that holds all of it
    for T in P.T_SIZES:
        tiled, idx = P.tile(fr, T)
        got = metrics(tiled, axis, sym)
        assert got.shape == (T, 4) and got.dtype == np.float32
        assert (got.view(np.uint32) == got[idx].view(np.uint32)).all(), f"T {T}: a frame's outputs depend on where it lands"
        if T >= F:
            canon = got[:F].copy() if canon is None else canon
            assert (got.view(np.uint32) == canon[idx].view(np.uint32)).all(), f"T {T}: other bits than the first launch"
        td, deg, flags = got[:, 0].astype(np.float64), got[:, 1].astype(np.float64), got[:, 2:]
        r = {k: v[idx] for k, v in ref.items()}
        assert np.isfinite(got).all()
        assert (np.abs(td - r["td"]) <= 4 * P.U * r["td"]).all(), f"T {T} tdiff"
        zero = r["deg32"] == 0
        e = np.abs(deg - r["deg32"])[~zero] / P.ulps(r["deg32"][~zero])
        if T == 257:
            wrapped = ext.obj_pose_metrics(dev(tiled["gR"]), dev(tiled["gt"]), dev(tiled["pR"]), dev(tiled["pt"]), axis, bool(sym))
            assert (wrapped.cpu().numpy().view(np.uint32) == got.view(np.uint32)).all()   # the Python entry: the same launch
            print(f"mode ({axis},{sym}): max |rdiff - acos64(restated cosine)| {e.max():.2f} ulp (held to {ACOS_ULPS}); "
                  f"max |tdiff - fp64| / tdiff {np.max(np.abs(td - r['td']) / r['td']) / P.U:.2f} u")
        assert (deg[zero] == 0).all()
        assert (e <= ACOS_ULPS).all(), f"T {T}: {e.max()} ulp"
        lo = r["lo"] - ACOS_ULPS * P.ulps(r["lo"])
        hi = r["hi"] + ACOS_ULPS * P.ulps(r["hi"])
        assert ((lo <= deg) & (deg <= hi)).all(), f"T {T} rdiff outside the derived interval"
        assert (flags == r["flags"]).all(), f"T {T} flags"
    kind = fr["kind"]
    assert canon[kind.index("scaled"), 1] == 0.0   # trace > 3 / cosine > 1: the clamp, not NaN
    ident = canon[kind.index("identical"), 1]
    for s in P.HALF_TURNS:
        d = canon[kind.index("flip" + "".join("+" if v > 0 else "-" for v in s)), 1]
        same = (s[axis] > 0 or sym) if 0 <= axis <= 2 else (s in P.FLIPS.get(axis, []))
        assert (d == ident) if same else (d > 179.9), (s, d, ident)   # a float32 trace of -1 +- 1e-7: 179.98 degrees


@pytest.mark.parametrize("axis,sym", MODES)
def test_non_finite_frames_fail_their_flags_and_touch_nothing_else(axis, sym):
    fr, _ = case(axis, sym)
    clean, idx = P.tile(fr, 65)
    k = fr["kind"].index("thr5--")          # both flags 1 when clean
    nan_at, inf_at = int(np.flatnonzero(idx == k)[-1]), int(np.flatnonzero(idx == k)[0])
    assert nan_at >= 26 and inf_at < 26
    want = metrics(clean, axis, sym)
    assert (want[[nan_at, inf_at], 2:] == 1).all()
    bad = {key: v.copy() for key, v in clean.items()}
    bad["pR"][64] = clean["pR"][nan_at]     # the second workgroup's only frame as well
    bad["pt"][64], bad["gt"][64], bad["gR"][64] = clean["pt"][nan_at], clean["gt"][nan_at], clean["gR"][nan_at]
    col = axis if 0 <= axis <= 2 else 1     # an element every mode reads
    for t in (nan_at, 64):
        bad["pR"][t, 1, col] = np.nan
    bad["pt"][inf_at, 2] = np.inf
    ref65 = {key: v.copy() for key, v in bad.items()}
    for key in ref65:                        # the same launch with clean frames in the three places
        ref65[key][[nan_at, inf_at, 64]] = clean[key][nan_at]
    got, ref = metrics(bad, axis, sym), metrics(ref65, axis, sym)
    assert (got[[nan_at, inf_at, 64], 2:] == 0).all(), got[[nan_at, inf_at, 64]]
    assert got[inf_at, 0] == np.inf
    others = np.setdiff1d(np.arange(65), [nan_at, inf_at, 64])
    assert (got[others].view(np.uint32) == ref[others].view(np.uint32)).all()
    assert (ref[[nan_at, inf_at, 64], 2:] == 1).all()


# ---- posed_chamfer -----------------------------------------------------------------------------------------------------------
def chamfer(*args):
    from hotrack_amd import ext
    out = ext.posed_chamfer(*args)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N,M,T", [(1, 1, 3), (512, 513, 2), (513, 512, 2), (511, 8, 1), (2048, 7, 2)])
def test_chamfer_at_the_tile_edges(N, M, T):
    from test_gpu_seq_eval import _case, _chamfer_fp64
    A, B, Ra, ta, Rb, tb = _case(300 + N + M + T, N, M, T)
    got = chamfer(A, B, Ra, ta, Rb, tb)
    want = _chamfer_fp64(A, B, Ra, ta, Rb, tb)
    rel = ((got.double() - want).abs() / want).max().item()
    print(f"N {N} M {M} T {T}: max rel. err vs fp64 {rel:.3g}")
    assert got.shape == (T,) and rel <= 1e-5
    # swapping the clouds: each direction's per-tile partials are the same floats (the same queries, candidates and poses), sa and
    # sb trade places, and sa / N + sb / M is a commutative fp32 addition of the same two quotients: exactly equal
    assert torch.equal(chamfer(B, A, Rb, tb, Ra, ta), got)


def test_chamfer_no_frames_and_one_point_clouds():
    from test_gpu_seq_eval import _case
    A, B, Ra, ta, Rb, tb = _case(9, 5, 4, 2)
    assert chamfer(A, B, Ra[:0], ta[:0], Rb[:0], tb[:0]).shape == (0,)
    # two one-point clouds posed onto the same point: identity / axis-permuting rotations and dyadic numbers, exact in fp32
    a, b = dev(np.array([[1.0, 2.0, 3.0]], np.float32)), dev(np.array([[1.5, 3.0, -2.0]], np.float32))
    eye = np.eye(3, dtype=np.float32)
    rx = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)     # (x, y, z) -> (x, -z, y)
    Ra, ta = dev(np.stack([eye, eye])), dev(np.array([[0.5, 0, 0], [0.25, 0.5, 0.75]], np.float32))
    Rb, tb = dev(np.stack([rx, rx])), dev(np.array([[0, 0, 0], [-0.25, 0.5, 0.75]], np.float32))
    out = chamfer(a, b, Ra, ta, Rb, tb).cpu().numpy()
    assert (out == 0).all(), out
    far = chamfer(a, b, Ra, ta, Rb, dev(np.array([[0, 0, 4.0], [-0.25, 3.5, 4.75]], np.float32))).cpu().numpy()
    assert (far == np.array([8.0, 10.0], np.float32)).all(), far   # |(0,0,4)| and |(0,3,4)| in both directions
