"""GPU: the seven launches of hotrack_amd/csrc/iknet.hip, through hotrack_amd.ext.iknet_forward with closed-form folded weights
(tests/_iknet_kernel_cases.py), against exact expectations and float64.

  routing      every layer an exact selection: raw_quat and kp_hf equal the float32 restatement of the pack bit for bit, which
               pins the pack layout, the parent table, the indexing of all seven launches and the hidden layers' offsets;
  padding      1e30 in the weight's two padded columns changes nothing: the kernel's own zeros stand there;
  biases       a zero layer delivers relu(bias) exactly, for b1 and each bh[l];
  rows         a dense 16-row forward equals every prefix, every row alone and a run on a work buffer of 0xFF bytes, bitwise;
  one dense    one dense layer among routing layers against float64 with the a-priori bound (K + 2) 2^-24 (sum |w x| + |b|);
  head         raw_quat == bo bit for bit, theta against float64 at 4 x the float32 restatement's own error per group."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _iknet_kernel_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
_DEV = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def weights(key, build):
    """One device copy per weight set and module run."""
    if key not in _DEV:
        w = build()
        w = w[0] if isinstance(w, tuple) else w
        _DEV[key] = {k: dev(v) for k, v in w.items()}
    return _DEV[key]


def forward(w, kp, R, t, camera=False):
    from hotrack_amd import ext
    raw, theta, hf = ext.iknet_forward(dev(kp), dev(R), dev(t), w["w1"], w["b1"], w["wh"], w["bh"], w["wo"], w["bo"], camera=camera)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), theta.cpu().numpy(), hf.cpu().numpy()


def forward_raw_entry(w, kp, R, t, work):
    """Straight through the C entry, with the caller's work buffer."""
    from hotrack_amd import ext
    M = kp.shape[0]
    k, r, tt = dev(kp), dev(R), dev(t)
    raw = torch.empty((M, 60), dtype=torch.float32, device="cuda")
    theta = torch.empty((M, 45), dtype=torch.float32, device="cuda")
    hf = torch.empty((M, 3, 21), dtype=torch.float32, device="cuda")
    rc = ext._lib.pn2x_iknet_forward(M, 0, k.data_ptr(), r.data_ptr(), tt.data_ptr(), w["w1"].data_ptr(), w["b1"].data_ptr(),
                                     w["wh"].data_ptr(), w["bh"].data_ptr(), w["wo"].data_ptr(), w["bo"].data_ptr(), work.data_ptr(),
                                     hf.data_ptr(), raw.data_ptr(), theta.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return raw.cpu().numpy(), theta.cpu().numpy(), hf.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("M", [1, 7, 16])
def test_routing_is_exact(M, camera):
    kp, R, t = C.keypoints(M, 10 + M)
    pack = C.pack_fp32(kp, R, t, camera)
    for s in range(3):
        raw, _, hf = forward(weights(("route", s), lambda: C.routing(s)), kp, R, t, camera)
        want = C.routing_expected(pack, s)
        bad = np.argwhere(raw != want)
        assert bad.size == 0, f"set {s}: first wrong (row, output) {bad[0]}, column {C.column_set(s)[bad[0][1]]}"
        assert (hf.reshape(M, 63) == pack[:, :63]).all()


def test_padded_columns_hold_the_kernels_own_zeros():
    kp, R, t = C.keypoints(16, 5)
    w = weights(("route", 1), lambda: C.routing(1))
    base = forward(w, kp, R, t)
    big = dict(w)
    big["w1"] = w["w1"].clone()
    big["w1"][:, 126:128] = 1e30
    got = forward(big, kp, R, t)
    for a, b in zip(base, got):
        assert (bits(a) == bits(b)).all()
    assert (base[0] == C.routing_expected(C.pack_fp32(kp, R, t, False), 1)).all()


@pytest.mark.parametrize("p", range(6))
def test_bias_offsets_are_exact(p):
    kp, R, t = C.keypoints(7, 20 + p)
    built = C.bias_case(p)
    raw, _, _ = forward({k: dev(v) for k, v in built[0].items()}, kp, R, t)
    assert (raw == built[1][None]).all(), np.argwhere(raw != built[1][None])[:4]


def test_rows_are_independent_bitwise():
    from hotrack_amd import ext
    kp, R, t = C.keypoints(16, 30)
    w = weights("he", C.he_state)
    full = forward(w, kp, R, t)
    assert np.isfinite(full[0]).all() and np.abs(full[0]).max() > 0.1
    for M in range(1, 17):
        part = forward(w, kp[:M], R[:M], t[:M])
        for a, b in zip(full, part):
            assert (bits(a[:M]) == bits(b)).all(), f"prefix {M}"
        one = forward(w, kp[M - 1:M], R[M - 1:M], t[M - 1:M])
        for a, b in zip(full, one):
            assert (bits(a[M - 1:M]) == bits(b)).all(), f"row {M - 1} alone"
    floats = int(ext._lib.pn2x_iknet_work_floats())
    assert floats == 32768
    work = torch.full((4 * floats,), 255, dtype=torch.uint8, device="cuda")
    dirty = forward_raw_entry(w, kp, R, t, work)
    for a, b in zip(full, dirty):
        assert (bits(a) == bits(b)).all()


@pytest.mark.parametrize("p", range(7))
def test_one_dense_layer_against_fp64(p):
    """|got - relu(fp64)| <= (K + 2) 2^-24 (sum |w x| + |b|) per output: K products and K - 1 additions in some order, the bias
    addition; the inputs of the dense layer are exact fp32 values because every other layer routes.  Derived, not measured."""
    kp, R, t = C.keypoints(16, 4)
    pack = C.pack_fp32(kp, R, t, False)
    w, ref, bound, ratio = C.dense_case(p, pack)
    raw, _, _ = forward({k: dev(v) for k, v in w.items()}, kp, R, t)
    err = np.abs(raw.astype(np.float64) - ref)
    hard = (ratio >= 1e3) & (ref != 0)
    print(f"position {p}: max err / bound {np.max(err / bound):.3f}; cancelling outputs {int(hard.sum())}, their worst relative error "
          f"{np.max(err[hard] / np.abs(ref[hard])):.3g}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:4]
    assert hard.sum() >= 15


def test_head_conversion_per_group():
    table, groups = C.quat_table()
    tol = C.head_tolerances()
    want = C.theta_fp64(table)
    w = C._zero_set()
    _route = C.routing(0)[0]   # live activations under the zero head weight
    for k in ("w1", "wh"):
        w[k] = _route[k]
    wd = {k: dev(v) for k, v in w.items()}
    worst = {nm: 0.0 for nm in groups}
    for row in range(16):
        M = row + 1
        kp, R, t = C.keypoints(M, 40 + row)
        wd["bo"] = dev(table[row].reshape(60))
        raw, theta, _ = forward(wd, kp, R, t)
        assert (bits(raw) == bits(np.broadcast_to(table[row].reshape(1, 60), (M, 60)))).all()
        assert np.isfinite(theta).all()
        assert (bits(theta) == bits(np.broadcast_to(theta[:1], (M, 45)))).all()   # the same quaternion in every row
        got = theta[0].reshape(15, 3).astype(np.float64)
        for nm, mask in groups.items():
            j = mask[row]
            if not j.any():
                continue
            err = float(np.abs(got[j] - want[row][j]).max())
            worst[nm] = max(worst[nm], err)
            if tol[nm] == 0.0:
                assert (got[j] == want[row][j]).all(), (nm, row)
            else:
                assert err <= tol[nm], (nm, row, err, tol[nm])
    for nm in groups:
        print(f"{nm:14s} worst |theta - fp64| {worst[nm]:.3e}  tolerance {tol[nm]:.3e}")
    assert (want[groups["identity"]] == 0).all()
