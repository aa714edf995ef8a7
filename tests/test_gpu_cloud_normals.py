"""GPU: ext.cloud_normals (hotrack_amd/csrc/cloud_normals.hip) against numpy in fp64 (tests/_cloud_normals_ref.py): neighbour
sets by fp64 distance with a stable sort, covariance centred in fp64, numpy.linalg.eigh.  Directions are compared by the norm of
the cross product with the reference normal, `variation` absolutely.

Tolerances: 4 x the worst figure of an fp32 numpy restatement of the kernel's arithmetic (two-pass covariance, trace scaling,
five cyclic Jacobi sweeps) against the fp64 reference over the very clouds of CASES, measured here on the CPU before anything
is compared -- the kernel differs from the restatement in the order of its sums and in nothing else.  A query is left out of the
direction comparison only when its fp64 eigengap (l1 - l0) / l2 is below 0.05 or its k-th and (k+1)-th fp64 distances agree to
1e-6 relative; at most 5 % of a case's usable queries, asserted."""
import numpy as np
import pytest
import torch

import _cloud_normals_ref as R

pytestmark = pytest.mark.gpu


def _run(points, k, orient="none", valid=None, viewpoint=None):
    from hotrack_amd import ext
    dev = torch.device("cuda", 0)
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid)).to(dev)
    w = None if viewpoint is None else torch.from_numpy(np.asarray(viewpoint, np.float32)).to(dev)
    n, var = ext.cloud_normals(torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev), k=k, viewpoint=w, valid=v, orient=orient)
    return n.cpu().numpy(), var.cpu().numpy()


@pytest.fixture(scope="module")
def references():
    """Every case's clouds and fp64 reference, computed once, and the two tolerances."""
    refs = {case: R.case_reference(case) for case in R.CASES + R.VARIATION_CASES}
    worst_cross = max(refs[case][2] for case in R.CASES)
    worst_var = max(v[3] for v in refs.values())
    print("fp32 restatement vs fp64 over CASES: worst cross-norm %.3e, worst |variation error| %.3e" % (worst_cross, worst_var))
    assert 0 < worst_cross < 1e-5 and 0 < worst_var < 1e-5   # (the restatement itself is sound)
    return refs, 4 * worst_cross, 4 * worst_var


def _check(got_n, got_v, ref, tol_n, tol_v, what, directions=True):
    ok, cmp = ref["usable"], ref["compare"]
    assert np.isfinite(got_n).all() and np.isfinite(got_v).all(), what
    if not directions:
        cmp = np.zeros_like(cmp)
    excluded = 1 - cmp.sum() / max(ok.sum(), 1)
    assert excluded <= R.MAX_EXCLUDED or not directions, f"{what}: {excluded:.3f} of the usable queries left out"
    lens = np.linalg.norm(got_n.astype(np.float64), axis=1)
    live = np.linalg.norm(ref["normal"], axis=1) > 0
    assert np.abs(lens[live] - 1).max(initial=0) < 1e-6 and (got_n[~live] == 0).all() and (got_v[~live] == 0).all(), what
    cross = R.cross_norm(got_n[cmp], ref["normal"][cmp]).max(initial=0)
    dv = np.abs(got_v.astype(np.float64) - ref["variation"])[ok].max(initial=0)
    print(f"{what}: cross-norm {cross:.3e} (tol {tol_n:.3e}), variation {dv:.3e} (tol {tol_v:.3e}), excluded {excluded:.4f}")
    assert cross <= tol_n, what
    assert dv <= tol_v, what


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "N%d-k%d-B%d" % c[:3])
def test_normals_and_variation_against_fp64(references, case):
    refs, tol_n, tol_v = references
    clouds, ref, _, _ = refs[case]
    got_n, got_v = _run(clouds, case[1])
    assert got_n.shape == clouds.shape and got_v.shape == clouds.shape[:2]
    for b in range(clouds.shape[0]):
        _check(got_n[b], got_v[b], ref[b], tol_n, tol_v, f"case {case} cloud {b}")


@pytest.mark.parametrize("case", R.VARIATION_CASES, ids=lambda c: "N%d-k%d-B%d" % c[:3])
def test_variation_of_three_point_neighbourhoods(references, case):
    """k = 3 among more than 64 points: `variation`, zeros and unit length on every usable query (no direction comparison: 40 %
    of these triangles are slivers)."""
    refs, tol_n, tol_v = references
    clouds, ref, _, _ = refs[case]
    got_n, got_v = _run(clouds, case[1])
    for b in range(clouds.shape[0]):
        _check(got_n[b], got_v[b], ref[b], tol_n, tol_v, f"case {case} cloud {b}", directions=False)


def test_exact_plane(references):
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(8), indexing="ij"), -1).reshape(-1, 2) * 0.01
    pts = np.concatenate([g + rng.uniform(-0.003, 0.003, g.shape), np.zeros((128, 1))], 1).astype(np.float32)
    n, v = _run(pts[None], 30)
    assert np.abs(n[0, :, :2]).max() <= references[1] and np.abs(np.abs(n[0, :, 2]) - 1).max() < 1e-6
    assert np.abs(v).max() <= references[2]


def test_mask_equals_the_compacted_cloud(references):
    refs, tol_n, tol_v = references
    pts = R.capsule_half(77, 257, 5e-4)
    valid = np.random.default_rng(78).random(257) >= 0.4
    n, v = _run(pts[None], 30, valid=valid[None])
    nc, vc = _run(pts[valid][None], 30)
    assert np.array_equal(n[0][valid].view(np.int32), nc[0].view(np.int32)) and np.array_equal(v[0][valid].view(np.int32), vc[0].view(np.int32))
    assert (n[0][~valid] == 0).all() and (v[0][~valid] == 0).all()
    _check(n[0], v[0], R.normals_fp64(pts, 30, valid), tol_n, tol_v, "masked cloud")   # uint8 mask: the same
    n8, v8 = _run(pts[None], 30, valid=valid[None].astype(np.uint8))
    assert np.array_equal(n8, n) and np.array_equal(v8, v)


def test_two_valid_points_give_zeros():
    pts = R.capsule_half(3, 64)
    valid = np.zeros(64, bool)
    valid[[5, 40]] = True
    n, v = _run(pts[None], 8, valid=valid[None])
    assert (n == 0).all() and (v == 0).all()


def test_non_finite_rows_count_as_masked(references):
    refs, tol_n, tol_v = references
    pts = R.capsule_half(11, 257, 5e-4)
    bad = np.zeros(257, bool)
    bad[[0, 17, 100, 256]] = True
    dirty = pts.copy()
    dirty[0, 0], dirty[17, 1], dirty[100, 2], dirty[256] = np.nan, np.inf, -np.inf, np.nan
    n, v = _run(dirty[None], 30)
    nm, vm = _run(pts[None], 30, valid=~bad[None])
    assert np.isfinite(n).all() and np.isfinite(v).all()
    assert np.array_equal(n.view(np.int32), nm.view(np.int32)) and np.array_equal(v.view(np.int32), vm.view(np.int32))
    assert (n[0][bad] == 0).all() and (v[0][bad] == 0).all()
    _check(n[0], v[0], R.normals_fp64(dirty, 30), tol_n, tol_v, "cloud with NaN / inf rows")


def test_identical_points_give_zeros():
    pts = np.tile(np.array([[0.01, -0.02, 0.5]], np.float32), (65, 1))
    n, v = _run(pts[None], 30)
    assert (n == 0).all() and (v == 0).all()


@pytest.mark.parametrize("mode", ["none", "view", "reference"])
def test_orientation(references, mode):
    refs, tol_n, _ = references
    pts = R.capsule_half(21, 257, 5e-4)
    view = np.array([[0.02, -0.01, 0.0]], np.float32)
    ref = R.normals_fp64(pts, 30)
    cmp = ref["compare"]
    n = _run(pts[None], 30, orient=mode, viewpoint=view)[0][0].astype(np.float64)
    want = R.orient_numpy(ref["normal"], pts, view[0], mode)
    w = view[0].astype(np.float64) - pts.astype(np.float64)
    if mode == "view":
        assert ((n * w).sum(1)[cmp] >= 0).all()
    elif mode == "reference":
        nz = (n != 0) & cmp[:, None]
        assert (np.sign(n[nz]) == np.sign(w[nz])).all()
    else:
        assert (n[np.arange(257), np.argmax(np.abs(n), 1)][cmp] > 0).all()
    # the sign rule decides on a quantity that may sit at zero (a component, or the dot product): compare where the fp64 rule
    # is decided by more than the tolerance
    dec = np.abs(ref["normal"] * w).min(1) > tol_n if mode == "reference" else (
        np.abs((ref["normal"] * w).sum(1)) > tol_n if mode == "view" else
        np.sort(np.abs(ref["normal"]), 1)[:, 2] - np.sort(np.abs(ref["normal"]), 1)[:, 1] > tol_n)
    sel = cmp & dec
    assert sel.sum() > 0.9 * 257
    if mode != "reference":   # (the reference's rule leaves the line of n: its components are compared below)
        assert R.cross_norm(n[sel], ref["normal"][sel]).max() <= tol_n
    assert np.abs(n[sel] - want[sel]).max() <= tol_n   # the same signs, every component within the direction tolerance
    # default viewpoint: the origin
    if mode == "view":
        a = _run(pts[None], 30, orient="view")[0]
        b = _run(pts[None], 30, orient="view", viewpoint=np.zeros((1, 3), np.float32))[0]
        assert np.array_equal(a, b)


def test_range_is_refused_in_words():
    from hotrack_amd import ext
    dev = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="3 to 2048 points"):
        ext.cloud_normals(torch.zeros((1, 2049, 3), device=dev))
    for k in (2, 65):
        with pytest.raises(ValueError, match="3 to 64 neighbours"):
            ext.cloud_normals(torch.zeros((1, 100, 3), device=dev), k=k)


def test_two_calls_give_the_same_bits():
    pts = R.case_clouds((1024, 30, 1, 1e-3))
    a, b = _run(pts, 30, orient="view"), _run(pts, 30, orient="view")
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
