"""GPU: ext.hand_frame (hotrack_amd/csrc/kabsch.hip: hand_frame_kernel -- the palm fit plus the canonicalisation of the cloud and the
keypoints, one workgroup per cloud) beyond its one (16, 1024, num = 6) test: point counts around the 256-thread stride and zero,
1 to 16 palm points picked in no particular order, shared and per-cloud templates, the second copy into a wider row buffer, the
per-cloud non-finite flag, and the calls it must reject.

The fit is held to the float64 SVD (_kabsch_ref of test_gpu_fused.py) at 2e-6, as in the existing test; the transform is compared
with the float64 canonicalisation (p - t) R / scale of the KERNEL'S OWN R and t, at 2e-6 max(1, |ref|max): that separates the fit
from the transform."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fused import _kabsch_ref  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE = 0.2
SENTINEL = -7.0


def _rotations(g, B):
    q = torch.randn(B, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).view(B, 3, 3)


def _frames(B, N, J, num, shared, seed):
    """A palm template (1 | B, num, 3), keypoints whose palm_idx rows are a rigid motion of it plus 2 mm of noise, a cloud
    around the hand.  palm_idx: `num` of the J keypoints in no particular order.  CPU float32."""
    g = torch.Generator().manual_seed(seed)
    tmpl = torch.randn(1 if shared else B, num, 3, generator=g) * 0.05
    Rgt = _rotations(g, B)
    trans = torch.randn(B, 1, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.5])
    palm_idx = torch.randperm(J, generator=g)[:num]
    if num > 1:
        while bool((palm_idx[1:] > palm_idx[:-1]).all()):  # not a monotone selection
            palm_idx = palm_idx[torch.randperm(num, generator=g)]
    kp = torch.randn(B, J, 3, generator=g) * 0.08 + trans
    kp[:, palm_idx] = tmpl.expand(B, -1, -1) @ Rgt.transpose(1, 2) + trans + 0.002 * torch.randn(B, num, 3, generator=g)
    pts = torch.randn(B, N, 3, generator=g) * 0.1 + trans
    return tmpl.contiguous(), kp.contiguous(), palm_idx.int(), pts.contiguous()


def _canon64(p, R, t):
    """(p - t) R / scale in float64: p (B, M, 3), R (B,3,3), t (B,3,1) as the kernel returned them."""
    s = float(torch.tensor(SCALE, dtype=torch.float32))
    return (p.double() - t.double().transpose(1, 2)) @ R.double() / s


def _check(tmpl, kp, palm_idx, pts, R, t, xyz2, xyz1, what):
    B, N, J = pts.shape[0], pts.shape[1], kp.shape[1]
    assert R.shape == (B, 3, 3) and t.shape == (B, 3, 1) and xyz2.shape == (B, N, 3) and xyz1.shape == (B, J, 3)
    R, t, xyz2, xyz1 = R.cpu(), t.cpu(), xyz2.cpu(), xyz1.cpu()
    Rr, tr = _kabsch_ref(tmpl.expand(B, -1, -1), kp[:, palm_idx.long()])
    eR, et = float((R - Rr).abs().max()), float((t - tr).abs().max())
    print(f"{what}: |R - svd| {eR:.2e}, |t - svd| {et:.2e}")
    assert eR <= 2e-6 and et <= 2e-6, (what, eR, et)
    assert float((torch.det(R.double()) - 1).abs().max()) <= 1e-5
    for name, got, src in (("xyz2", xyz2, pts), ("xyz1", xyz1, kp)):
        if src.shape[1] == 0:
            continue
        ref = _canon64(src, R, t)
        err, bound = float((got.double() - ref).abs().max()), 2e-6 * max(1.0, float(ref.abs().max()))
        print(f"{what}: {name} |diff| {err:.2e} of {bound:.2e}")
        assert err <= bound, (what, name, err, bound)


SHAPES = [(1, 1, 21, 6, True), (3, 0, 21, 6, True), (5, 255, 21, 6, False), (5, 256, 21, 6, True), (5, 257, 21, 3, False),
          (70, 1024, 21, 16, False), (2, 1000, 5, 4, True)]


@pytest.mark.parametrize("B,N,J,num,shared", SHAPES)
def test_hand_frame_shapes_match_fp64(B, N, J, num, shared):
    from hotrack_amd import ext
    tmpl, kp, palm_idx, pts = _frames(B, N, J, num, shared, seed=B * 1000 + N + num)
    assert tmpl.shape[0] == (1 if shared else B) and len(set(palm_idx.tolist())) == num
    R, t, xyz2, xyz1 = ext.hand_frame(tmpl.cuda(), kp.cuda(), palm_idx.cuda(), pts.cuda(), SCALE)
    _check(tmpl, kp, palm_idx, pts, R, t, xyz2, xyz1, f"B={B} N={N} J={J} num={num} shared={shared}")
    # the same fit as ext.kabsch on the gathered palm points, bit for bit (one solver)
    R2, t2 = ext.kabsch(tmpl.cuda(), kp[:, palm_idx.long()].contiguous().cuda())
    assert torch.equal(R2, R) and torch.equal(t2, t)


@pytest.mark.parametrize("width,col", [(132, 5), (3, 0)])
def test_xyz2_copy_fills_its_columns_and_nothing_else(width, col):
    from hotrack_amd import ext
    B, N = 5, 257
    tmpl, kp, palm_idx, pts = _frames(B, N, 21, 6, False, seed=31)
    buf = torch.full((B, N, width), SENTINEL, device="cuda")
    R, t, xyz2, xyz1 = ext.hand_frame(tmpl.cuda(), kp.cuda(), palm_idx.cuda(), pts.cuda(), SCALE, xyz2_copy=buf[:, :, col:col + 3])
    _check(tmpl, kp, palm_idx, pts, R, t, xyz2, xyz1, f"copy into columns [{col}:{col + 3}) of {width}")
    assert torch.equal(buf[:, :, col:col + 3], xyz2)
    keep = torch.ones(width, dtype=torch.bool, device="cuda")
    keep[col:col + 3] = False
    assert bool((buf[:, :, keep] == SENTINEL).all())
    plain = ext.hand_frame(tmpl.cuda(), kp.cuda(), palm_idx.cuda(), pts.cuda(), SCALE)
    assert all(torch.equal(a, b) for a, b in zip(plain, (R, t, xyz2, xyz1)))


def test_nonfinite_flags_only_the_bad_clouds():
    from hotrack_amd import ext
    B, N = 6, 300
    tmpl, kp, palm_idx, pts = _frames(B, N, 21, 6, False, seed=47)
    not_palm = next(k for k in range(21) if k not in palm_idx.tolist())
    clean_kp, clean_pts = kp.clone(), pts.clone()
    pts[1, 123, 1] = float("nan")                       # one point of cloud 1
    kp[3, not_palm, 2] = float("inf")                   # a keypoint of cloud 3 the fit does not use
    kp[4, int(palm_idx[2]), 0] = float("nan")           # a keypoint of cloud 4 the fit does use
    flags = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    R, t, xyz2, xyz1 = ext.hand_frame(tmpl.cuda(), kp.cuda(), palm_idx.cuda(), pts.cuda(), SCALE, nonfinite=flags)
    assert flags.dtype == torch.int32 and flags.tolist() == [0, 1, 0, 1, 1, 0]
    good = torch.tensor([0, 2, 5])
    alone = ext.hand_frame(tmpl[good].contiguous().cuda(), clean_kp[good].contiguous().cuda(), palm_idx.cuda(), clean_pts[good].contiguous().cuda(), SCALE)
    for name, a, b in zip(("R", "t", "xyz2", "xyz1"), (R, t, xyz2, xyz1), alone):
        assert torch.equal(a[good.cuda()], b), name
    # cloud 1: one bad point, the fit and every other output are those of the clean cloud
    ok = torch.ones(N, dtype=torch.bool)
    ok[123] = False
    assert bool(torch.isfinite(R[1]).all()) and bool(torch.isfinite(t[1]).all()) and bool(torch.isfinite(xyz1[1]).all())
    assert bool(torch.isfinite(xyz2[1][ok.cuda()]).all()) and not bool(torch.isfinite(xyz2[1, 123]).all())
    one = ext.hand_frame(tmpl[1:2].contiguous().cuda(), clean_kp[1:2].contiguous().cuda(), palm_idx.cuda(), clean_pts[1:2].contiguous().cuda(), SCALE)
    assert torch.equal(R[1:2], one[0]) and torch.equal(t[1:2], one[1]) and torch.equal(xyz1[1:2], one[3])
    assert torch.equal(xyz2[1][ok.cuda()], one[2][0][ok.cuda()])
    # cloud 3: the fit does not see the bad keypoint
    assert bool(torch.isfinite(R[3]).all()) and bool(torch.isfinite(t[3]).all()) and bool(torch.isfinite(xyz2[3]).all())
    assert not bool(torch.isfinite(xyz1[3, not_palm]).all())
    # without the flag argument the outputs are the same
    again = ext.hand_frame(tmpl.cuda(), kp.cuda(), palm_idx.cuda(), pts.cuda(), SCALE)
    for a, b in zip((R, t, xyz2, xyz1), again):
        assert torch.equal(torch.nan_to_num(a, 1e9, 2e9, -2e9), torch.nan_to_num(b, 1e9, 2e9, -2e9))


def test_rejected_calls_raise_and_leave_no_error_pending():
    from hotrack_amd import ext
    from hotrack_amd.pointnet2_hip import Pn2Error
    B, N = 5, 64
    tmpl, kp, palm_idx, pts = _frames(B, N, 21, 6, True, seed=59)
    dev = [x.cuda() for x in (tmpl, kp, palm_idx, pts)]
    t17, _, idx17, _ = _frames(B, N, 21, 17, True, seed=60)
    with pytest.raises(Pn2Error):                                   # more palm points than the kernel's LDS array holds
        ext.hand_frame(t17.cuda(), dev[1], idx17.cuda(), dev[3], SCALE)
    with pytest.raises(Pn2Error):
        ext.hand_frame(*dev, 0.0)
    with pytest.raises(Pn2Error):                                   # a template batch that is neither 1 nor B
        ext.hand_frame(tmpl.expand(2, -1, -1).contiguous().cuda(), dev[1], dev[2], dev[3], SCALE)
    wide = torch.full((B, N + 1, 8), SENTINEL, device="cuda")
    with pytest.raises(ValueError):                                 # rows of cloud b + 1 do not follow those of cloud b
        ext.hand_frame(*dev, SCALE, xyz2_copy=wide[:, :N, 0:3])
    assert bool((wide == SENTINEL).all())
    R, t, xyz2, xyz1 = ext.hand_frame(*dev, SCALE)                   # a valid call afterwards succeeds
    torch.cuda.synchronize()
    _check(tmpl, kp, palm_idx, pts, R, t, xyz2, xyz1, "after the rejected calls")
