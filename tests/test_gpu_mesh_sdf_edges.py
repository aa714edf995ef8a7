"""GPU: the mesh -> signed-distance kernels (hotrack_amd/csrc/mesh_sdf.hip: sdf.mesh_signed_distance, sdf.mesh_sdf_volume) at the
edge cases of tests/_mesh_edge_cases.py -- slivers, placement and scale, contact and coplanar queries, topologies and launch
shapes -- at the tolerances the CPU tests (tests/test_mesh_sdf_edges.py) hold the torch route to; run-to-run and face-order
bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mesh_cases as MC  # noqa: E402
import _mesh_edge_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
SLIVER_GROUPS = [(s, r) for s in EC.SLIVER_SHAPES for r in EC.SLIVER_RATIOS]
SLIVER_IDS = [f"{s}-{r:g}" for s, r in SLIVER_GROUPS]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _kernel(c, faces=None):
    """-> (d, winding) tensors of the point entry on the case; asserts that a second run is bitwise equal."""
    from hotrack_amd import sdf
    q, v = torch.from_numpy(c.queries.copy()).cuda(), torch.from_numpy(c.verts.copy()).cuda()
    f = torch.from_numpy(np.ascontiguousarray(c.faces if faces is None else faces)).cuda()
    d, w = sdf.mesh_signed_distance(q, v, f, return_winding=True)
    d2, w2 = sdf.mesh_signed_distance(q, v, f, return_winding=True)
    assert torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(w), _bits(w2)), f"{c.name}: two runs differ"
    return d, w


@pytest.mark.parametrize("shape,ratio", SLIVER_GROUPS, ids=SLIVER_IDS)
def test_kernel_on_slivers(shape, ratio):
    worst, failed = 0.0, []
    for name in EC.sliver_names(shape, ratio):
        c = EC.case(name)
        d, w = _kernel(c)
        worst = max(worst, EC.magnitude_error(c, d.cpu().numpy()))
        try:
            EC.check(c, d.cpu().numpy(), w.cpu().numpy(), label="kernel")
        except AssertionError as e:
            failed.append(str(e))
    print(f"kernel, {shape} {ratio:g}: max | |d| - |oracle| | over the orders and offsets = {worst:.3e} m")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("name", EC.MESH_CASES)
def test_kernel_on_mesh_cases(name):
    c = EC.case(name)
    d, w = _kernel(c)
    EC.check(c, d.cpu().numpy(), w.cpu().numpy(), label="kernel")


@pytest.mark.parametrize("name", EC.VOLUMES)
def test_volume_entry(name):
    from hotrack_amd import sdf
    c = EC.case(name)
    res, stride = c.volume
    v, f = torch.from_numpy(c.verts.copy()).cuda(), torch.from_numpy(c.faces.copy()).cuda()
    d, _ = _kernel(c)
    d_ref = EC.reference(name)[0]
    far = np.abs(d_ref) >= MC.SIGN_MIN
    want = np.clip(d_ref, -0.1, 0.1)
    for dtype in (torch.float32, torch.float16):
        vol = sdf.mesh_sdf_volume(v, f, res, stride, 0.1, dtype)
        assert vol.shape == (res, res, res) and vol.dtype == dtype
        # the point entry on grid(res, stride), bit for bit, before clamping and rounding; and two runs are bitwise equal
        assert torch.equal(_bits(vol.reshape(-1)), _bits(d.clamp(-0.1, 0.1).to(dtype)))
        assert torch.equal(_bits(vol), _bits(sdf.mesh_sdf_volume(v, f, res, stride, 0.1, dtype)))
        got = vol.cpu().numpy().reshape(-1)
        assert np.isfinite(got).all() and float(np.abs(got).max()) <= float(np.float32(0.1))
        if "sign" in c.checks:
            assert (~far).mean() <= MC.SIGN_SKIP_MAX and ((got < 0) == (want < 0))[far].all()
        if dtype == torch.float32:
            err = float(np.abs(np.abs(got.astype(np.float64)) - np.abs(want)).max())
            print(f"kernel, {name} fp32: max | |d| - |oracle| | = {err:.3e} m (bound {EC.tol(c):.3e})")
            assert err <= EC.tol(c)
        else:
            want16 = want.astype(np.float16)
            same = (got < 0) == (want16 < 0)  # equal signs: ordered bits
            ulps = np.abs(got.view(np.int16).astype(np.int32) - want16.view(np.int16).astype(np.int32))[same]
            print(f"kernel, {name} fp16: at most {int(ulps.max())} ulp from the rounded oracle")
            assert same[far].all() and int(ulps.max()) <= 1 and float(np.abs(got[~same]).max(initial=0.0)) <= MC.SIGN_MIN


def test_face_order_inside_a_chunk_changes_no_distance_bit():
    c = EC.case("box_with_slivers")
    d, w = _kernel(c)
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(len(c.faces))
        d2, w2 = _kernel(c, c.faces[perm])
        assert torch.equal(_bits(d), _bits(d2))
        assert float((w - w2).abs().max()) <= 1e-5  # the angles are summed in face order
