"""CPU: the mesh -> signed-distance path at the edge cases of tests/_mesh_edge_cases.py -- first the float64 oracle itself, where a
closed form or a bracket is known (slivers, the box with sliver faces, queries on and in the planes of the box), then the torch
route (network/models/mesh_sdf.py::signed_distance_torch) on every case at the cases' tolerances."""
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
from models import mesh_sdf  # noqa: E402

SLIVER_GROUPS = [(s, r) for s in EC.SLIVER_SHAPES for r in EC.SLIVER_RATIOS]
SLIVER_IDS = [f"{s}-{r:g}" for s, r in SLIVER_GROUPS]


def _torch_route(c):
    d, w = mesh_sdf.signed_distance_torch(torch.from_numpy(c.queries.copy()), torch.from_numpy(c.verts.copy()),
                                          torch.from_numpy(c.faces.copy()), return_winding=True)
    return d.numpy(), w.numpy()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ratio", SLIVER_GROUPS, ids=SLIVER_IDS)
def test_oracle_on_slivers_lies_between_the_edges_and_the_height(shape, ratio):
    """A triangle's closest point is at most its smallest altitude away from its nearest edge point.  The bracket is held to
    1e-10 m: the oracle's normal is a float64 cross product whose direction is good to 1.1e-16 / sin(angle), 1.1e-10 at
    height / base = 1e-6, times a query at most 0.3 m from the vertex: 3e-11 m in the distance to the plane."""
    low, high, slack = 0.0, 0.0, 1e-10
    for name in EC.sliver_names(shape, ratio):
        c = EC.case(name)
        d = np.abs(EC.reference(name)[0])
        d_edges, h = EC.edge_distance(c), EC.sliver_height(c)
        low, high = max(low, float((d_edges - h - d).max())), max(high, float((d - d_edges).max()))
    print(f"oracle, {shape} {ratio:g}: at most {high:.3e} m above the edge distance, {low:.3e} m below edge distance - height")
    assert high <= slack and low <= slack


@pytest.mark.parametrize("name", ["box_with_slivers", "coplanar_box"])
def test_oracle_equals_the_box_closed_form(name):
    err = float(np.abs(EC.reference(name)[0] - MC.box_sdf(EC.case(name).queries)).max())
    print(f"float64 oracle vs the box closed form, {name}: {err:.3e}")
    assert err <= 1e-12


def test_oracle_is_zero_on_the_surface():
    c = EC.case("contact_box")
    assert float(np.abs(MC.box_sdf(c.queries)).max()) <= 1e-12  # the queries are on the box
    for name in EC.CONTACT:
        worst = float(np.abs(EC.reference(name)[0]).max())
        print(f"float64 oracle, {name}: max |d| = {worst:.3e}")
        assert worst <= EC.tol(EC.case(name))  # (midpoints and centroids are rounded to fp32: within 4e-9 m of the surface)
    assert float(np.abs(EC.reference("contact_box")[0] - MC.box_sdf(c.queries)).max()) <= 1e-12


@pytest.mark.parametrize("name", EC.SIGNED)
def test_oracle_leaves_few_queries_out_of_the_sign_check(name):
    c = EC.case(name)
    d, w = EC.reference(name)
    near = float((np.abs(d) < MC.SIGN_MIN).mean())
    print(f"{name}: {near:.3%} of the queries nearer than {MC.SIGN_MIN} m")
    assert near <= MC.SIGN_SKIP_MAX
    if "open" in c.checks:
        half = float((np.abs(w - 0.5) < EC.OPEN_WN_MARGIN).mean())
        print(f"{name}: {half:.3%} of the queries within {EC.OPEN_WN_MARGIN} of winding 0.5")
        assert half <= MC.SIGN_SKIP_MAX
    assert (~EC.sign_mask(c, d, w)).mean() <= MC.SIGN_SKIP_MAX


def test_oracle_winding_numbers_of_the_topologies():
    d, w = EC.reference("nested_boxes")
    inner = MC.box_sdf(EC.case("nested_boxes").queries) < -MC.SIGN_MIN
    assert inner.any() and np.abs(w[inner] - 2.0).max() <= 1e-9 and (d[inner] < 0).all()
    d, w = EC.reference("box_reversed")
    assert np.abs(w[inner] + 1.0).max() <= 1e-9 and (d > 0).all()  # negative iff winding > 0.5: an inverted mesh has no inside
    w = EC.reference("box_open")[1]
    assert ((w > 0.05) & (w < 0.95)).any()


# ---- the torch route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ratio", SLIVER_GROUPS, ids=SLIVER_IDS)
def test_torch_route_on_slivers(shape, ratio):
    worst, failed = 0.0, []
    for name in EC.sliver_names(shape, ratio):
        c = EC.case(name)
        d, w = _torch_route(c)
        worst = max(worst, EC.magnitude_error(c, d))
        try:
            EC.check(c, d, w, label="torch route")
        except AssertionError as e:
            failed.append(str(e))
    print(f"torch route, {shape} {ratio:g}: max | |d| - |oracle| | over the orders and offsets = {worst:.3e} m")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("name", EC.MESH_CASES + EC.VOLUMES)
def test_torch_route_on_mesh_cases(name):
    c = EC.case(name)
    d, w = _torch_route(c)
    EC.check(c, d, w, label="torch route")


@pytest.mark.parametrize("name", EC.VOLUMES)
def test_mesh_to_volume_cpu(name):
    c = EC.case(name)
    res, stride = c.volume
    v, f = torch.from_numpy(c.verts.copy()), torch.from_numpy(c.faces.copy())
    vol32 = mesh_sdf.mesh_to_volume(v, f, res, stride, clamp=0.1, dtype=torch.float32)
    assert vol32.shape == (res, res, res) and vol32.dtype == torch.float32
    d = mesh_sdf.signed_distance_torch(torch.from_numpy(c.queries.copy()), v, f)
    assert torch.equal(vol32.reshape(-1).view(torch.int32), d.clamp(-0.1, 0.1).view(torch.int32))  # the point route on grid(res, stride)
    vol16 = mesh_sdf.mesh_to_volume(v, f, res, stride, clamp=0.1, dtype=torch.float16).numpy().reshape(-1)
    d_ref = EC.reference(name)[0]
    want = np.clip(d_ref, -0.1, 0.1).astype(np.float16)
    far = np.abs(d_ref) >= MC.SIGN_MIN
    ulps = np.abs(vol16.view(np.int16).astype(np.int32) - want.view(np.int16).astype(np.int32))[far]  # equal signs: ordered bits
    print(f"torch route, {name} fp16: at most {int(ulps.max())} ulp from the rounded oracle")
    assert ((vol16 < 0) == (want < 0))[far].all() and int(ulps.max()) <= 1
