"""CPU: SyntheticManoHand (a hand with MANO's structure: pose blend shapes, mean pose, regressed joints, vertex fingertips, root
centring) and the optional entries of HandModel.skinning_tables() / lbs_forward_from_tables that describe it -- and that a
plain hand's tables and outputs kept their bits (tests/golden/lbs_tables_plain.npz, recorded before the entries existed by
tests/golden/make_golden_lbs_tables.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), os.path.join(ROOT, "tests", "golden"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from models.hand_model import HandModel, SyntheticLBSHand, SyntheticManoHand, lbs_forward_from_tables  # noqa: E402

MANO_ENTRIES = ("posedirs", "pose_mean", "kp_vertex", "centre_root")
_MODELS = {}


def _mano(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _MODELS:
        _MODELS[key] = SyntheticManoHand(**kw)
    return _MODELS[key]


def _poses(n, seed, angle=1.5):
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    pose = torch.cat([(torch.rand(n, 3, generator=g, dtype=f64) * 2 - 1) * 2.0, (torch.rand(n, 45, generator=g, dtype=f64) * 2 - 1) * angle], 1)
    return pose, torch.rand(n, 3, generator=g, dtype=f64) - 0.5, torch.randn(n, 10, generator=g, dtype=f64) * 2


def test_the_model_has_manos_structure():
    m = _mano()
    assert (m.num_verts, m.num_pose, m.num_betas) == (778, 45, 10)
    assert tuple(m.th_v_template.shape) == (778, 3) and tuple(m.th_shapedirs.shape) == (778, 3, 10)
    assert tuple(m.th_posedirs.shape) == (778, 3, 135) and tuple(m.th_comps.shape) == (45, 45)
    J = m.th_J_regressor
    assert tuple(J.shape) == (16, 778) and bool((J >= 0).all()) and torch.allclose(J.sum(dim=1), torch.ones(16), atol=1e-6)
    W = m.th_weights
    assert tuple(W.shape) == (778, 16) and int((W > 0).sum(dim=1).max()) <= 4 and torch.allclose(W.sum(dim=1), torch.ones(778), atol=1e-6)
    assert float(m.th_hands_mean.abs().max()) > 0 and len(m.tip_vertices) == 5
    assert sorted(m.contact_zones) == [1, 2, 3, 4, 5] and all(len(z) > 0 for z in m.contact_zones.values())
    # three levels under the wrist, five fingers
    depth = [0] * 16
    for j in range(1, 16):
        depth[j] = depth[m.PARENTS[j]] + 1
    assert sorted(depth) == [0] + [1] * 5 + [2] * 5 + [3] * 5
    assert SyntheticManoHand(num_verts=97, weights_per_vertex=1).skinning_tables()["skin_idx"].shape == (97, 1)


def test_keypoints_are_root_centred_and_tips_are_vertices():
    m = _mano()
    pose, trans, beta = _poses(3, 5)
    with torch.no_grad():
        verts, kp = m(pose, th_betas=beta, th_trans=trans)
    assert float((kp[:, 0] - trans).abs().max()) < 1e-12                      # the root sits at the translation
    for slot, j in enumerate((4, 8, 12, 16, 20)):                             # thumb, index, middle, ring, pinky
        assert torch.equal(kp[:, j], verts[:, m.tip_vertices[slot]])


def test_pose_blend_shapes_reach_millimetres():
    m = _mano()
    pose, trans, _ = _poses(6, 6)
    without = SyntheticManoHand()
    without.th_posedirs.zero_()
    with torch.no_grad():
        d = (m(pose, th_trans=trans)[0] - without(pose, th_trans=trans)[0]).norm(dim=-1)
    print(f"pose blend shapes move vertices by up to {float(d.max()) * 1e3:.2f} mm (mean {float(d.mean()) * 1e3:.2f} mm)")
    assert 1e-3 < float(d.max()) < 3e-2


def test_tables_carry_the_mano_entries():
    t = _mano().skinning_tables()
    assert t is not None and all(k in t for k in MANO_ENTRIES)
    assert tuple(t["posedirs"].shape) == (778, 3, 135) and tuple(t["pose_mean"].shape) == (45,)
    assert t["kp_vertex"].dtype == torch.long and t["centre_root"] is True
    kpv = t["kp_vertex"].tolist()
    assert [j for j, v in enumerate(kpv) if v >= 0] == [4, 8, 12, 16, 20]     # keypoint order: the tip closes each finger
    taken = {4, 8, 12, 16, 20}
    assert not taken & set(t["parents"].tolist()) and not taken & set(t["skin_idx"].flatten().tolist())
    assert all(int(t["pose_block"][j]) == -1 for j in taken) and sorted(b for b in t["pose_block"].tolist() if b >= 0) == list(range(15))
    assert t["skin_idx"].shape[1] <= 4 and all(int(t["parents"][j]) < j for j in range(1, 21))


@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("registered", [False, True])
def test_tables_reproduce_forward(with_beta, registered):
    m = SyntheticManoHand()
    t = m.skinning_tables()
    pose, trans, beta = _poses(5, 11 + 2 * with_beta + registered)
    b = beta[:1] if registered else beta
    with torch.no_grad():
        if registered:
            m.register_beta(b if with_beta else torch.zeros(1, 10, dtype=torch.float64))
            want = m(pose.clone(), th_trans=trans, use_registed_beta=True)
        else:
            want = m(pose.clone(), th_betas=b if with_beta else None, th_trans=trans)
        got = lbs_forward_from_tables(t, pose, trans, b if with_beta else None)
    dv, dk = float((want[0].double() - got[0]).abs().max()), float((want[1].double() - got[1]).abs().max())
    print(f"beta {with_beta}, registered {registered}: tables vs forward: vertices {dv:.2e} m, keypoints {dk:.2e} m")
    assert want[0].dtype == torch.float64 and dv <= HandModel.TABLES_TOL and dk <= HandModel.TABLES_TOL


def test_a_claim_without_the_pose_blend_shapes_is_refused():
    """Only the CLAIM loses the term: forward() keeps it, and the check must see the difference."""

    class Claim(SyntheticManoHand):
        def _lbs_tables(self):
            t = super()._lbs_tables()
            t["posedirs"] = torch.zeros_like(t["posedirs"])
            return t

    assert Claim().skinning_tables() is None and _mano().skinning_tables() is not None


@pytest.mark.parametrize("entry", ["pose_mean", "kp_vertex", "centre_root"])
def test_a_claim_without_another_entry_is_refused(entry):
    class Claim(SyntheticManoHand):
        def _lbs_tables(self):
            t = super()._lbs_tables()
            del t[entry]
            return t

    assert Claim().skinning_tables() is None


@pytest.mark.parametrize("D", [0, 10])
def test_a_plain_hand_keeps_its_bits(D):
    from make_golden_lbs_tables import inputs
    g = np.load(os.path.join(ROOT, "tests", "golden", "lbs_tables_plain.npz"))
    t = SyntheticLBSHand(num_betas=D).skinning_tables()
    assert sorted(t) == g[f"b{D}_keys"].tolist() and not any(k in t for k in MANO_ENTRIES)
    for k, v in t.items():
        want = torch.from_numpy(g[f"b{D}_t_{k}"])
        assert v.dtype == want.dtype and torch.equal(v, want), k
    pose, trans, beta = inputs(D)
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        with torch.no_grad():
            v, kp = lbs_forward_from_tables(t, pose.to(dt), trans.to(dt), None if beta is None else beta.to(dt))
        assert torch.equal(v, torch.from_numpy(g[f"b{D}_{name}_verts"])) and torch.equal(kp, torch.from_numpy(g[f"b{D}_{name}_kp"]))


def test_shape_keypoint_basis_holds():
    m = _mano()
    pose, _, _ = _poses(1, 21, angle=0.8)
    basis = m.shape_keypoint_basis(pose)
    assert basis is not None
    K0, K = (x.double() for x in basis)
    g = torch.Generator().manual_seed(3)
    for scale in (1.0, 3.0, 10.0):
        beta = torch.randn(1, 10, generator=g, dtype=torch.float64) * scale
        with torch.no_grad():
            _, kp = m(pose, th_betas=beta)
        # the basis is handed out in float32: its own rounding of 0.1 m keypoints and of K, times |beta|
        assert float((K0 + torch.einsum("d,dkc->kc", beta[0], K) - kp[0]).abs().max()) <= 1e-6


def test_hand_model_option_parses():
    import argparse

    import parse_args
    from models.hand_model import named_hand_model
    parser = argparse.ArgumentParser()
    parse_args.add_args(parser)
    args = parser.parse_args(["--hand_model", "synthetic_mano"])
    assert args.hand_model == "synthetic_mano" and isinstance(named_hand_model(args.hand_model), SyntheticManoHand)
    with pytest.raises(ValueError):
        named_hand_model("mano")
