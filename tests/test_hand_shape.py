"""The hand model's shape space (network/models/hand_model.py) and the torch route of the hand shape-code search
(gf_optimize_hand_shape, network/models/optimization_hand.py) against the IMPORTED reference driving the same hand model
(tests/golden/hand_shape_opt.npz, made by tests/golden/make_golden_shape.py).  CPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))
G = os.path.join(ROOT, "tests", "golden")

from models.hand_model import SyntheticLBSHand  # noqa: E402
from models.optimization_hand import gf_optimize_hand_shape, kp2length  # noqa: E402


def test_zero_shape_is_bitwise_the_shapeless_hand():
    a, b = SyntheticLBSHand(), SyntheticLBSHand(num_betas=10)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    g = torch.Generator().manual_seed(0)
    pose, trans = torch.randn(6, 48, generator=g) * 0.3, torch.randn(6, 3, generator=g)
    va, ka = a(th_pose_coeffs=pose, th_trans=trans)
    for kw in ({}, {"th_betas": torch.zeros(6, 10)}, {"th_betas": torch.zeros(1, 10)}, {"use_registed_beta": True}):
        vb, kb = b(th_pose_coeffs=pose, th_trans=trans, **kw)
        assert torch.equal(va, vb) and torch.equal(ka, kb), kw
    # a model without a shape space ignores a registered shape and has no basis
    a.register_beta(torch.ones(1, 10))
    assert torch.equal(a(th_pose_coeffs=pose, th_trans=trans, use_registed_beta=True)[1], ka)
    assert a.shape_keypoint_basis(torch.zeros(1, 48)) is None


def test_registered_shape_is_applied():
    b = SyntheticLBSHand(num_betas=10)
    beta = torch.linspace(-1, 1, 10)[None]
    pose = torch.zeros(2, 48)
    b.register_beta(beta)
    _, k1 = b(th_pose_coeffs=pose, use_registed_beta=True)
    _, k2 = b(th_pose_coeffs=pose, th_betas=beta.expand(2, -1))
    assert torch.equal(k1, k2)
    assert (k1 - b(th_pose_coeffs=pose)[1]).abs().max() > 1e-3


@pytest.mark.parametrize("posed", [False, True])
def test_shape_keypoint_basis_reproduces_forward(posed):
    hm = SyntheticLBSHand(num_betas=10)
    g = torch.Generator().manual_seed(1)
    pose = torch.randn(1, 48, generator=g) * 0.3 if posed else torch.zeros(1, 48)
    K0, K = hm.shape_keypoint_basis(pose)
    assert K0.shape == (21, 3) and K.shape == (10, 21, 3)
    assert hm.shape_keypoint_basis(pose)[0] is K0  # cached
    beta = (torch.rand(8, 10, generator=g, dtype=torch.float64) * 2 - 1) * 20
    _, kp = hm(th_pose_coeffs=pose.double().expand(8, -1), th_betas=beta)
    pred = K0.double() + torch.einsum("rd,dkc->rkc", beta, K.double())
    assert float((pred - kp).abs().max()) < 1e-6


def test_shape_keypoint_basis_rejects_a_non_affine_model():
    class Curved(SyntheticLBSHand):
        def forward(self, th_pose_coeffs, th_betas=None, **kw):
            v, k = super().forward(th_pose_coeffs, th_betas=th_betas, **kw)
            if th_betas is not None:
                k = k + 1e-4 * (th_betas ** 2).sum(-1)[:, None, None]
            return v, k

    assert Curved(num_betas=10).shape_keypoint_basis(torch.zeros(1, 48)) is None


def test_bone_length_jacobian_has_full_rank():
    hm = SyntheticLBSHand(num_betas=10)
    f = lambda b: kp2length(hm(th_pose_coeffs=torch.zeros(1, 48, dtype=torch.float64), th_betas=b[None])[1])[0]
    J = torch.autograd.functional.jacobian(f, torch.zeros(10, dtype=torch.float64))
    assert J.shape == (15, 10)
    sv = torch.linalg.svdvals(J)
    assert int(torch.linalg.matrix_rank(J)) == 10 and float(sv[-1] / sv[0]) > 0.05


CALLS = [("m1_768", 768, None), ("m3_768", 768, 3), ("fail_768", 768, None), ("m1_5120", 5120, None)]


@pytest.mark.parametrize("name,P,history", CALLS, ids=[c[0] for c in CALLS])
def test_torch_route_matches_the_reference(name, P, history):
    g = np.load(os.path.join(G, "hand_shape_opt.npz"))
    hm = SyntheticLBSHand(num_betas=10)
    opt = gf_optimize_hand_shape({"device": "cpu"}, hand_model=hm, particle_size=P)
    opt.pre_sampled_particle = torch.from_numpy(g[f"pre_{P}"])
    opt.keep_trace = True
    assert not opt.use_kernel()
    keys = [f"{name}_{i}" for i in range(history)] if history else [name]
    for i, key in enumerate(keys):
        with torch.no_grad():
            shape = opt.optimize(torch.from_numpy(g[f"{key}_pred_kp"]), use_old=history is not None)
        assert shape.shape == (1, 10) and opt.old_pred_length.shape == (1, i + 1, 15)
        np.testing.assert_allclose(shape.numpy()[0], g[f"{key}_shape"], rtol=0, atol=1e-5)
        # the search size each iteration sampled with = the previous iteration's updated search size
        np.testing.assert_allclose(opt.trace[:-1, 3:].numpy(), g[f"{key}_search"][1:], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(g[f"{key}_search"][0], 5.0, rtol=1e-6)
        if name == "fail_768":
            assert torch.equal(shape, torch.zeros(1, 10)) and not opt.trace[:, 2].any()
        else:
            assert opt.trace[:, 2].any()
