"""Generates tests/golden/hand_shape_opt.npz from the IMPORTED reference's gf_optimize_hand_shape (optimization_hand.py:30-124).
RUNS ONLY IN THE BUILD CONTAINER (needs the reference checkout); tests and the GPU box only read the .npz.

The reference class is created with object.__new__ (its __init__ loads a MANO layer: licensed assets) and given exactly the
attributes its methods read: CPU device, this repository's SyntheticLBSHand(num_betas=10) as `mano_layer_right`, seeded
particles.  The model's forward is wrapped to record the shape codes of every call, which give per iteration the current
estimate (row 0 of the pre-sampled particles is zero) and the search size the iteration sampled with (least squares over the
other rows, in float64).  No reference file is touched or copied.

Cases (P = particles):
  m1_768     one call (mode 1), targets from a shaped hand plus keypoint noise;
  m3_768_*   three calls with use_old=True (mode 3): T = 1, 2, 3 rows of target lengths;
  fail_768   targets from the zero shape exactly: every iteration takes the failure branch, the shape stays zero;
  m1_5120    one call at the reference's particle count."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_hand import _load  # noqa: E402
from make_golden_sdf import import_reference  # noqa: E402

D = 10
BETA_TRUE = np.array([1.2, -0.8, 0.5, 1.5, -1.1, 0.3, -0.6, 0.9, -1.4, 0.7], np.float32)


def particles(P, seed):
    g = torch.Generator().manual_seed(seed)
    pre = torch.randn(P, D, generator=g)
    pre[0] = 0
    return pre


def make_ref(oh, hand, pre):
    o = object.__new__(oh.gf_optimize_hand_shape)
    o.optimize_dim, o.particle_size, o.iteration, o.beta = D, pre.shape[0], 20, 0.9
    o.device, o.scaling_coefficient2 = "cpu", 2000
    o.initial_scale = torch.ones(D) * 5
    o.mano_layer_right = hand
    o.pre_sampled_particle = pre.clone()
    return o


class Recorder:
    def __init__(self, hand):
        self.hand, self.calls = hand, []
        self.orig = hand.forward

    def __enter__(self):
        def fwd(*a, **k):
            self.calls.append(k["th_betas"].detach().clone())
            return self.orig(*a, **k)
        self.hand.forward = fwd
        return self

    def __exit__(self, *exc):
        del self.hand.forward


def recover(calls, pre):
    """(iterations, D) current estimate and (iterations, D) search size of every iteration from the recorded shape codes."""
    pre64 = pre.double()
    h = torch.stack([c[0] for c in calls]).double()
    s = torch.stack([((c.double() - c[0].double()) * pre64).sum(0) / (pre64 ** 2).sum(0) for c in calls])
    return h.numpy(), s.numpy()


def main():
    _, oh = import_reference()
    SyntheticLBSHand = _load("hand_model").SyntheticLBSHand
    hand = SyntheticLBSHand(num_betas=D)
    rng = np.random.default_rng(3)
    zero_pose = torch.zeros(1, 48)
    with torch.no_grad():
        _, kp_true = hand.forward(th_pose_coeffs=zero_pose, th_trans=torch.zeros(1, 3), th_betas=torch.from_numpy(BETA_TRUE)[None])
        _, kp_zero = hand.forward(th_pose_coeffs=zero_pose, th_trans=torch.zeros(1, 3), th_betas=torch.zeros(1, D))
    noisy = lambda: (kp_true + torch.from_numpy(rng.normal(0, 0.001, (1, 21, 3)).astype(np.float32))).float()
    pres = {768: particles(768, 11), 5120: particles(5120, 12)}
    out = {"beta_true": BETA_TRUE, "pre_768": pres[768].numpy(), "pre_5120": pres[5120].numpy(),
           "params": np.array([20, 0.9, 2000, 5.0])}
    report = {}

    def run(name, o, kp, use_old):
        with Recorder(hand) as rec, torch.no_grad():
            res = o.optimize(kp, use_old=use_old) if use_old else o.optimize(kp)
        h, s = recover(rec.calls, o.pre_sampled_particle)
        out[f"{name}_pred_kp"] = kp.numpy()
        out[f"{name}_shape"] = res.detach().clone().numpy().reshape(-1)
        out[f"{name}_h"], out[f"{name}_search"] = h.astype(np.float32), s.astype(np.float32)
        report[name] = {"targets": int(o.old_pred_length.shape[1]), "shape": out[f"{name}_shape"].round(4).tolist()}

    run("m1_768", make_ref(oh, hand, pres[768]), noisy(), False)
    o3 = make_ref(oh, hand, pres[768])
    for i in range(3):
        run(f"m3_768_{i}", o3, noisy(), True)
    run("fail_768", make_ref(oh, hand, pres[768]), kp_zero.clone(), False)
    run("m1_5120", make_ref(oh, hand, pres[5120]), noisy(), False)
    np.savez_compressed(os.path.join(HERE, "hand_shape_opt.npz"), **out)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
