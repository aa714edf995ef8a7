"""Records SyntheticLBSHand's skinning tables and lbs_forward_from_tables outputs (tests/golden/lbs_tables_plain.npz) as they
were BEFORE the tables interface learnt its optional MANO entries: tests/test_hand_model_mano.py asserts that a plain model's
tables and outputs keep these bits.  Run from the commit that precedes the extension; not part of the suite."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "network"))

from models.hand_model import SyntheticLBSHand, lbs_forward_from_tables  # noqa: E402


def inputs(num_betas):
    """Seeded poses (4, 48), translations (4, 3) and shape codes (4, num_betas) or None, float64."""
    g = torch.Generator().manual_seed(77 + num_betas)
    pose = torch.cat([(torch.rand(4, 3, generator=g, dtype=torch.float64) * 2 - 1) * 2.0,
                      (torch.rand(4, 45, generator=g, dtype=torch.float64) * 2 - 1) * 1.2], dim=1)
    trans = torch.rand(4, 3, generator=g, dtype=torch.float64) - 0.5
    beta = torch.randn(4, num_betas, generator=g, dtype=torch.float64) if num_betas else None
    return pose, trans, beta


def main():
    out = {}
    for D in (0, 10):
        t = SyntheticLBSHand(num_betas=D).skinning_tables()
        out[f"b{D}_keys"] = np.array(sorted(t))
        for k, v in t.items():
            out[f"b{D}_t_{k}"] = v.numpy()
        pose, trans, beta = inputs(D)
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            with torch.no_grad():
                v, kp = lbs_forward_from_tables(t, pose.to(dt), trans.to(dt), None if beta is None else beta.to(dt))
            out[f"b{D}_{name}_verts"], out[f"b{D}_{name}_kp"] = v.numpy(), kp.numpy()
    np.savez_compressed(os.path.join(HERE, "lbs_tables_plain.npz"), **out)


if __name__ == "__main__":
    main()
