"""The cpu_baseline port (oracle/cpu_reference.py) against the reference's Python fallback operators, as recorded in
tests/golden/cpu_reference_fallback.npz (tests/golden/make_golden_cpu_reference.py: inputs + the imported fallback's outputs)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpu_reference_fallback.npz")


def test_port_equals_reference_fallback():
    from oracle import cpu_reference as P
    z = {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}
    xyz, ref_idx = z["xyz"], z["fps_idx"]
    idx = P.furthest_point_sample(xyz, 64)
    assert torch.equal(idx.long(), ref_idx)
    new = torch.gather(xyz, 1, ref_idx.unsqueeze(-1).expand(-1, -1, 3))
    assert torch.equal(P.ball_query(0.2, 16, xyz, new).long(), z["ball_r02_k16"])
    d, i = P.three_nn(xyz, new)
    assert torch.equal(i.long(), z["nn_idx"]) and torch.equal(d, z["nn_dist"])
    d, i = P.knn(8, new[:, :21].contiguous(), xyz)
    assert torch.equal(i.long(), z["knn8_idx"]) and torch.allclose(d, z["knn8_dist"], equal_nan=True)
    f, gi = z["f"], z["group_idx"]
    assert torch.equal(P.grouping_operation(f, gi), z["group"])
    assert torch.equal(P.gather_operation(f, gi[:, :, 0]), z["gather"])
    assert torch.allclose(P.three_interpolate(f, z["interp_idx"], z["interp_w"]), z["interp"])
