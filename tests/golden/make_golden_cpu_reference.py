"""Generates tests/golden/cpu_reference_fallback.npz: the reference's Python fallback operators
(network/models/pointnet_utils.py, CUDA=False branch), IMPORTED from a reference checkout, on seeded inputs.
tests/test_cpu_reference.py checks the cpu_baseline port (oracle/cpu_reference.py) against these vectors.

    python tests/golden/make_golden_cpu_reference.py <reference checkout>

Stored: every input the test feeds both implementations and every output of the reference.  No reference file is
touched or copied.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/: _cases
from _cases import cloud  # noqa: E402

OUT = os.path.join(HERE, "cpu_reference_fallback.npz")


def main(ref):
    sys.path[:0] = [ref, os.path.join(ref, "network"), os.path.join(ref, "network", "models")]
    ref_pu = __import__("pointnet_utils")
    assert os.path.abspath(ref_pu.__file__).startswith(os.path.abspath(ref)) and ref_pu.CUDA is False
    torch.manual_seed(0)
    xyz = torch.from_numpy(cloud(1, 2, 512, "hand"))
    orig = torch.randint
    torch.randint = lambda lo, hi, size, **kw: torch.zeros(size, dtype=torch.long)  # the fallback's random start -> 0 (CUDA)
    try:
        fps_idx = ref_pu.farthest_point_sample(xyz, 64)
    finally:
        torch.randint = orig
    new = torch.gather(xyz, 1, fps_idx.unsqueeze(-1).expand(-1, -1, 3))
    nn_d, nn_i = ref_pu.three_nn(xyz, new)
    knn_d, knn_i = ref_pu.knn_point(8, new[:, :21].contiguous(), xyz)
    f = torch.randn(2, 7, 512)
    gi = torch.randint(0, 512, (2, 9, 4))
    w = torch.rand(2, 64, 3)
    ii = torch.randint(0, 512, (2, 64, 3))
    out = {"xyz": xyz, "fps_idx": fps_idx, "ball_r02_k16": ref_pu.query_ball_point(0.2, 16, xyz, new),
           "nn_dist": nn_d, "nn_idx": nn_i, "knn8_dist": knn_d, "knn8_idx": knn_i,
           "f": f, "group_idx": gi, "group": ref_pu.group_operation(f, gi), "gather": ref_pu.gather_operation(f, gi[:, :, 0]),
           "interp_w": w, "interp_idx": ii, "interp": ref_pu.three_interpolate(f, ii, w)}
    np.savez_compressed(OUT, **{k: v.numpy() for k, v in out.items()})
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
