"""Closed-form IKNet parameters for tests/golden/make_golden_iknet.py and the IKNet tests: integer-hash lattices, exact in
float32 on every machine, no RNG stream (the 21.7 MB of weights are recomputed, not committed)."""
import numpy as np


def lattice(shape, salt: int, lo: float, hi: float) -> np.ndarray:
    """Values in [lo, hi] on a 10007-point grid, scrambled by a quadratic integer hash of the flat index."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    h = (i * 2654435761 + salt * 40503 + ((i * i) % 65521) * 97) % 10007
    return (lo + (hi - lo) * (h.astype(np.float64) / 10006.0)).astype(np.float32).reshape(shape)


def iknet_state(layers: int = 6, width: int = 1024, d_in: int = 126, d_out: int = 60) -> dict:
    """{state_dict key: float32 array} of an IKNet: He-scaled weights, small biases and non-trivial BatchNorm statistics."""
    sd, last = {}, d_in
    for i in range(layers):
        s = (6.0 / last) ** 0.5
        sd[f"linear.{i}.weight"] = lattice((width, last), 10 * i + 1, -s, s)
        sd[f"linear.{i}.bias"] = lattice((width,), 10 * i + 2, -0.05, 0.05)
        sd[f"bn.{i}.weight"] = lattice((width,), 10 * i + 3, 0.8, 1.2)
        sd[f"bn.{i}.bias"] = lattice((width,), 10 * i + 4, -0.1, 0.1)
        sd[f"bn.{i}.running_mean"] = lattice((width,), 10 * i + 5, -0.2, 0.2)
        sd[f"bn.{i}.running_var"] = lattice((width,), 10 * i + 6, 0.5, 1.5)
        last = width
    s = (3.0 / width) ** 0.5
    sd[f"linear.{layers}.weight"] = lattice((d_out, width), 101, -s, s)
    sd[f"linear.{layers}.bias"] = lattice((d_out,), 102, -0.1, 0.1) + np.tile(np.array([0.5, 0, 0, 0], np.float32), d_out // 4)
    return sd


def load_into(model) -> None:
    """Copies iknet_state() into an IKNet-shaped torch module (num_batches_tracked left as it is)."""
    import torch
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in iknet_state().items():
            sd[k].copy_(torch.from_numpy(v))
