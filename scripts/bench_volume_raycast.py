"""Times hotrack_amd.sdf.volume_raycast (hotrack_amd/csrc/sdf_raycast.hip) against network/models/volume_render.volume_raycast_torch on
the same GPU, with scripts/bench_tsdf_fuse.py's protocol and poses: res 128 and 201, the synthetic sequences' fp16
volume, 480 x 640, F = 1 and 10 frames, with and without normals; 3 warm-up calls, then the median (min .. max) of 20 event-timed
calls per route.  Also prints the time to write the outputs once at the measured HBM copy rate (6.29 TB/s), the average march steps
per hit ray (counted by the torch route) and the comparison launch's time.  No per-kernel profile is taken: the figures are
event-timed calls, launch overhead included.

    python scripts/bench_volume_raycast.py [--out profiles/volume_raycast_bench.json] [--torch_calls 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tsdf_fuse import HBM_BYTES_PER_S, frames, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--torch_calls", type=int, default=20)
    args = ap.parse_args()
    from datasets.synthetic import capsule_volume
    from hotrack_amd import sdf
    from models.volume_render import volume_raycast_torch
    dev = torch.device("cuda", 0)
    H, W = 480, 640
    rows = []
    for res in (128, 201):
        scale = 0.4 / (res - 1)
        vol = torch.from_numpy(capsule_volume(res, scale)).to(dev)
        for F in (1, 10):
            depth, seg, intr, rot, trans = frames(F, dev)
            z, _, steps = volume_raycast_torch(vol, scale, intr, rot, trans, (H, W), normals=False, return_steps=True)
            hit = z > 0
            steps_per_hit = float(steps[hit].float().mean())
            zk, _ = sdf.volume_raycast(vol, scale, intr, rot, trans, (H, W), normals=False)
            compare = timed(lambda: sdf.raycast_compare(zk, depth, seg), 20)
            for normals in (False, True):
                kernel = timed(lambda: sdf.volume_raycast(vol, scale, intr, rot, trans, (H, W), normals=normals), 20)
                route = timed(lambda: volume_raycast_torch(vol, scale, intr, rot, trans, (H, W), normals=normals), args.torch_calls)
                floor_us = F * H * W * 4 * (4 if normals else 1) / HBM_BYTES_PER_S * 1e6
                rows.append({"res": res, "frames": F, "normals": normals, "kernel": kernel, "torch": route, "output_write_floor_us": floor_us,
                             "torch_over_kernel": route["median_ms"] / kernel["median_ms"], "hit_share": float(hit.float().mean()),
                             "march_steps_per_hit_ray": steps_per_hit, "compare": compare})
                print("res %3d  F %2d  normals %d  kernel %8.1f us (%.1f .. %.1f)  torch %10.1f us (%.1f .. %.1f)  x%.0f  outputs written once at "
                      "HBM rate %5.2f us  steps / hit ray %.1f  compare %.1f us"
                      % (res, F, normals, 1e3 * kernel["median_ms"], 1e3 * kernel["min_ms"], 1e3 * kernel["max_ms"], 1e3 * route["median_ms"],
                         1e3 * route["min_ms"], 1e3 * route["max_ms"], route["median_ms"] / kernel["median_ms"], floor_us, steps_per_hit,
                         1e3 * compare["median_ms"]), flush=True)
    out = {"bench": "volume_raycast", "device": torch.cuda.get_device_name(0), "per_kernel_profile": False, "rows": rows}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
