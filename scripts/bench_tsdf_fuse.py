"""Times hotrack_amd.sdf.tsdf_integrate (hotrack_amd/csrc/tsdf_fuse.hip) against network/models/shape_fusion.tsdf_integrate_torch
on the same GPU: res 128 and 201, F = 1 and 10 frames of 480 x 640 rendered from the synthetic capsule at poses
round it, the synthetic sequences' fp16 volume; 3 warm-up calls, then the median (min .. max) of 20 event-timed calls per route.
Also prints the time of two reads and two writes of volume and weights at the measured HBM copy rate (6.29 TB/s).

    python scripts/bench_tsdf_fuse.py [--out profiles/tsdf_fuse_bench.json] [--torch_calls 20]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "network"))

HBM_BYTES_PER_S = 6.29e12


def frames(F, device):
    from datasets.synthetic import _rot, capsule_surface, render_depth_frame
    K = dict(fx=600.0, fy=600.0, cx=320.0, cy=240.0)
    depth, seg, rot, trans = [], [], [], []
    for k in range(F):
        R = _rot(np.array([0.3, 1.0, 0.2]), 0.6 * k + 0.2)
        t = np.array([0.01 * k, -0.01, 0.5])
        pts = capsule_surface(np.random.default_rng(100 + k), 16384) @ R.T + t
        d, s, _, _ = render_depth_frame(None, pts, K, 480, 640, splat=1)
        depth.append(torch.from_numpy(d)), seg.append(torch.from_numpy(s))
        rot.append(torch.from_numpy(R.astype(np.float32))), trans.append(torch.from_numpy(t.astype(np.float32)))
    intr = torch.tensor([[K["fx"], K["fy"], K["cx"], K["cy"]]] * F, dtype=torch.float32)
    return [x.to(device).contiguous() for x in (torch.stack(depth), torch.stack(seg), intr, torch.stack(rot), torch.stack(trans))]


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--torch_calls", type=int, default=20)
    args = ap.parse_args()
    from datasets.synthetic import capsule_volume
    from hotrack_amd import sdf
    from models.shape_fusion import tsdf_integrate_torch
    dev = torch.device("cuda", 0)
    rows = []
    for res in (128, 201):
        scale = 0.4 / (res - 1)
        prior = torch.from_numpy(capsule_volume(res, scale, model_radius=0.03)).to(dev)
        for F in (1, 10):
            fr = frames(F, dev)
            kw = dict(trunc=5 * scale)
            vol, wt = prior.clone(), torch.full((res,) * 3, 8.0, device=dev)
            kernel = timed(lambda: sdf.tsdf_integrate(vol, wt, scale, *fr, **kw), 20)
            vol_t, wt_t = prior.clone(), torch.full((res,) * 3, 8.0, device=dev)
            route = timed(lambda: tsdf_integrate_torch(vol_t, wt_t, scale, *fr, **kw), args.torch_calls)
            floor_us = 2 * res ** 3 * (prior.element_size() + 4) / HBM_BYTES_PER_S * 1e6
            row = {"res": res, "frames": F, "kernel": kernel, "torch": route, "read_write_floor_us": floor_us}
            rows.append(row)
            print("res %3d  F %2d  kernel %8.1f us (%.1f .. %.1f)  torch %9.1f us (%.1f .. %.1f)  volume + weights read and written once at HBM rate %5.1f us"
                  % (res, F, 1e3 * kernel["median_ms"], 1e3 * kernel["min_ms"], 1e3 * kernel["max_ms"], 1e3 * route["median_ms"],
                     1e3 * route["min_ms"], 1e3 * route["max_ms"], floor_us), flush=True)
    print(json.dumps({"bench": "tsdf_fuse", "device": torch.cuda.get_device_name(0), "rows": rows}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"bench": "tsdf_fuse", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
