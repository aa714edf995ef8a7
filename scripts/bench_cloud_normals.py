"""Times ext.cloud_normals (hotrack_amd/csrc/cloud_normals.hip) against a torch route for the same normals (cdist -> topk ->
centred covariance -> linalg.eigh) at B in {1, 8}, N in {1024, 2048}, k = 30, and one ObservedSurface.add step against one frame
of gf_optimize_obj.optimize on a 256-point synthetic sequence.  Prints one JSON line; medians of event-timed runs after a warm-up.

    python scripts/bench_cloud_normals.py [--runs 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network")]


def timed(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    return float(np.median(times))


def torch_normals(points, k):
    d = torch.cdist(points, points)
    idx = d.topk(k, dim=-1, largest=False).indices                      # (B,N,k)
    nb = torch.gather(points[:, None].expand(-1, points.shape[1], -1, -1), 2, idx[..., None].expand(-1, -1, -1, 3))
    c = nb - nb.mean(2, keepdim=True)
    lam, vec = torch.linalg.eigh(c.transpose(-1, -2) @ c)
    n = vec[..., 0]
    return torch.where(((n * -points).sum(-1, keepdim=True) < 0), -n, n), lam[..., 0] / lam.sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    args = ap.parse_args()
    from hotrack_amd import ext, sdf
    from datasets.synthetic import SyntheticObjectSequences
    from models.obs_surface import ObservedSurface
    from models.optimization_obj import gf_optimize_obj
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "k": 30, "unit": "us", "kernel": {}, "torch_route": {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for B in (1, 8):
        for N in (1024, 2048):
            d = torch.randn((B, N, 3), device=dev, generator=g)
            pts = (0.03 * d / d.norm(dim=-1, keepdim=True) + torch.tensor([0.0, 0.0, 0.5], device=dev)).contiguous()
            out["kernel"][f"B{B}_N{N}"] = timed(lambda: ext.cloud_normals(pts, k=30, orient="view"), args.runs)
            out["torch_route"][f"B{B}_N{N}"] = timed(lambda: torch_normals(pts, 30), args.runs)
    cfg = {"device": dev, "data_cfg": {"dataset_name": "HO3D"}, "opt": {}, "num_points": 256, "obj_category": ["bottle"],
           "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt"}
    seq = SyntheticObjectSequences(cfg, 1, 2)[0]
    opt = gf_optimize_obj(cfg, seed=0)
    opt.load_volume(seq[0]["sdf_volume"], seq[0]["voxel_scale"])
    pose = {k: seq[0]["jittered_obj_pose"][k].to(dev) for k in ("rotation", "translation")}
    cloud = seq[0]["obj_points"].to(dev)
    surf = ObservedSurface(256).start(cloud, pose)

    def add():
        surf.frames = 1   # every timed step replaces M // 2 points, the largest step of a sequence
        surf.add(cloud, pose, opt._corners, opt.voxel_scale)

    out["surface_add_256"] = timed(add, args.runs)
    out["optimize_frame_256"] = timed(lambda: opt.optimize(cloud, pose), args.runs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
