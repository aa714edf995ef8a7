"""Times hotrack_amd.sdf.obj_refine / obj_refine_batch (hotrack_amd/csrc/sdf_refine.hip) against the torch route
(network/models/pose_refine.obj_refine_torch) and against the 11-launch particle search of the same frame
(hotrack_amd.sdf.obj_optimize) on the same GPU: N = 512, 1024, 4096 points, iters = 8, S = 1, 4, 16 problems, the
synthetic sequences' fp16 201^3 capsule volume; 3 warm-up calls, then the median (min .. max) of 20 event-timed calls per route.

    python scripts/bench_obj_refine.py [--out profiles/obj_refine_bench.json] [--torch_calls 20]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    from _sdf_cases import _axis_angle, object_points, random_pose
    from datasets.synthetic import capsule_volume
    from hotrack_amd import sdf
    from models.pose_refine import obj_refine_torch
    dev = torch.device("cuda", 0)
    res, scale, iters = 201, 0.002, 8
    vol = torch.from_numpy(capsule_volume(res, scale)).to(dev)
    corner = sdf.CornerVolume(vol)
    pre = torch.from_numpy(np.random.default_rng(0).standard_normal((2048, 6)).astype(np.float32)).to(dev)
    pre[0] = 0
    rows = []
    for n in (512, 1024, 4096):
        R0, t0 = random_pose(1000 + n)
        pc = object_points(n, n, "capsule").astype(np.float64)
        cam = torch.from_numpy((pc @ R0.astype(np.float64).T + t0).astype(np.float32)).to(dev)
        R = torch.from_numpy((R0.astype(np.float64) @ _axis_angle(np.array([1.0, 2.0, 0.5]), 0.02)).astype(np.float32)).to(dev)
        t = torch.from_numpy(t0 + np.float32(0.002)).to(dev)
        search = timed(lambda: sdf.obj_optimize(cam, R, t, pre, corner, scale), 20)
        route = timed(lambda: obj_refine_torch(cam, R, t, vol, scale, iters), args.torch_calls)
        for S in (1, 4, 16):
            if S == 1:
                kernel = timed(lambda: sdf.obj_refine(cam, R, t, corner, scale, iters), 20)
            else:
                cache = {}
                kernel = timed(lambda: sdf.obj_refine_batch([cam] * S, [R] * S, [t] * S, [corner] * S, scale, iters, cache=cache), 20)
            row = {"n": n, "problems": S, "iters": iters, "kernel": kernel, "torch_one_problem": route, "obj_optimize_one_problem": search}
            rows.append(row)
            print("N %4d  S %2d  kernel %7.1f us (%.1f .. %.1f)  torch (one problem) %9.1f us (%.1f .. %.1f)  particle search (one problem, 11 launches) %7.1f us"
                  % (n, S, 1e3 * kernel["median_ms"], 1e3 * kernel["min_ms"], 1e3 * kernel["max_ms"], 1e3 * route["median_ms"],
                     1e3 * route["min_ms"], 1e3 * route["max_ms"], 1e3 * search["median_ms"]), flush=True)
    doc = {"bench": "obj_refine", "device": torch.cuda.get_device_name(0), "res": res, "rows": rows}
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
