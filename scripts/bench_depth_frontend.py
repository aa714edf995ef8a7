"""Depth frames -> hand / object clouds on the MI355X: DepthFrontEnd.clouds (network/models/frame_frontend.py: the two depth-frame
kernels, FPS, the row gather) against the host route that existed before it -- numpy back-projection, split and crop per frame,
then datasets.data_utils.farthest_point_sample per cloud, with its random cut to 5 * npoint and its transfers -- on the same frames:
480 x 640 depth, the segmentation at 240 x 320 x 3, npoint = 1024, B in {1, 8}, frames rendered from the synthetic hand-object
sequences (datasets/synthetic.py, from_depth).

    python scripts/bench_depth_frontend.py [--calls 50] [--warmup 5] [--host-calls 10] [--batches 1 8] [--out profiles/depth_frontend_bench.json]

The device route is timed per call with device events round DepthFrontEnd.clouds on frames already on the device, eager and as a
replay of a captured graph, after warm-up; the upload of a batch's depth and segmentation is timed on its own (`upload_ms`).  The
host route is timed with the host clock per batch of frames (it ends in a device-to-host copy, which synchronises).  The two
alternate call by call.  The JSON holds medians and ranges.

Kernel times, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o depth_frontend -- python scripts/bench_depth_frontend.py --device-only --calls 20
The stats list depth_classify_kernel, depth_place_kernel, the FPS kernel and gather_rows_kernel, one of each per call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network")]
NPOINT, H, W = 1024, 480, 640
HAND_RADIUS, OBJ_RADIUS = 0.15, 0.25


def frames(count):
    """`count` rendered frames: depth (H,W) float32, seg (H/2,W/2,3) uint8, intrinsics, the two crop centres -- host arrays."""
    from datasets.synthetic import SyntheticHandObjectSequences
    from models.hand_model import SyntheticLBSHand
    cfg = {"num_points": NPOINT, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"], "hand_model": SyntheticLBSHand()}
    seq = SyntheticHandObjectSequences(cfg, 1, count, res=5, stride=0.1, from_depth=True)[0]
    out = []
    for fr in seq:
        k = fr["intrinsics"]
        out.append({"depth": fr["depth"][0].numpy(), "seg": np.ascontiguousarray(fr["seg"][0].numpy()[::2, ::2]),
                    "intrinsics": np.array([k["fx"], k["fy"], k["cx"], k["cy"]], dtype=np.float32),
                    "hand_centre": fr["hand_centre"][0].numpy(), "obj_centre": fr["obj_centre"][0].numpy()})
    return out


def host_route(batch, device, rng):
    """What a reader does per frame on the host (reference datasets/HO3D_dataset.py:66-112, :163-177), FPS on the GPU in the middle."""
    from datasets.data_utils import farthest_point_sample
    out = []
    for fr in batch:
        depth = fr["depth"]
        fx, fy, cx, cy = fr["intrinsics"]
        seg = fr["seg"].repeat(2, axis=0).repeat(2, axis=1).reshape(-1, 3)   # nearest-neighbour resize at the exact factor
        choose = (depth > 1e-6).reshape(-1).nonzero()[0]
        z = depth.reshape(-1)[choose].astype(np.float32)
        v, u = np.divmod(choose, W)
        cld = np.stack([(u.astype(np.float32) - cx) * z / fx, (v.astype(np.float32) - cy) * z / fy, z], axis=1)
        seg = seg[choose]
        clouds = []
        for channel, centre, radius in ((0, fr["hand_centre"], HAND_RADIUS), (1, fr["obj_centre"], OBJ_RADIUS)):
            pts = cld[seg[:, channel] == 255]
            pts = pts[np.linalg.norm(pts - centre, axis=-1) < radius]
            clouds.append(pts[farthest_point_sample(pts, NPOINT, device, rng)])
        out.append(clouds)
    return out


def device_frames(batch, dev):
    stack = lambda key: torch.from_numpy(np.stack([fr[key] for fr in batch])).to(dev)
    return {k: stack(k) for k in ("depth", "seg", "intrinsics", "hand_centre", "obj_centre")}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def summary(ms, digits=4):
    return {"median": round(statistics.median(ms), digits), "min": round(min(ms), digits), "max": round(max(ms), digits), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--host-calls", type=int, default=10)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    p.add_argument("--device-only", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_frontend_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_frontend.py needs a GPU")
    from models.frame_frontend import DepthFrontEnd
    dev = torch.device("cuda", 0)
    every = frames(max(a.batches))
    report = {"device": torch.cuda.get_device_name(0), "depth": [H, W], "seg": [H // 2, W // 2, 3], "npoint": NPOINT, "cap": 5 * NPOINT,
              "warmup": a.warmup, "results": []}
    for B in a.batches:
        batch = every[:B]
        front = DepthFrontEnd(NPOINT, hand_radius=HAND_RADIUS, obj_radius=OBJ_RADIUS, device=dev)
        fr = device_frames(batch, dev)
        rng = np.random.default_rng(0)
        n_host = 0 if a.device_only else a.host_calls
        for _ in range(a.warmup):
            out = front.clouds(fr)
        for _ in range(min(a.warmup, 2) if n_host else 0):
            host_route(batch, dev, rng)
        torch.cuda.synchronize()
        graph = None
        if not a.device_only:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                front.clouds(fr)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                front.clouds(fr)
            for _ in range(a.warmup):
                graph.replay()
            torch.cuda.synchronize()
        eager, replay, host, upload = [], [], [], []
        for i in range(a.calls):   # the routes alternate call by call
            eager.append(timed(lambda: front.clouds(fr))[0])
            if graph is not None:
                replay.append(timed(graph.replay)[0])
                upload.append(timed(lambda: device_frames(batch, dev))[0])
            if i < n_host:
                t0 = time.perf_counter()
                host_route(batch, dev, rng)
                host.append((time.perf_counter() - t0) * 1e3)
        rec = {"B": B, "class_pixels": out["counts"].cpu().numpy().tolist(), "eager_ms": summary(eager)}
        if replay:
            rec["graph_replay_ms"], rec["upload_ms"] = summary(replay), summary(upload)
        if host:
            rec["host_route_ms"] = summary(host, 2)
            rec["host_over_eager_median"] = round(statistics.median(host) / statistics.median(eager), 1)
            rec["host_over_replay_plus_upload_median"] = round(statistics.median(host) / (statistics.median(replay) + statistics.median(upload)), 1)
        print(json.dumps(rec), flush=True)
        report["results"].append(rec)
    if not a.device_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
