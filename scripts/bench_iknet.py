"""Per-frame IKNet forward on the MI355X: kernel route (hotrack_amd/csrc/iknet.hip) against the torch route, M = 1, 8, 16 rows.

    python scripts/bench_iknet.py [--iters 200] [--warmup 20] [--graph]

Times IKNet.solve (palm fit + network + quaternion conversion) with device events around `iters` calls after `warmup` calls
(--graph: each route captured into a HIP graph and replayed), prints one JSON line per (route, M) and, for the kernel route,
the weight bytes the seven launches read over the measured time against the 8 TB/s HBM bound.

Kernel times, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/iknet_trace -o iknet -- python scripts/bench_iknet.py --iters 100
The stats list iknet_layer_kernel<128, true>, five iknet_layer_kernel<1024, false> and iknet_head_kernel per call."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network"), os.path.join(ROOT, "tests")]

WEIGHT_BYTES = 4 * (1024 * 128 + 5 * 1024 * 1024 + 60 * 1024 + 6 * 1024 + 60)
HBM_BYTES_PER_S = 8e12


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--graph", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iknet.py needs a GPU")
    from _iknet_cases import load_into
    from models.hand_model import SyntheticLBSHand
    from models.iknet import IKNet
    m = IKNet({"device": "cuda", "network": {"iknetframe": "kp"}})
    load_into(m)
    m = m.cuda().eval()
    hm = SyntheticLBSHand()
    with torch.no_grad():
        _, rest = hm.forward(th_pose_coeffs=torch.zeros(1, 48), th_trans=torch.zeros(1, 3))
    palm = rest[:, [0, 1, 5, 9, 13, 17]].cuda()
    g = torch.Generator().manual_seed(0)
    for M in (1, 8, 16):
        with torch.no_grad():
            _, kp = hm.forward(th_pose_coeffs=0.3 * torch.randn(M, 48, generator=g), th_trans=torch.tensor([[0.0, 0.0, 0.5]]).expand(M, 3))
        kp = kp.cuda().contiguous()
        outs = {}
        for route in ("kernel", "torch"):
            m.use_kernel = route == "kernel"
            with torch.no_grad():
                call = lambda: m.solve(kp, palm)
                for _ in range(a.warmup):
                    out = call()
                if a.graph:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        out = call()
                    call = graph.replay
                    call()
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    call()
                e.record()
                torch.cuda.synchronize()
            us = s.elapsed_time(e) * 1e3 / a.iters
            outs[route] = out[0].clone()
            rec = {"route": route, "M": M, "graph": a.graph, "us_per_frame": round(us, 2)}
            if route == "kernel":
                rec["weight_GBps"] = round(WEIGHT_BYTES / (us * 1e-6) / 1e9, 1)
                rec["hbm_bound_us"] = round(WEIGHT_BYTES / HBM_BYTES_PER_S * 1e6, 2)
            print(json.dumps(rec), flush=True)
        print(json.dumps({"M": M, "max_abs_diff_kernel_vs_torch": float((outs["kernel"] - outs["torch"]).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
