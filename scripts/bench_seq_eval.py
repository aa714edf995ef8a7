"""Per-sequence evaluation on the MI355X: the kernel route (hotrack_amd/csrc/seq_eval.hip) against the torch composition of the
reference's expressions on the same GPU (network/models/eval_metrics.py, route='torch': the baseline), N = M = 2048 points,
T = 32, 256, 1024 frames.

    python scripts/bench_seq_eval.py [--calls 20] [--warmup 3] [--frames 32 256 1024] [--out profiles/seq_eval_bench.json]

One call = what ObjTrackModel_Optimization.compute_loss enqueues per sequence: the pose metrics of the T frames and the posed
chamfer of the T frames.  Each call is timed on its own with device events; the two routes alternate call by call, after
`warmup` calls of each; the JSON holds the median and the range per route and T, the pair rate T * N * M / median of the
chamfer and the largest difference between the routes' results.

Kernel times, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o seq_eval -- python scripts/bench_seq_eval.py --kernel-only --calls 5
The stats list posed_chamfer_kernel, posed_chamfer_sum_kernel and obj_pose_metrics_kernel, one of each per call."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network")]


def sequence(T, N, M, seed=0):
    from datasets.synthetic import _rot, model_points
    rng = np.random.default_rng(seed)
    A, B = model_points(seed, N), model_points(seed + 1, M) * 1.01
    Ra = np.stack([_rot(rng.standard_normal(3), rng.uniform(0, np.pi)) for _ in range(T)])
    Rb = np.stack([Ra[f] @ _rot(rng.standard_normal(3), np.deg2rad(rng.uniform(0.5, 12))) for f in range(T)])
    ta = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, (T, 3))
    tb = ta + rng.normal(0, 0.003, (T, 3))
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda().contiguous()
    return A.cuda(), B.cuda().contiguous(), f(Ra), f(ta), f(Rb), f(tb)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, nargs="+", default=[32, 256, 1024])
    p.add_argument("--points", type=int, default=2048)
    p.add_argument("--kernel-only", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_eval_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seq_eval.py needs a GPU")
    from models import eval_metrics
    routes = ("kernel",) if a.kernel_only else ("kernel", "torch")
    N = M = a.points
    report = {"device": torch.cuda.get_device_name(0), "N": N, "M": M, "calls": a.calls, "warmup": a.warmup, "results": []}
    for T in a.frames:
        A, B, Ra, ta, Rb, tb = sequence(T, N, M)
        gt, pred = {"rotation": Ra, "translation": ta}, {"rotation": Rb, "translation": tb}

        def call(route):
            return (eval_metrics.obj_pose_metrics(gt, pred, -1, False, route=route), eval_metrics.posed_chamfer(A, B, Ra, ta, Rb, tb, route=route))

        def chamfer(route):
            return eval_metrics.posed_chamfer(A, B, Ra, ta, Rb, tb, route=route)

        times = {(r, w): [] for r in routes for w in ("call", "chamfer")}
        outs = {}
        for r in routes:
            for _ in range(a.warmup):
                outs[r] = call(r)
        torch.cuda.synchronize()
        for _ in range(a.calls):
            for r in routes:  # alternated: drift of the clocks hits both routes alike
                for what, fn in (("call", call), ("chamfer", chamfer)):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn(r)
                    e.record()
                    e.synchronize()
                    times[(r, what)].append(s.elapsed_time(e) * 1e3)
        rec = {"T": T}
        for r in routes:
            for what in ("call", "chamfer"):
                v = times[(r, what)]
                rec[f"{r}_{what}_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            rec[f"{r}_chamfer_Gpairs_per_s"] = round(T * N * M / (rec[f"{r}_chamfer_us"]["median"] * 1e-6) / 1e9, 1)
        if len(routes) == 2:
            rec["speedup_call_median"] = round(rec["torch_call_us"]["median"] / rec["kernel_call_us"]["median"], 1)
            rec["chamfer_max_rel_diff"] = float(((outs["kernel"][1] - outs["torch"][1]).abs() / outs["torch"][1]).max())
            rec["rdiff_max_abs_diff_deg"] = float((outs["kernel"][0][:, 1] - outs["torch"][0][:, 1]).abs().max())
            rec["flags_equal"] = bool(torch.equal(outs["kernel"][0][:, 2:], outs["torch"][0][:, 2:]))
        print(json.dumps(rec), flush=True)
        report["results"].append(rec)
    if not a.kernel_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
