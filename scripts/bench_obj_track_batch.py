"""Lockstep object tracking: S sequential `gf_optimize_obj.optimize` calls per frame step (one sequence at a time, route a)
against ONE `optimize_batch` of S (route b), on the synthetic capsule sequences at the reference's sizes (2048 particles, 1024
points, 201^3 fp16 corner volume, 10 iterations).

    python scripts/bench_obj_track_batch.py [--sizes 1,2,4,8,16,32] [--frames 20] [--reps 15] [--out FILE.md]

Per S and route: a repetition tracks max(`frames`, `--steps-total` / S) frame steps, so that a timed window is a few tenths of
a second at every S (frame t+1 starts from frame t's pose, as the tracker does; the `frames` clouds of a sequence repeat), timed
twice over the same work -- device time between two HIP events and wall time from the first Python line of the first step to
the end of a device synchronise -- and divided by the number of steps.  The two routes alternate repetition by repetition
(other work shares the machine: a drift hits both), after `--warmup` untimed repetitions of each.  Reported: the median and
the quartiles (q1-q3) over the repetitions.  `volumes`: `shared` = all S sequences track one object (one volume in cache),
`distinct` = every sequence has a copy of its own (S x 130 MB of lookup volume competing for the caches).  The final poses of
the two routes are compared bit for bit before anything is timed.  Needs a GPU: there is no fall-back."""
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


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return statistics.median(v), q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--frames", type=int, default=20, help="clouds per synthetic sequence, and the least steps per repetition")
    ap.add_argument("--steps-total", type=int, default=1280, help="a repetition runs max(frames, steps_total // S) frame steps")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--volumes", default="both", choices=["shared", "distinct", "both"])
    ap.add_argument("--res", type=int, default=201)
    ap.add_argument("--stride", type=float, default=0.002)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--out", default=None, help="write the table (markdown) here, and the raw figures next to it as .json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_obj_track_batch.py measures on a GPU; none is visible")
    from datasets.synthetic import SyntheticObjectSequences
    from hotrack_amd import sdf
    from models.optimization_obj import gf_optimize_obj

    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in args.sizes.split(",")]
    cfg = {"device": dev, "num_points": args.points, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}}
    ds = SyntheticObjectSequences(cfg, max(sizes), args.frames, res=args.res, stride=args.stride)
    seqs = [ds[s] for s in range(max(sizes))]
    clouds = [[fr["obj_points"].to(dev) for fr in seq] for seq in seqs]              # resident: the loader is not what is timed
    starts = [{k: seq[0]["jittered_obj_pose"][k].to(dev) for k in ("rotation", "translation")} for seq in seqs]
    volume = seqs[0][0]["sdf_volume"].to(dev).contiguous()
    opt = gf_optimize_obj({"device": dev}, seed=0)
    opt.load_volume(volume, args.stride)
    shared = opt._corners

    def steps_of(S):
        return max(args.frames, args.steps_total // S)

    def track_single(S, corners):
        poses = [dict(p) for p in starts[:S]]
        for t in range(steps_of(S)):
            for k in range(S):
                opt._corners = corners[k]   # (per sequence, not per frame, in the tracker: an attribute store)
                poses[k] = opt.optimize(clouds[k][t % args.frames], poses[k])
        return poses

    def track_batch(S, corners):
        poses = [dict(p) for p in starts[:S]]
        for t in range(steps_of(S)):
            poses = opt.optimize_batch([clouds[k][t % args.frames] for k in range(S)], poses, corners)
        return poses

    def timed(fn, S, corners):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        fn(S, corners)
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - w0
        return e0.elapsed_time(e1) * 1e3 / steps_of(S), wall * 1e6 / steps_of(S)   # microseconds per frame step

    rows = []
    modes = ["shared", "distinct"] if args.volumes == "both" else [args.volumes]
    for mode in modes:
        for S in sizes:
            corners = [shared] * S if mode == "shared" else [shared] + [sdf.CornerVolume(volume.clone()) for _ in range(S - 1)]
            a, b = track_single(S, corners), track_batch(S, corners)
            same = all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for x, y in zip(a, b) for k in ("rotation", "translation"))
            if not same:
                raise SystemExit(f"S = {S} ({mode}): the two routes' final poses differ -- nothing timed")
            for _ in range(args.warmup):
                timed(track_single, S, corners)
                timed(track_batch, S, corners)
            res = {"a": ([], []), "b": ([], [])}
            for _ in range(args.reps):
                for name, fn in (("a", track_single), ("b", track_batch)):
                    d, w = timed(fn, S, corners)
                    res[name][0].append(d)
                    res[name][1].append(w)
            row = {"volumes": mode, "S": S, "steps": steps_of(S), "bit_equal": True}
            for name in ("a", "b"):
                for what, v in zip(("device", "wall"), res[name]):
                    m, q1, q3 = quartiles(v)
                    row[f"{name}_{what}_us"] = {"median": m, "q1": q1, "q3": q3}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del corners
            torch.cuda.empty_cache()

    def cell(r, key):
        c = r[key]
        return "%.1f (%.1f-%.1f)" % (c["median"], c["q1"], c["q3"])

    lines = ["# Lockstep object tracking: S sequential optimize calls against one optimize_batch of S",
             "",
             "`python scripts/bench_obj_track_batch.py --sizes %s --frames %d --steps-total %d --reps %d --warmup %d --volumes %s`"
             % (args.sizes, args.frames, args.steps_total, args.reps, args.warmup, args.volumes),
             "",
             "Per frame step, microseconds: median (q1-q3) over %d repetitions of max(%d, %d / S) steps, routes alternating; %s; "
             "p = %d, n = %d, %d^3 fp16 corner volume, %d iterations." % (args.reps, args.frames, args.steps_total, torch.cuda.get_device_name(0),
                                                                         opt.pre_sampled_particle.shape[0], args.points, args.res, opt.iteration),
             "(a) = S sequential optimize calls, (b) = one optimize_batch of S.  Final poses of (a) and (b): bit-equal in every row.",
             "",
             "| volumes | S | steps | (a) device | (b) device | b/a device | (a) wall | (b) wall | b/a wall | (b) wall per sequence |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %d | %s | %s | %.2f | %s | %s | %.2f | %.0f |" % (
            r["volumes"], r["S"], r["steps"], cell(r, "a_device_us"), cell(r, "b_device_us"), r["b_device_us"]["median"] / r["a_device_us"]["median"],
            cell(r, "a_wall_us"), cell(r, "b_wall_us"), r["b_wall_us"]["median"] / r["a_wall_us"]["median"], r["b_wall_us"]["median"] / r["S"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
            json.dump({"args": vars(args), "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
