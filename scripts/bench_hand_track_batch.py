"""Lockstep hand tracking: S sequential fused `gf_optimize_hand_pose.optimize` calls per frame step (one sequence at a time,
route a -- the parent route) against ONE `optimize_batch` of S (route b), on the synthetic hand-object sequences at the
reference's sizes (5120 candidates x 5 iterations, 778 vertices, 151^3 volume, 640 x 480 mask).

    python scripts/bench_hand_track_batch.py [--sizes 1,2,4,8,16] [--reps 15] [--rounds 3] [--hand_model synthetic_mano] [--out FILE.md]

`--hand_model synthetic_mano` is the hand with MANO's structure: route a is then what `optimize_batch` falls back to without
`opt.lockstep_mano` (optimize() per sequence on the single MANO kernels), route b the lockstep MANO route with the switch on
(`ext.hand_pose_mano_opt_batch`; its offsets workspace is S times route a's).

Every S runs in a child process of its own under a time limit (`--limit` seconds); the first child that fails, or runs out of
time, ends the run -- nothing more is started on the device after it.  Per S and route a repetition is `--steps-total` / S frame
steps (each step starts every sequence from its frame's initial pose: the optimiser's work per step is the same in both routes),
timed twice over the same work -- device time between two HIP events and wall time to the end of a device synchronise -- and
divided by the number of steps.  The routes alternate repetition by repetition after `--warmup` untimed ones.  Reported: median
and quartiles over all repetitions, and, for the margin the S = 1 comparison is read against, the spread (max - min) of route
a's own medians over `--rounds` rounds of `--reps` repetitions in the same run.  The two routes' results are compared bit for
bit before anything is timed.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network")]


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return statistics.median(v), q[0], q[2]


def child(args, S):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hand_track_batch.py measures on a GPU; none is visible")
    from datasets.synthetic import SyntheticHandObjectSequences
    from models.hand_model import named_hand_model
    from models.optimization_hand import gf_optimize_hand_pose

    dev = torch.device("cuda", 0)
    hm = named_hand_model(args.hand_model)
    cfg = {"device": dev, "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"], "hand_model": hm,
           "opt": {"fused_pose": True, "lockstep_mano": True}}
    ds = SyntheticHandObjectSequences(cfg, S, 2)
    opt = gf_optimize_hand_pose(cfg, hand_model=hm, particle_size=args.particles)
    opt.load_volume(ds[0][0]["sdf_volume"], ds[0][0]["voxel_scale"])
    if not opt.use_kernel():
        raise SystemExit("the device-resident route is not available: nothing to compare")
    if opt._kernel_model()["mano"] != (args.hand_model == "synthetic_mano"):
        raise SystemExit(f"--hand_model {args.hand_model}: not the kind of skinning tables the name stands for")
    calls = []
    for s in range(S):   # resident inputs: the loader is not what is timed
        f0, f1 = ds[s]
        pose = {k: f1["gt_hand_pose"][k].to(dev) for k in ("rotation", "translation")}
        obj = {k: v.to(dev) for k, v in f1["gt_obj_pose"].items()}
        calls.append((f1["gt_hand_pose"]["mano_pose"].to(dev), pose, f1["jittered_hand_kp"].to(dev), f0["gt_hand_kp"].to(dev),
                      torch.ones(1, 21, dtype=torch.bool, device=dev), obj, None, f1["projection"], f1["background_mask"].to(dev)))
    steps = max(4, args.steps_total // S)

    def single():
        for _ in range(steps):
            out = [opt.optimize(*c) for c in calls]
        return out

    def batch():
        for _ in range(steps):
            out = opt.optimize_batch(calls)
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps, (time.perf_counter() - w0) * 1e6 / steps   # microseconds per frame step

    with torch.no_grad():
        a, b = single(), batch()
        if not all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for ra, rb in zip(a, b) for x, y in zip(ra, rb)):
            raise SystemExit(f"S = {S}: the two routes' results differ -- nothing timed")
        for _ in range(args.warmup):
            timed(single)
            timed(batch)
        res = {"a": ([], []), "b": ([], [])}
        round_medians = []
        for _ in range(args.rounds):
            for _ in range(args.reps):
                for name, fn in (("a", single), ("b", batch)):
                    d, w = timed(fn)
                    res[name][0].append(d)
                    res[name][1].append(w)
            round_medians.append((statistics.median(res["a"][0][-args.reps:]), statistics.median(res["a"][1][-args.reps:])))
    row = {"S": S, "steps": steps, "bit_equal": True, "device": torch.cuda.get_device_name(0), "particles": args.particles,
           "hand_model": args.hand_model, "vertices": opt._kernel_model()["V"],
           "iterations": opt.iteration,
           "a_round_spread_us": {"device": max(m[0] for m in round_medians) - min(m[0] for m in round_medians),
                                 "wall": max(m[1] for m in round_medians) - min(m[1] for m in round_medians)}}
    for name in ("a", "b"):
        for what, v in zip(("device", "wall"), res[name]):
            m, q1, q3 = quartiles(v)
            row[f"{name}_{what}_us"] = {"median": m, "q1": q1, "q3": q3}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--steps-total", type=int, default=64, help="a repetition runs max(4, steps_total // S) frame steps")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--particles", type=int, default=5120)
    ap.add_argument("--hand_model", choices=("synthetic", "synthetic_mano"), default="synthetic",
                    help="synthetic_mano: the per-sequence fallback (a) against the lockstep MANO route (b)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--out", default=None, help="write the table (markdown) here, and the raw figures next to it as .json")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args, args.child)
    rows = []
    passed = [a for a in sys.argv[1:]]
    for S in (int(s) for s in args.sizes.split(",")):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), *passed, "--child", str(S)], capture_output=True, text=True,
                               timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"S = {S}: no result within {args.limit} s -- stopped, nothing more is started")
        if p.returncode != 0:
            raise SystemExit(f"S = {S}: the child ended with status {p.returncode} -- stopped\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        rows += [json.loads(l[4:]) for l in p.stdout.splitlines() if l.startswith("ROW ")]
        print(json.dumps(rows[-1]), flush=True)

    def cell(r, key):
        c = r[key]
        return "%.1f (%.1f-%.1f)" % (c["median"], c["q1"], c["q3"])

    lines = ["# Lockstep hand tracking: S sequential fused optimize calls against one optimize_batch of S", "",
             "`python scripts/bench_hand_track_batch.py --sizes %s --steps-total %d --reps %d --rounds %d --warmup %d --particles %d%s`"
             % (args.sizes, args.steps_total, args.reps, args.rounds, args.warmup, args.particles,
                "" if args.hand_model == "synthetic" else " --hand_model " + args.hand_model), "",
             "Per frame step, microseconds: median (q1-q3) over %d x %d repetitions of max(4, %d / S) steps, routes alternating; %s; "
             "%d candidates x %d iterations." % (args.rounds, args.reps, args.steps_total, rows[0]["device"], rows[0]["particles"],
                                                 rows[0]["iterations"]),
             "(a) = S sequential optimize calls (the parent route), (b) = one optimize_batch of S; results bit-equal in every row.  "
             "Spread = max - min of (a)'s own round medians in the same run.", "",
             "| S | steps | (a) device | (b) device | b/a device | (a) spread device | (a) wall | (b) wall | b/a wall | (a) spread wall | (b) wall per sequence |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %d | %s | %s | %.2f | %.1f | %s | %s | %.2f | %.1f | %.0f |" % (
            r["S"], r["steps"], cell(r, "a_device_us"), cell(r, "b_device_us"), r["b_device_us"]["median"] / r["a_device_us"]["median"],
            r["a_round_spread_us"]["device"], cell(r, "a_wall_us"), cell(r, "b_wall_us"),
            r["b_wall_us"]["median"] / r["a_wall_us"]["median"], r["a_round_spread_us"]["wall"], r["b_wall_us"]["median"] / r["S"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
            json.dump({"args": {k: v for k, v in vars(args).items() if k != "child"}, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
