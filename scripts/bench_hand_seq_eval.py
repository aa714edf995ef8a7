"""Evaluation of tracked hand sequences: the per-frame `HandTrackModel.compute_loss` loop, once per sequence (route a -- the
parent route), against ONE `compute_loss_batch` for all S sequences (route b: two launches, hotrack_amd/csrc/kabsch.hip), on
synthetic tracked sequences of T frames (tests/_hand_eval_cases.make_case: results resident on the device, ground truth on the
host as the datasets hand it over).

    python scripts/bench_hand_seq_eval.py [--frames 100] [--sizes 1,8] [--reps 15] [--rounds 3] [--out FILE.md]

Every (S, with / without IKNet outputs) runs in a child process of its own under a time limit (`--limit` seconds); the first
child that fails, or runs out of time, ends the run -- nothing more is started on the device after it.  With IKNet outputs the
results carry `global_pose` and `MANO_theta` (the pose branch: no palm fits); without, the two palm fits per frame run.  A
repetition evaluates all S sequences once, timed twice over the same work -- device time between two HIP events and wall time to
the end of a device synchronise -- and divided by S.  The routes alternate repetition by repetition after `--warmup` untimed
ones.  Reported: median and quartiles over all repetitions, and the spread (max - min) of route a's own medians over `--rounds`
rounds of `--reps` repetitions.  Before anything is timed the two routes' dictionaries are compared: the same keys (route b adds
MANO_theta_diff), lengths and L1 terms within 2e-6, angles within 5e-3 degrees, the `init` keys left out (first frame against
mean: the documented difference).  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network"), os.path.join(ROOT, "tests")]


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return statistics.median(v), q[0], q[2]


def child(args, S, iknet):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hand_seq_eval.py measures on a GPU; none is visible")
    import _hand_eval_cases as C
    from hotrack_amd import pointnet2_utils
    from models import pointnet_utils
    from models.hand_network import HandTrackNet
    from models.track_network import HandTrackModel
    from netinit import make_cfg

    dev = torch.device("cuda", 0)
    pointnet_utils.set_operator_backend(pointnet2_utils)
    model = HandTrackModel(make_cfg(dev), handnet=HandTrackNet).to(dev).eval()
    frames, offsets, palm = C.make_case((args.frames,) * S, pose_mode=iknet, with_gt=True, with_theta=iknet, seed=args.frames)
    seqs, rets = [], []
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        one = {k: v[a:b] for k, v in frames.items()}
        tmpl = palm[q] if palm is not None else torch.zeros(6, 3)
        d, r = C.tracker_io(one, tmpl, device=dev)
        seqs.append(d)
        rets.append(r)
    flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": iknet}

    def loop():
        model.fused_hand_eval = False
        return [model.compute_loss(d, r, dict(flags))[0] for d, r in zip(seqs, rets)]

    def batch():
        return [o[0] for o in model.compute_loss_batch(seqs, rets, dict(flags))]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / S, (time.perf_counter() - w0) * 1e6 / S   # microseconds per sequence

    with torch.no_grad():
        a, b = loop(), batch()
        for da, db in zip(a, b):
            if [k for k in db if k != "MANO_theta_diff"] != list(da):
                raise SystemExit(f"S = {S}: the two routes report different keys -- nothing timed\n{list(da)}\n{list(db)}")
            for k in da:
                if "init" not in k and abs(da[k] - db[k]) > (5e-3 if k.endswith("_r_diff") else 2e-6):
                    raise SystemExit(f"S = {S}: {k} differs between the routes ({da[k]} / {db[k]}) -- nothing timed")
        for _ in range(args.warmup):
            timed(loop)
            timed(batch)
        res = {"a": ([], []), "b": ([], [])}
        round_medians = []
        for _ in range(args.rounds):
            for _ in range(args.reps):
                for name, fn in (("a", loop), ("b", batch)):
                    d, w = timed(fn)
                    res[name][0].append(d)
                    res[name][1].append(w)
            round_medians.append((statistics.median(res["a"][0][-args.reps:]), statistics.median(res["a"][1][-args.reps:])))
    row = {"S": S, "iknet": bool(iknet), "frames": args.frames, "device": torch.cuda.get_device_name(0),
           "a_round_spread_us": {"device": max(m[0] for m in round_medians) - min(m[0] for m in round_medians),
                                 "wall": max(m[1] for m in round_medians) - min(m[1] for m in round_medians)}}
    for name in ("a", "b"):
        for what, v in zip(("device", "wall"), res[name]):
            m, q1, q3 = quartiles(v)
            row[f"{name}_{what}_us"] = {"median": m, "q1": q1, "q3": q3}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100, help="frames per sequence")
    ap.add_argument("--sizes", default="1,8")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--out", default=None, help="write the table (markdown) here, and the raw figures next to it as .json")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        S, iknet = args.child.split(",")
        return child(args, int(S), iknet == "1")
    rows = []
    passed = [a for a in sys.argv[1:]]
    for S in (int(s) for s in args.sizes.split(",")):
        for iknet in (0, 1):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), *passed, "--child", f"{S},{iknet}"], capture_output=True,
                                   text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"S = {S}: no result within {args.limit} s -- stopped, nothing more is started")
            if p.returncode != 0:
                raise SystemExit(f"S = {S}: the child ended with status {p.returncode} -- stopped\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            rows += [json.loads(l[4:]) for l in p.stdout.splitlines() if l.startswith("ROW ")]
            print(json.dumps(rows[-1]), flush=True)

    def cell(r, key):
        c = r[key]
        return "%.0f (%.0f-%.0f)" % (c["median"], c["q1"], c["q3"])

    lines = ["# Evaluating tracked hand sequences: the per-frame compute_loss loop against one compute_loss_batch", "",
             "`python scripts/bench_hand_seq_eval.py --frames %d --sizes %s --reps %d --rounds %d --warmup %d`"
             % (args.frames, args.sizes, args.reps, args.rounds, args.warmup), "",
             "Per sequence of %d frames, microseconds: median (q1-q3) over %d x %d repetitions, routes alternating; %s."
             % (args.frames, args.rounds, args.reps, rows[0]["device"]),
             "(a) = compute_loss per sequence (the parent route), (b) = one compute_loss_batch of S.  Spread = max - min of (a)'s own "
             "round medians in the same run.", "",
             "| S | IKNet outputs | (a) device | (b) device | b/a device | (a) spread device | (a) wall | (b) wall | b/a wall | (a) spread wall |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %s | %s | %s | %.3f | %.0f | %s | %s | %.3f | %.0f |" % (
            r["S"], "yes" if r["iknet"] else "no", cell(r, "a_device_us"), cell(r, "b_device_us"),
            r["b_device_us"]["median"] / r["a_device_us"]["median"], r["a_round_spread_us"]["device"], cell(r, "a_wall_us"),
            cell(r, "b_wall_us"), r["b_wall_us"]["median"] / r["a_wall_us"]["median"], r["a_round_spread_us"]["wall"]))
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
