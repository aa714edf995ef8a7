"""Hand-object interaction columns of tracked hand sequences: eval_metrics.hand_interaction_metrics on its kernel route (two
launches, hotrack_amd/csrc/hand_interact.hip) against its torch route (lbs_forward_from_tables + the nearest-voxel lookup as
torch operations, chunked over the frames) on the same fp32 GPU tensors.

    python scripts/bench_hand_interaction.py [--seqs 4] [--frames 100] [--verts 778] [--res 151] [--model synthetic_mano]
                                             [--reps 15] [--rounds 3] [--out FILE.md]

S sequences of T frames of a seeded hand (random poses half a metre in front of the camera) against one fp16 sphere volume per
sequence.  The measurement runs in a child process under a time limit (`--limit` seconds); if it fails or runs out of time the
run ends there.  A repetition evaluates all S sequences once and is timed twice over the same work: device time between two HIP
events and wall time to the end of a device synchronise.  The routes alternate repetition by repetition after `--warmup` untimed
ones.  Reported: median and quartiles over all repetitions, and the spread (max - min) of the torch route's own medians over
`--rounds` rounds of `--reps` repetitions.  Before anything is timed the two routes' values are compared (the counts may differ by
the few vertices that sit on a voxel's face; more than 1 % of the vertices ends the run).  Needs a GPU: there is no fall-back."""
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


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hand_interaction.py measures on a GPU; none is visible")
    from models import eval_metrics
    from models.hand_model import SyntheticLBSHand, SyntheticManoHand, rodrigues

    dev = torch.device("cuda", 0)
    S, T, V, res = args.seqs, args.frames, args.verts, args.res
    hand = SyntheticManoHand(num_verts=V) if args.model == "synthetic_mano" else SyntheticLBSHand(num_verts=V, num_betas=10)
    tables = hand.skinning_tables()
    g = torch.Generator().manual_seed(7)
    F = S * T
    voxel_scale = round(0.45 / res, 4)
    ax = (torch.arange(res, dtype=torch.float32) - res // 2 + 0.5) * voxel_scale
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    volumes = [(torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - (0.03 + 0.01 * q)).half().to(dev).contiguous() for q in range(S)]
    t = torch.tensor([-0.02, -0.09, 0.5]) + 0.03 * torch.randn(F, 3, generator=g)
    frames = {"MANO_theta": 0.25 * torch.randn(F, 45, generator=g), "global_rotation": rodrigues(torch.tensor([0.25, -0.3, 0.35]) + 0.4 * torch.randn(F, 3, generator=g)),
              "global_translation": t, "obj_rotation": rodrigues(0.5 * torch.randn(F, 3, generator=g)),
              "obj_translation": t + torch.tensor([0.0, 0.06, 0.04]) + 0.01 * torch.randn(F, 3, generator=g),
              "beta": 0.8 * torch.randn(S, 10, generator=g), "rest_of": torch.arange(F) // T}
    frames["pred_kp"] = torch.zeros(F, 21, 3)
    frames = {k: v.to(dev).contiguous() for k, v in frames.items()}
    offsets = [q * T for q in range(S + 1)]
    seq_off = torch.tensor(offsets, dtype=torch.int32, device=dev)

    def run(route):
        return eval_metrics.hand_interaction_metrics(frames, offsets, tables, volumes, voxel_scale, route=route,
                                                     seq_off=seq_off if route == "kernel" else None)

    def timed(route):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        run(route)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - w0) * 1e6   # microseconds per call

    with torch.no_grad():
        rk, _, keys = run("kernel")
        rt, _, _ = run("torch")
        flips = float(((rk[:, 1] - rt[:, 1]).abs() * V).max())
        if not flips <= 0.01 * V:
            raise SystemExit(f"the routes' inside counts differ by {flips:.0f} vertices in a frame -- nothing timed")
        for _ in range(args.warmup):
            timed("torch")
            timed("kernel")
        res_ = {"torch": ([], []), "kernel": ([], [])}
        round_medians = []
        for _ in range(args.rounds):
            for _ in range(args.reps):
                for name in ("torch", "kernel"):
                    d, w = timed(name)
                    res_[name][0].append(d)
                    res_[name][1].append(w)
            round_medians.append((statistics.median(res_["torch"][0][-args.reps:]), statistics.median(res_["torch"][1][-args.reps:])))
    row = {"S": S, "frames": T, "verts": V, "res": res, "model": args.model, "device": torch.cuda.get_device_name(0),
           "count_difference_vertices": flips,
           "torch_round_spread_us": {"device": max(m[0] for m in round_medians) - min(m[0] for m in round_medians),
                                     "wall": max(m[1] for m in round_medians) - min(m[1] for m in round_medians)}}
    for name in ("torch", "kernel"):
        for what, v in zip(("device", "wall"), res_[name]):
            m, q1, q3 = quartiles(v)
            row[f"{name}_{what}_us"] = {"median": m, "q1": q1, "q3": q3}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=100, help="frames per sequence")
    ap.add_argument("--verts", type=int, default=778)
    ap.add_argument("--res", type=int, default=151)
    ap.add_argument("--model", default="synthetic_mano", choices=["synthetic_mano", "synthetic_shaped"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds the measurement may take")
    ap.add_argument("--out", default=None, help="write the table (markdown) here, and the raw figures next to it as .json")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--child"], capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"no result within {args.limit} s -- stopped, nothing more is started")
    if p.returncode != 0:
        raise SystemExit(f"the child ended with status {p.returncode} -- stopped\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    rows = [json.loads(l[4:]) for l in p.stdout.splitlines() if l.startswith("ROW ")]
    r = rows[0]
    cell = lambda key: "%.0f (%.0f-%.0f)" % (r[key]["median"], r[key]["q1"], r[key]["q3"])
    lines = ["# Hand-object interaction columns: the kernel route against the torch route", "",
             "`python scripts/bench_hand_interaction.py --seqs %d --frames %d --verts %d --res %d --model %s --reps %d --rounds %d --warmup %d`"
             % (args.seqs, args.frames, args.verts, args.res, args.model, args.reps, args.rounds, args.warmup), "",
             "One call for %d sequences x %d frames, microseconds: median (q1-q3) over %d x %d repetitions, routes alternating; %s."
             % (r["S"], r["frames"], args.rounds, args.reps, r["device"]),
             "Spread = max - min of the torch route's own round medians in the same run.", "",
             "| torch device | kernel device | kernel/torch device | torch spread device | torch wall | kernel wall | kernel/torch wall | torch spread wall |",
             "|---|---|---|---|---|---|---|---|",
             "| %s | %s | %.4f | %.0f | %s | %s | %.4f | %.0f |" % (
                 cell("torch_device_us"), cell("kernel_device_us"), r["kernel_device_us"]["median"] / r["torch_device_us"]["median"],
                 r["torch_round_spread_us"]["device"], cell("torch_wall_us"), cell("kernel_wall_us"),
                 r["kernel_wall_us"]["median"] / r["torch_wall_us"]["median"], r["torch_round_spread_us"]["wall"])]
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
