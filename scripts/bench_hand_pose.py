"""Per-frame cost of the hand-pose particle optimiser (gf_optimize_hand_pose.optimize) on the MI355X: the torch route against
the device-resident route (opt.fused_pose, hotrack_amd/csrc/hand_pose.hip), P = 5120 candidates x 5 iterations.

    python scripts/bench_hand_pose.py [--particles 5120] [--frames 16] [--warmup 3] [--rounds 3] [--hand_model synthetic_mano]

The synthetic hand-object sequence (datasets/synthetic.SyntheticHandObjectSequences, 151^3 fp16 volume, 640 x 480 silhouette)
is tracked the way HandTrackModel drives the optimiser: jittered ground-truth keypoints stand in for HandTrackNet, the previous
optimum and a rigid keypoint fit for IKNet, the result feeds the next frame.  All inputs are staged on the device first.
`rounds` times, alternating: the torch route, the fused route eager, the fused route as a replayed graph -- each `warmup`
passes over the sequence untimed, then one timed pass with device events around every optimize() call (steady state: no
first-call costs).  Prints one JSON line: per route the median and the range of the per-optimize time over all rounds, the
per-round medians, and the largest keypoint difference between the routes.  With --hand_model synthetic_mano the hand has
MANO's structure (SyntheticManoHand: the MANO kernels with their pose-offset pre-pass) and the plain hand is measured beside it
in the same run, the two models' routes alternating; the line then holds one record per model.

Kernel times, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/hand_pose_trace -o hand_pose -- \\
        python scripts/bench_hand_pose.py --rounds 1 --routes fused
The stats list hand_pose_eval_kernel<true> and hand_pose_update_kernel, five calls each per optimize() (with --hand_model
synthetic_mano: hand_pose_offsets_kernel, hand_pose_mano_eval_kernel<true> and hand_pose_update_kernel)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network"), os.path.join(ROOT, "tests")]

ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}


def make_optimiser(hm, particles, fused, seq):
    from models.optimization_hand import gf_optimize_hand_pose
    opt = gf_optimize_hand_pose({"device": "cuda", "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": fused}},
                                hand_model=hm, particle_size=particles, seed=0)
    opt.load_volume(seq[0]["sdf_volume"], seq[0]["voxel_scale"])
    return opt


def stage(seq, hm):
    """Per frame the device-resident inputs of optimize() except the previous frame's keypoints."""
    from hotrack_amd import ext
    g = torch.Generator().manual_seed(0)
    frames = []
    with torch.no_grad():
        _, kp0 = hm.forward(th_pose_coeffs=torch.zeros(1, 48, device="cuda"), th_trans=torch.zeros(1, 3, device="cuda"))
        for fr in seq:
            kp = (fr["gt_hand_kp"] + 0.002 * torch.randn(1, 21, 3, generator=g)).cuda()
            R, t = ext.kabsch(kp0.contiguous(), kp.contiguous())
            vis = torch.ones(1, 21, dtype=torch.bool, device="cuda")
            vis[0, [8, 12]] = False  # two occluded fingertips: the attraction term is formed
            frames.append(dict(pose={"rotation": R.reshape(1, 3, 3), "translation": t.reshape(1, 3, 1)}, kp=kp, vis=vis,
                               obj={k: v.cuda() for k, v in fr["gt_obj_pose"].items()},
                               proj={k: float(v[0]) for k, v in fr["projection"].items()}, mask=fr["background_mask"].cuda()))
    return frames


def run_pass(opt, frames, timed, graphs=None):
    """One pass over the sequence; returns (per-optimize ms or [], final keypoints per frame)."""
    times, kps, prev_kp, theta = [], [], None, torch.zeros(1, 45, device="cuda")
    for i, f in enumerate(frames):
        last = prev_kp if prev_kp is not None else None
        args = (theta, f["pose"], f["kp"], last, f["vis"], f["obj"], None, f["proj"], f["mask"])
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if graphs is not None and last is not None:
            key = "g"
            if key not in graphs:  # one graph for every frame with a previous frame: static inputs, replayed
                static = dict(theta=theta.clone(), R=f["pose"]["rotation"].clone(), t=f["pose"]["translation"].clone(), kp=f["kp"].clone(),
                              last=last.clone(), vis=f["vis"].clone(), oR=f["obj"]["rotation"].clone(), ot=f["obj"]["translation"].clone())
                sargs = (static["theta"], {"rotation": static["R"], "translation": static["t"]}, static["kp"], static["last"], static["vis"],
                         {"rotation": static["oR"], "translation": static["ot"]}, None, f["proj"], f["mask"])
                opt.optimize(*sargs)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = opt.optimize(*sargs)
                graphs[key] = (graph, static, out)
            graph, static, out = graphs[key]
            s.record()
            for k, v in (("theta", theta), ("R", f["pose"]["rotation"]), ("t", f["pose"]["translation"]), ("kp", f["kp"]), ("last", last),
                         ("vis", f["vis"]), ("oR", f["obj"]["rotation"]), ("ot", f["obj"]["translation"])):
                static[k].copy_(v, non_blocking=True)
            graph.replay()
            kp, th = out[0].clone(), out[1].clone()
            e.record()
        else:
            s.record()
            kp, th, _, _ = opt.optimize(*args)
            e.record()
        torch.cuda.synchronize()
        if timed and i > 0:
            times.append(s.elapsed_time(e))
        prev_kp, theta = kp.clone(), th.clone()
        kps.append(prev_kp)
    return times, kps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=5120)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--routes", default="torch,fused,fused_graph")
    p.add_argument("--hand_model", default="synthetic", choices=["synthetic", "synthetic_mano"])
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hand_pose.py needs a GPU")
    from datasets.synthetic import SyntheticHandObjectSequences
    from models.hand_model import named_hand_model
    routes = a.routes.split(",")
    models = {}
    for name in dict.fromkeys([a.hand_model, "synthetic"]):  # the MANO hand first, the plain hand beside it
        hm = named_hand_model(name)
        cfg = {"num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"], "hand_model": hm}
        seq = SyntheticHandObjectSequences(cfg, 1, a.frames)[0]
        opts = {"torch": make_optimiser(hm, a.particles, False, seq), "fused": make_optimiser(hm, a.particles, True, seq)}
        if not opts["fused"].use_kernel():
            raise SystemExit("bench_hand_pose.py: the fused route is not available")
        models[name] = dict(opts=opts, frames=stage(seq, opts["fused"].mano_layer_right), graphs={}, per_round={r: [] for r in routes}, kps={})
    with torch.no_grad():
        for _ in range(a.rounds):
            for r in routes:
                for m in models.values():
                    opt, gr = m["opts"]["torch" if r == "torch" else "fused"], (m["graphs"] if r == "fused_graph" else None)
                    for _ in range(a.warmup):
                        run_pass(opt, m["frames"], False, gr)
                    t, m["kps"][r] = run_pass(opt, m["frames"], True, gr)
                    m["per_round"][r].append(t)
    recs = {}
    for name, m in models.items():
        per_round, kps = m["per_round"], m["kps"]
        rec = {"particles": a.particles, "iterations": 5, "frames_timed_per_round": a.frames - 1, "rounds": a.rounds}
        for r in routes:
            allt = [x for t in per_round[r] for x in t]
            rec[r] = {"ms_per_optimize_median": round(statistics.median(allt), 4), "min": round(min(allt), 4), "max": round(max(allt), 4),
                      "round_medians": [round(statistics.median(t), 4) for t in per_round[r]]}
        if "torch" in kps and "fused" in kps:
            rec["max_kp_diff_fused_vs_torch_m"] = float(max((x - y).abs().max() for x, y in zip(kps["fused"], kps["torch"])))
            fused_runs = [x for r in routes if r != "torch" for t in per_round[r] for x in t]
            rec["every_fused_run_beats_every_torch_run"] = max(fused_runs) < min(x for t in per_round["torch"] for x in t)
        recs[name] = rec
    print(json.dumps(recs["synthetic"] if a.hand_model == "synthetic" else recs), flush=True)


if __name__ == "__main__":
    main()
