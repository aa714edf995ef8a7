"""Times hotrack_amd.sdf.tsdf_integrate_batch (one launch for S sequences; hotrack_amd/csrc/tsdf_fuse.hip) against S calls of the
unchanged hotrack_amd.sdf.tsdf_integrate on the same data, with scripts/bench_tsdf_fuse.py's protocol and data:
S = 1, 4, 8 sequences of F = 1 and 10 frames of 480 x 640 each, res 128 and 201, the synthetic capsule's fp16 volume; 3 warm-up
calls, then the median (min .. max) of 20 event-timed calls.  Sequence k fuses the ten rendered frames starting at frame k (so
the sequences' poses differ); both routes read the same packed arrays.
Then, end to end: 8 synthetic --from_depth object sequences tracked with opt.fuse_depth, one `forward` per sequence (--seq_batch 1)
against `forward_batch` on two groups of 4 with opt.lockstep_fuse; wall-clock seconds with a device synchronisation, the median
of --e2e_runs runs after one warm-up run each.

    python scripts/bench_tsdf_fuse_batch.py [--out profiles/tsdf_fuse_batch_bench.json] [--e2e_frames 12] [--e2e_runs 3]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "network"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_tsdf_fuse import frames, timed  # noqa: E402


def kernel_rows(dev):
    from datasets.synthetic import capsule_volume
    from hotrack_amd import sdf
    rows = []
    pool = frames(10, dev)
    for res in (128, 201):
        scale = 0.4 / (res - 1)
        prior = torch.from_numpy(capsule_volume(res, scale, model_radius=0.03)).to(dev)
        kw = dict(trunc=5 * scale)
        for F in (1, 10):
            for S in (1, 4, 8):
                order = [[(k + i) % 10 for i in range(F)] for k in range(S)]
                packed = [torch.cat([x[o] for o in order]).contiguous() for x in pool]
                vols, wts = [prior.clone() for _ in range(S)], [torch.full((res,) * 3, 8.0, device=dev) for _ in range(S)]
                cache = {}
                batch = timed(lambda: sdf.tsdf_integrate_batch(vols, wts, scale, *packed, [F] * S, cache=cache, **kw), 20)
                slices = [[x[k * F:(k + 1) * F] for x in packed] for k in range(S)]
                vols1, wts1 = [prior.clone() for _ in range(S)], [torch.full((res,) * 3, 8.0, device=dev) for _ in range(S)]

                def singles():
                    for k in range(S):
                        sdf.tsdf_integrate(vols1[k], wts1[k], scale, *slices[k], **kw)
                single = timed(singles, 20)
                rows.append({"res": res, "frames": F, "sequences": S, "batch": batch, "singles": single,
                             "singles_over_batch": single["median_ms"] / batch["median_ms"]})
                print("res %3d  F %2d  S %d  one batched launch %8.1f us (%.1f .. %.1f)  %d single launches %8.1f us (%.1f .. %.1f)  ratio %.2f"
                      % (res, F, S, 1e3 * batch["median_ms"], 1e3 * batch["min_ms"], 1e3 * batch["max_ms"], S, 1e3 * single["median_ms"],
                         1e3 * single["min_ms"], 1e3 * single["max_ms"], rows[-1]["singles_over_batch"]), flush=True)
    return rows


def end_to_end(dev, n_frames, runs, res=201, stride=0.002, n_seq=8, group=4):
    from datasets.synthetic import SyntheticObjectSequences
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    flags = {"track_flag": True, "test_flag": True, "save_flag": False}

    def cfg(lockstep):
        return {"device": dev, "data_cfg": {"dataset_name": "HO3D"}, "num_points": 1024, "obj_category": ["bottle"],
                "opt": {"updateobjshape": False, "fuse_depth": True, "fuse_every": 10, "lockstep_fuse": lockstep},
                "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt", "from_depth": True}

    data = SyntheticObjectSequences(cfg(False), n_seq, n_frames, res=res, stride=stride, from_depth=True, model_radius=0.03)
    seqs = [data[k] for k in range(n_seq)]

    def model(lockstep):
        m = ObjTrackModel_Optimization(cfg(lockstep))
        m.optimizer = gf_optimize_obj(cfg(lockstep), seed=7)
        return m

    def one_by_one(m, inputs):
        return [m(seq, dict(flags)) for seq in inputs]

    def in_groups(m, inputs):
        out = []
        for i in range(0, n_seq, group):
            out += m.forward_batch(inputs[i:i + group], dict(flags))
        return out

    result = {"sequences": n_seq, "frames": n_frames, "res": res, "group": group, "runs": runs}
    kept = {}
    for name, lockstep, fn in (("seq_batch_1", False, one_by_one), ("seq_batch_4_lockstep_fuse", True, in_groups)):
        m = model(lockstep)
        secs = []
        with torch.no_grad():
            for run in range(runs + 1):   # (run 0 warms up)
                inputs = copy.deepcopy(seqs)
                torch.cuda.synchronize()
                start = time.perf_counter()
                kept[name] = fn(m, inputs)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - start)
        result[name] = {"median_s": statistics.median(secs[1:]), "min_s": min(secs[1:]), "max_s": max(secs[1:])}
        print("%s: %d sequences x %d frames  %.3f s (%.3f .. %.3f)  %.1f frames / s" % (name, n_seq, n_frames, result[name]["median_s"], result[name]["min_s"],
              result[name]["max_s"], n_seq * n_frames / result[name]["median_s"]), flush=True)
    a, b = kept["seq_batch_1"], kept["seq_batch_4_lockstep_fuse"]
    result["bit_equal"] = all(torch.equal(x[-1]["translation"], y[-1]["translation"]) and
                              torch.equal(x[0]["obj_fused"]["volume"], y[0]["obj_fused"]["volume"]) for x, y in zip(a, b))
    result["speedup"] = result["seq_batch_1"]["median_s"] / result["seq_batch_4_lockstep_fuse"]["median_s"]
    print("bit-equal poses and fused volumes: %s; seq_batch 1 / seq_batch 4: %.2f" % (result["bit_equal"], result["speedup"]), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--e2e_frames", type=int, default=12)
    ap.add_argument("--e2e_runs", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "tsdf_fuse_batch", "device": torch.cuda.get_device_name(0), "rows": kernel_rows(dev)}
    if args.e2e_frames > 0:
        out["end_to_end"] = end_to_end(dev, args.e2e_frames, args.e2e_runs)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
