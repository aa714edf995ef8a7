"""Mesh -> SDF volume on the MI355X: the kernel route (hotrack_amd/csrc/mesh_sdf.hip) against the torch composition of the same
definition on the same GPU (network/models/mesh_sdf.py, route='torch': the baseline), 201^3 and 151^3 volumes of the synthetic
capsule's mesh (4096 faces) and of the test torus (2688 faces).

    python scripts/bench_mesh_sdf.py [--calls 10] [--warmup 2] [--res 201 151] [--torch-calls 1] [--out profiles/mesh_sdf_bench.json]

One call = sdf.mesh_sdf_volume: a memset, the prepare launch, the volume launch and the one-word read-back of the face-index
check.  Each call is timed on its own with device events; the two routes alternate call by call after their warm-up.  The torch
route launches ~100 kernels per chunk of 2^22 (voxel, face) pairs, so it is timed `--torch-calls` times per configuration and only
where the configuration has at most `--torch-max-pairs` pairs (0 calls: skipped).  The JSON holds the median and the range per
route, the pair rate voxels * faces / median, and that rate against the fp32 vector peak with PAIR_FLOP operations per pair.

Kernel times, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o mesh_sdf -- python scripts/bench_mesh_sdf.py --kernel-only --calls 3
The stats list mesh_sdf_kernel and mesh_sdf_prepare_kernel, one of each per call."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network"), os.path.join(ROOT, "tests")]

# fp32 operations per (voxel, triangle) pair, counted in mesh_sdf_kernel's inner loop with an FMA as two: 9 for the three
# query - vertex differences, 3 x 22 for the edges, 35 for the face region, 55 for the solid angle's products and square roots,
# ~30 for atan2f
PAIR_FLOP = 195
PEAK_FP32_VECTOR = 157.3e12  # MI355X, packed FMA issue on every SIMD


def meshes():
    import _mesh_cases as MC
    from datasets.synthetic import capsule_mesh
    return {"capsule": capsule_mesh(), "torus48": MC.mesh("torus48")}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--res", type=int, nargs="+", default=[201, 151])
    p.add_argument("--torch-calls", type=int, default=1)
    p.add_argument("--torch-max-pairs", type=float, default=1.0e10)
    p.add_argument("--kernel-only", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_sdf.py needs a GPU")
    from hotrack_amd import sdf
    from models import mesh_sdf
    report = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup, "pair_flop": PAIR_FLOP, "results": []}
    for name, (v, f) in meshes().items():
        v, f = torch.from_numpy(v.copy()).cuda(), torch.from_numpy(f.copy()).cuda()
        for res in a.res:
            stride = 0.4 / (res - 1)  # the +-0.2 m box: 0.002 at 201
            pairs = res ** 3 * f.shape[0]
            kernel = lambda: sdf.mesh_sdf_volume(v, f, res, stride, 0.1, torch.float16)
            torch_route = lambda: mesh_sdf.mesh_to_volume(v, f, res, stride, 0.1, torch.float16, route="torch")
            n_torch = 0 if (a.kernel_only or pairs > a.torch_max_pairs) else a.torch_calls
            for _ in range(a.warmup):
                vol = kernel()
            torch.cuda.synchronize()
            tk, tt, ref = [], [], None
            for i in range(a.calls):  # alternated while the torch route has calls left
                tk.append(timed(kernel)[0])
                if i < n_torch:
                    ms, ref = timed(torch_route)
                    tt.append(ms)
            med = statistics.median(tk)
            rec = {"mesh": name, "faces": int(f.shape[0]), "res": res, "stride": stride, "pairs": pairs,
                   "kernel_ms": {"median": round(med, 3), "min": round(min(tk), 3), "max": round(max(tk), 3)},
                   "kernel_Gpairs_per_s": round(pairs / (med * 1e-3) / 1e9, 1),
                   "kernel_share_of_fp32_vector_peak": round(pairs * PAIR_FLOP / (med * 1e-3) / PEAK_FP32_VECTOR, 3)}
            if tt:
                rec["torch_ms"] = {"median": round(statistics.median(tt), 1), "min": round(min(tt), 1), "max": round(max(tt), 1), "calls": len(tt)}
                rec["speedup_median"] = round(statistics.median(tt) / med, 1)
                rec["max_abs_diff_fp16"] = float((vol.float() - ref.float()).abs().max())
            print(json.dumps(rec), flush=True)
            report["results"].append(rec)
    if not a.kernel_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
