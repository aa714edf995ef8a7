"""SDF volume -> triangle mesh on the MI355X: the kernel route (hotrack_amd/csrc/sdf_mesh.hip) against the torch route of the same
algorithm on the same GPU (network/models/mesh_sdf.py, route='torch': the baseline), on the synthetic capsule's fp16 volume at
128^3 and 201^3 (the +-0.2 m box).

    python scripts/bench_volume_mesh.py [--calls 20] [--warmup 3] [--res 128 201] [--torch-calls 5] [--out FILE.json]

Per resolution, each timed call by call with device events after the warm-up, the routes alternating:
  kernel_call_ms      sdf.volume_mesh: the workspace allocation, the count entry (3 launches), the read-back of the two totals,
                      the output allocation and the emit entry (1 launch);
  kernel_launches_ms  the four launches alone, into buffers allocated before (the device time of the extraction);
  torch_call_ms       mesh_sdf.volume_to_mesh(route='torch') on the GPU volume.
`two_reads_ms` is two reads of the volume at HBM_BYTES_PER_S, the yardstick DESIGN.md 8k compares the launches with;
`traffic_ms` is what the four launches must move at that rate (the volume twice, the mask bytes written and read twice, the
prefix written; the sparse reads and writes of the surface's own voxels are left out).

Kernel times, in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o volume_mesh -- python scripts/bench_volume_mesh.py --kernel-only --calls 3"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network")]

HBM_BYTES_PER_S = 8.0e12  # MI355X


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def stats(ms, digits=4):
    return {"median": round(statistics.median(ms), digits), "min": round(min(ms), digits), "max": round(max(ms), digits), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--res", type=int, nargs="+", default=[128, 201])
    p.add_argument("--torch-calls", type=int, default=5)
    p.add_argument("--kernel-only", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_mesh.py needs a GPU")
    from datasets.synthetic import capsule_volume
    from hotrack_amd import pointnet2_hip as native
    from hotrack_amd import sdf
    from models import mesh_sdf
    report = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "results": []}
    for res in a.res:
        stride = 0.4 / (res - 1)
        vol = torch.from_numpy(capsule_volume(res, stride)).cuda()
        kernel = lambda: sdf.volume_mesh(vol, stride)
        torch_route = lambda: mesh_sdf.volume_to_mesh(vol, stride, route="torch")
        verts, faces = kernel()
        nv, nf = verts.shape[0], faces.shape[0]
        work = torch.empty((sdf.volume_mesh_work_bytes(res) // 4 + 1,), dtype=torch.int32, device="cuda")
        st = native._stream(vol)

        def launches():
            rc = sdf._lib.pn2s_volume_mesh_count(vol.data_ptr(), 1, res, stride, 0.0, work.data_ptr(), work.numel() * 4, st)
            rc = rc or sdf._lib.pn2s_volume_mesh_emit(vol.data_ptr(), 1, res, stride, 0.0, work.data_ptr(), work.numel() * 4, nv, nf,
                                                      verts.data_ptr(), faces.data_ptr(), st)
            native._check(rc, "bench_volume_mesh")

        n_torch = 0 if a.kernel_only else a.torch_calls
        for _ in range(a.warmup):
            kernel()
            launches()
            if n_torch:
                ref = torch_route()
        torch.cuda.synchronize()
        tk, tl, tt = [], [], []
        for i in range(a.calls):
            tk.append(timed(kernel)[0])
            tl.append(timed(launches)[0])
            if i < n_torch:
                tt.append(timed(torch_route)[0])
        n = res ** 3
        rec = {"res": res, "stride": stride, "vertices": nv, "triangles": nf, "work_bytes": sdf.volume_mesh_work_bytes(res),
               "kernel_call_ms": stats(tk), "kernel_launches_ms": stats(tl),
               "two_reads_ms": round(2 * 2 * n / HBM_BYTES_PER_S * 1e3, 4),
               "traffic_ms": round((2 * 2 * n + 3 * n + 4 * n) / HBM_BYTES_PER_S * 1e3, 4)}
        rec["launches_over_two_reads"] = round(rec["kernel_launches_ms"]["median"] / rec["two_reads_ms"], 1)
        if tt:
            rec["torch_call_ms"] = stats(tt, 2)
            rec["speedup_median"] = round(rec["torch_call_ms"]["median"] / rec["kernel_call_ms"]["median"], 1)
            rec["same_faces"] = bool(torch.equal(ref[1], faces))
            rec["max_vertex_diff"] = float((ref[0] - verts).abs().max())
        print(json.dumps(rec), flush=True)
        report["results"].append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
