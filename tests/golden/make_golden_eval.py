"""Generates tests/golden/eval_metrics.npz from the IMPORTED reference.  RUNS ONLY IN THE BUILD CONTAINER (needs
/root/reference); the tests only read the .npz file.  No reference file is touched or copied.

  pose cases   pose_utils.part_dof_utils.eval_part_full (per_instance=True: the per-pair terms) on 24 seeded pose pairs per
               symmetry mode: axis 0, 1, 2 each with and without up_and_down_sym, 3 (box), -1 (bottle), 5 (no symmetry).
               Rotation errors between 0.5 and 170 degrees, a third of the pairs composed with one of the mode's 180-degree
               flips (so the flip is the minimiser), translation errors between 1 mm and 20 cm.  A pair whose rdiff / tdiff
               falls within 1e-2 degrees / 1e-4 m of a threshold is redrawn, and the generator asserts that none is left: a
               threshold can never flip between implementations.
  chamfer      the reference's compute_chamfer (track_network.py:91-94) on its two transformed clouds (:431-432), fp32 on the
               CPU: 6 frames, N = 512, M = 384.  The expression is evaluated from the reference's own source text (the module
               itself imports the MANO layer and the optimisers, which this image cannot load).
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
MODES = [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, False), (-1, False), (5, False)]
PAIRS = 24


def reference_compute_chamfer():
    """The reference's compute_chamfer, compiled from its own file (only that function's source; nothing is copied)."""
    path = os.path.join(REF, "network", "models", "track_network.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_chamfer"]
    assert len(fn) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["compute_chamfer"]


def rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def flips(axis):
    if axis == 3:
        return [np.diag([-1., -1., 1.]), np.diag([-1., 1., -1.]), np.diag([1., -1., -1.])]
    if axis == -1:
        return [np.diag([-1., 1., -1.])]
    return []


def clear_of_thresholds(rdiff, tdiff):
    return (min(abs(rdiff - 5.0), abs(rdiff - 10.0)) > 1e-2) and (min(abs(tdiff - 0.05), abs(tdiff - 0.10)) > 1e-4)


def main():
    sys.path[:0] = [REF, os.path.join(REF, "pose_utils")]
    from pose_utils.part_dof_utils import eval_part_full
    out = {"modes": np.array([[a, int(s)] for a, s in MODES], dtype=np.int32)}
    for mi, (axis, sym) in enumerate(MODES):
        rng = np.random.default_rng(9000 + mi)
        gR, gt, pR, pt, ref = [], [], [], [], []
        angles = np.deg2rad(np.concatenate([[0.5, 1.0, 4.0, 4.9, 5.2, 9.5, 10.5, 170.0], np.exp(rng.uniform(np.log(0.5), np.log(170.0), PAIRS - 8))]))
        k = 0
        while len(gR) < PAIRS:
            R1 = rot(rng.standard_normal(3), rng.uniform(0, np.pi))
            R2 = R1 @ rot(rng.standard_normal(3), angles[len(gR)])
            F = flips(axis)
            if F and k % 3 == 2:  # the prediction sits near a flipped copy: the flip is the minimiser
                R2 = R2 @ F[(k // 3) % len(F)]
            if axis in (0, 1, 2) and sym and k % 3 == 2:  # upside down about an axis orthogonal to the symmetry axis
                R2 = R2 @ np.diag([(1. if (axis + 1) % 3 == j else -1.) for j in range(3)])
            k += 1
            t1 = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.1, 0.1, 3)
            d = rng.standard_normal(3)
            t2 = t1 + d / np.linalg.norm(d) * np.exp(rng.uniform(np.log(1e-3), np.log(0.2)))
            g = {"rotation": torch.from_numpy(R1.astype(np.float32)).reshape(1, 1, 3, 3), "translation": torch.from_numpy(t1.astype(np.float32)).reshape(1, 1, 3, 1)}
            p = {"rotation": torch.from_numpy(R2.astype(np.float32)).reshape(1, 1, 3, 3), "translation": torch.from_numpy(t2.astype(np.float32)).reshape(1, 1, 3, 1)}
            _, per = eval_part_full(g, p, per_instance=True, axis=axis, up_and_down_sym=sym)
            row = [float(per[key][0]) for key in ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")]
            if not clear_of_thresholds(row[1], row[0]):
                continue
            gR.append(g["rotation"].numpy().reshape(3, 3))
            gt.append(g["translation"].numpy().reshape(3))
            pR.append(p["rotation"].numpy().reshape(3, 3))
            pt.append(p["translation"].numpy().reshape(3))
            ref.append(row)
        ref = np.array(ref, dtype=np.float32)
        assert all(clear_of_thresholds(r[1], r[0]) for r in ref)
        # the batched call the trackers make gives the same per-pair terms and their means
        g = {"rotation": torch.from_numpy(np.stack(gR)).reshape(PAIRS, 1, 3, 3), "translation": torch.from_numpy(np.stack(gt)).reshape(PAIRS, 1, 3, 1)}
        p = {"rotation": torch.from_numpy(np.stack(pR)).reshape(PAIRS, 1, 3, 3), "translation": torch.from_numpy(np.stack(pt)).reshape(PAIRS, 1, 3, 1)}
        mean, per = eval_part_full(g, p, per_instance=True, axis=axis, up_and_down_sym=sym)
        batched = np.stack([per[key].numpy() for key in ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")], axis=-1)
        assert np.allclose(batched, ref, rtol=0, atol=1e-4) and (batched[:, 2:] == ref[:, 2:]).all()
        out[f"m{mi}_gt_R"], out[f"m{mi}_gt_t"], out[f"m{mi}_pred_R"], out[f"m{mi}_pred_t"] = np.stack(gR), np.stack(gt), np.stack(pR), np.stack(pt)
        out[f"m{mi}_ref"] = batched.astype(np.float32)
        out[f"m{mi}_mean"] = np.array([float(mean[key]) for key in ("tdiff_0", "rdiff_0", "5deg5cm_0", "10deg10cm_0")], dtype=np.float32)
        print(f"axis {axis:2d} sym {int(sym)}: rdiff {ref[:, 1].min():7.3f} .. {ref[:, 1].max():7.3f} deg, 5deg5cm {ref[:, 2].mean():.2f}, 10deg10cm {ref[:, 3].mean():.2f}")

    # ---- chamfer ---------------------------------------------------------------------------------------------------
    compute_chamfer = reference_compute_chamfer()
    rng = np.random.default_rng(9100)
    T, N, M = 6, 512, 384

    def cloud(n):  # a bottle-sized capsule's surface
        z, phi = rng.uniform(-0.11, 0.11, n), rng.uniform(0, 2 * np.pi, n)
        r = np.sqrt(np.maximum(0.04 ** 2 - (z - np.clip(z, -0.07, 0.07)) ** 2, 0.0))
        return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1).astype(np.float32)

    A, B = cloud(N), (cloud(M) * 1.03).astype(np.float32)
    Ra, ta, Rb, tb, ref = [], [], [], [], []
    gt_mesh, pred_mesh = torch.from_numpy(A), torch.from_numpy(B)
    for f in range(T):
        R1 = rot(rng.standard_normal(3), rng.uniform(0, np.pi)).astype(np.float32)
        t1 = (np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, 3)).astype(np.float32)
        R2 = (R1 @ rot(rng.standard_normal(3), np.deg2rad(0.5 * 3 ** f))).astype(np.float32)  # 0.5 .. 121 degrees
        t2 = (t1 + rng.normal(0, 0.002 * (f + 1), 3)).astype(np.float32)
        gR, gT, pRr, pT = (torch.from_numpy(x) for x in (R1, t1, R2, t2))
        a = torch.matmul(gt_mesh.clone(), gR.transpose(-1, -2)) + gT      # track_network.py:431
        b = torch.matmul(pred_mesh.clone(), pRr.transpose(-1, -2)) + pT    # :432
        ref.append(float(compute_chamfer(a, b)))
        Ra.append(R1)
        ta.append(t1)
        Rb.append(R2)
        tb.append(t2)
    out.update(cf_A=A, cf_B=B, cf_Ra=np.stack(Ra), cf_ta=np.stack(ta), cf_Rb=np.stack(Rb), cf_tb=np.stack(tb),
               cf_ref=np.array(ref, dtype=np.float32), cf_raw=np.array([float(compute_chamfer(gt_mesh, pred_mesh))], dtype=np.float32))
    print("chamfer (mm):", np.round(np.array(ref) * 1000, 3), "raw", float(out["cf_raw"][0]) * 1000)
    path = os.path.join(HERE, "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
