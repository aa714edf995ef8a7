"""GPU: pn2x_hand_interaction_metrics (hotrack_amd/csrc/hand_interact.hip) in two steps, so that a vertex on a voxel's edge can
neither hide nor fake a failure.

Geometry: the kernel's out_verts / out_kp against lbs_forward_from_tables in float64 with the fp32-rounded root matrix, to the
bounds the hand-pose geometry tests hold this arithmetic to: tests/_hand_pose_cases.GEOM_TOL (3e-7 m) for a plain hand and
max(3e-7, 4 x 7.4e-8) m, the bound of tests/test_gpu_hand_pose_mano.py, for a MANO-structured one.
Metrics: recomputed from the kernel's OWN vertices with oracle.sdf_oracle.nearest (bit-exact voxel on fp32 points) and numpy:
columns 0, 2, 3, 5, 7 and the share count / v must be EQUAL; columns 4 and 6 within tests/_hand_interact_cases.COL4_REL = 6 U and
COL6_REL = 13 U of their float64 value (U = 2^-24; derived there from the 5 and 21 terms); the sequence rows equal the serial
float64 mean of the kernel's float32 rows, bit for bit.
Scenes: tests/_hand_interact_cases.make_scene (S = 3 with an empty middle sequence; no vertex inside, every vertex inside,
vertices outside the volume, finger 0's whole tip region inside; two shape tables inside a sequence for a shaped hand)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_interact_cases as H  # noqa: E402
import _hand_pose_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
THRESHOLD = 0.005
MANO_GEOM_TOL = max(3e-7, 4 * 7.4e-8)
F16, F32 = torch.float16, torch.float32
#        name                 kind      V    K  res  dtype  empty finger  pred_kp
CASES = {"plain-22-k1":      ("plain", 22, 1, 5, F32, None, True),
         "plain-65-k4":      ("plain", 65, 4, 151, F16, None, True),
         "plain-257-k1":     ("plain", 257, 1, 151, F32, None, True),
         "shaped-257-k2":    ("shaped", 257, 2, 151, F16, None, True),
         "plain-778-k4":     ("plain", 778, 4, 5, F16, None, True),
         "plain-1024-k4":    ("plain", 1024, 4, 151, F16, None, True),
         "mano-22-k4":       ("mano", 22, 4, 151, F32, None, True),
         "mano-65-k1":       ("mano", 65, 1, 5, F16, None, True),
         "mano-257-k4":      ("mano", 257, 4, 151, F16, None, True),
         "mano-778-k4":      ("mano", 778, 4, 151, F32, None, True),
         "mano-1024-k1":     ("mano", 1024, 1, 5, F32, None, True),
         "empty-finger":     ("plain", 65, 1, 151, F16, 2, True),
         "no-pred-kp":       ("mano", 97, 4, 151, F16, None, False)}
_BUILT = {}


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _run(tables, fr, offsets, volumes, voxel_scale, **kw):
    """ext.hand_interaction_metrics on the scene's CPU tensors -> (rows, seq, mask, verts, kp) on the GPU."""
    from hotrack_amd import ext
    dev = "cuda"
    model = ext.hand_pose_model(tables, dev)
    d = lambda x: x.to(dev).contiguous()
    if "beta" in fr:
        G = fr["beta"].shape[0]
        rest = ((model["rest_joints"][None] + (d(fr["beta"]) @ model["shape_joints"]).view(G, -1, 3)).contiguous(),
                (model["rest_verts"][None] + (d(fr["beta"]) @ model["shape_verts"]).view(G, -1, 3)).contiguous())
        rest_of = d(fr["rest_of"].to(torch.int32))
    else:
        rest = (model["rest_joints"][None].contiguous(), model["rest_verts"][None].contiguous())
        rest_of = torch.zeros(fr["MANO_theta"].shape[0], dtype=torch.int32, device=dev)
    out = ext.hand_interaction_metrics(model, d(fr["global_rotation"]), d(fr["global_translation"]), d(fr["MANO_theta"]),
                                       d(fr["obj_rotation"]), d(fr["obj_translation"]), rest, rest_of,
                                       [None if v is None else d(v) for v in volumes], voxel_scale, offsets, THRESHOLD,
                                       pred_kp=d(fr["pred_kp"]) if "pred_kp" in fr else None, with_geometry=True, **kw)
    torch.cuda.synchronize()
    return out


def _case(name):
    """The case's scene (CPU, read-only), its float64 geometry and the kernel's results: built and run once, shared."""
    if name not in _BUILT:
        kind, V, K, res, dt, empty, with_kp = CASES[name]
        tables, _ = H.hand_tables(kind, V, K, empty_finger=empty)
        fr, offsets, volumes, vs = H.make_scene(tables, res, dt, seed=list(CASES).index(name), with_pred_kp=with_kp)
        ref = H.reference_geometry(tables, fr)
        got = _run(tables, fr, offsets, volumes, vs)
        _BUILT[name] = (tables, fr, offsets, volumes, vs, ref, got)
    return _BUILT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_geometry_against_float64(name):
    tables, fr, offsets, volumes, vs, (rv, rk), (rows, seq, mask, verts, kp) = _case(name)
    kind = CASES[name][0]
    tol = MANO_GEOM_TOL if kind == "mano" else C.GEOM_TOL
    F = fr["MANO_theta"].shape[0]
    assert verts.shape == rv.shape and kp.shape == (F, 21, 3) and verts.dtype == torch.float32
    dv = float((verts.double().cpu() - rv).abs().max())
    dk = float((kp.double().cpu() - rk).abs().max())
    print(f"{name}: max |vertex - float64| = {dv:.3e} m, keypoints {dk:.3e} m (bound {tol:.1e})")
    assert torch.isfinite(verts).all() and dv <= tol and dk <= tol
    if "beta" in fr:  # the two shape tables give different hands (rest_of is read)
        assert float((rv[0] - rv[1]).abs().max()) > 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_metrics_from_the_kernels_own_vertices(name):
    tables, fr, offsets, volumes, vs, _, (rows, seq, mask, verts, kp) = _case(name)
    kind, V, K, res, dt, empty, with_kp = CASES[name]
    assert mask == (0xff if with_kp else 0xbf) and rows.shape == (6, 8) and seq.shape == (3, 8)
    want, counts, sdfs = H.rows_from_vertices(tables, verts.cpu().numpy(), kp.cpu().numpy(), fr, offsets, volumes, vs, THRESHOLD)
    got = rows.cpu().numpy()
    print(f"{name}: inside counts {counts.tolist()}, fingers in contact {want[:, 3].tolist()}")
    for c in (0, 2, 3, 5, 7):
        assert (got[:, c] == want[:, c].astype(np.float32)).all() and (got[:, c].astype(np.float64) == want[:, c]).all(), (c, got[:, c], want[:, c])
    assert (got[:, 1] == (counts.astype(np.float32) / np.float32(V))).all(), (got[:, 1], counts)
    for c, rel in ((4, H.COL4_REL), (6, H.COL6_REL)):
        err = np.abs(got[:, c].astype(np.float64) - want[:, c])
        print(f"{name}: column {c} max relative error {np.max(err / np.maximum(want[:, c], 1e-30)):.3e} (bound {rel:.3e})")
        assert (err <= rel * np.abs(want[:, c])).all(), (c, got[:, c], want[:, c])
    if not with_kp:
        assert (got[:, 6] == 0).all()
    # the reduce launch: the serial float64 mean of the float32 rows, an empty sequence zero
    assert np.array_equal(_bits(seq), H.sequence_means(got, offsets).view(np.int32))
    assert (seq[1] == 0).all()
    # the scene is what it says it is
    if res == 151:
        half = (res // 2) * vs
        o = [(verts[f].double().cpu() - fr["obj_translation"][f].double()) @ fr["obj_rotation"][f].double() for f in range(6)]
        assert counts[0] == 0 and got[0, 0] == 0 and got[0, 2] == 0 and got[0, 5] > 0                 # no vertex inside
        assert (o[2].abs() > half + vs).any() and (o[5].abs() > half + vs).any()                        # clamped indices
        assert counts[4] == V and got[4, 1] == 1.0 and got[4, 5] < 0                                  # every vertex inside
        offs = [int(x) for x in tables["finger_offsets"]]
        region0 = tables["tips"][offs[0]:offs[1]].numpy()
        if len(region0) and V >= 65:
            assert sdfs[1][region0].max() < 0 and got[1, 3] >= 1 and got[1, 7] == 1                    # finger 0's whole region inside
    if empty is not None:  # a finger without a tip region is never in contact and not in the mean: at most four count
        assert got[:, 3].max() <= 4 and got[4, 3] == 4
    assert np.isfinite(got).all()


def test_sequences_alone_in_the_batch_and_twice():
    name = "shaped-257-k2"
    tables, fr, offsets, volumes, vs, _, (rows, seq, mask, verts, kp) = _case(name)
    again = _run(tables, fr, offsets, volumes, vs)
    for a, b in zip((rows, seq, verts, kp), (again[0], again[1], again[3], again[4])):
        assert np.array_equal(_bits(a), _bits(b))                                  # two runs: the same bits
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b == a:
            continue
        alone = {k: (v if k == "beta" else v[a:b]) for k, v in fr.items()}
        assert len(set(alone["rest_of"].tolist())) == 2                            # two shape tables inside the sequence
        r1, s1, _, v1, _ = _run(tables, alone, [0, b - a], [volumes[q]], vs)
        assert np.array_equal(_bits(r1), _bits(rows[a:b])) and np.array_equal(_bits(s1[0]), _bits(seq[q])), q
        assert np.array_equal(_bits(v1), _bits(verts[a:b]))
    one = {k: (v if k == "beta" else v[1:2]) for k, v in fr.items()}               # F = 1
    r1, s1, _, _, _ = _run(tables, one, [0, 1], [volumes[0]], vs)
    assert np.array_equal(_bits(r1[0]), _bits(rows[1])) and np.array_equal(_bits(s1[0]), _bits(rows[1]))
    # sequences that are all empty but one, in another order of volumes
    r2, s2, _, _, _ = _run(tables, {k: (v if k == "beta" else v[4:6]) for k, v in fr.items()}, [0, 0, 2, 2], [None, volumes[2], None], vs)
    assert np.array_equal(_bits(r2), _bits(rows[4:6])) and np.array_equal(_bits(s2[1]), _bits(seq[2])) and (s2[[0, 2]] == 0).all()


def test_graph_capture_replays_to_the_same_bits():
    from hotrack_amd import ext
    name = "mano-257-k4"
    tables, fr, offsets, volumes, vs, _, (rows, seq, mask, verts, kp) = _case(name)
    dev = "cuda"
    model = ext.hand_pose_model(tables, dev)
    d = lambda x: x.to(dev).contiguous()
    G = fr["beta"].shape[0]
    rest = ((model["rest_joints"][None] + (d(fr["beta"]) @ model["shape_joints"]).view(G, -1, 3)).contiguous(),
            (model["rest_verts"][None] + (d(fr["beta"]) @ model["shape_verts"]).view(G, -1, 3)).contiguous())
    buf = {k: d(fr[k]) for k in ("global_rotation", "global_translation", "MANO_theta", "obj_rotation", "obj_translation", "pred_kp")}
    vols = [None if v is None else d(v) for v in volumes]
    seq_off = torch.tensor(offsets, dtype=torch.int32, device=dev)
    table = torch.tensor([0 if v is None else v.data_ptr() for v in vols], dtype=torch.int64, device=dev)
    rest_of = d(fr["rest_of"].to(torch.int32))
    call = lambda: ext.hand_interaction_metrics(model, buf["global_rotation"], buf["global_translation"], buf["MANO_theta"], buf["obj_rotation"],
                                                buf["obj_translation"], rest, rest_of, vols, vs, offsets, THRESHOLD, pred_kp=buf["pred_kp"],
                                                seq_off=seq_off, vol_table=table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # two kernels on one stream: a linear graph
        g_rows, g_seq, _, _, _ = call()
    other = (0.2 * torch.randn(fr["MANO_theta"].shape, generator=torch.Generator().manual_seed(5))).float()
    buf["MANO_theta"].copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    moved = g_rows.clone()
    direct = call()[0]
    assert np.array_equal(_bits(moved), _bits(direct)) and not np.array_equal(_bits(moved), _bits(rows))   # the replay follows the buffers
    buf["MANO_theta"].copy_(fr["MANO_theta"])
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(g_rows), _bits(rows)) and np.array_equal(_bits(g_seq), _bits(seq))


def test_eval_metrics_kernel_route_and_units():
    from models import eval_metrics
    tables, fr, offsets, volumes, vs, _, (rows, seq, mask, verts, kp) = _case("shaped-257-k2")
    dev = {k: v.cuda() for k, v in fr.items() if k != "global_aa"}
    r, s, keys = eval_metrics.hand_interaction_metrics(dev, offsets, tables, [None if v is None else v.cuda() for v in volumes], vs,
                                                       contact_threshold=THRESHOLD, route="kernel")
    unit = torch.ones(8, device="cuda")
    unit[list(H.MM)] = 1000.0
    assert tuple(keys) == eval_metrics.HAND_INTERACTION_KEYS
    assert torch.equal(r, rows * unit) and torch.equal(s, seq * unit)
    with pytest.raises(RuntimeError):  # CPU volumes cannot take the kernel route
        eval_metrics.hand_interaction_metrics(dev, offsets, tables, volumes, vs, route="kernel")


# ---- end to end: a tracked synthetic hand-object sequence (the small settings of tests/test_gpu_hand_track_batch.py) -----------------
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}
LENGTHS = (4, 3, 2)


class OracleNet(torch.nn.Module):
    """Ground-truth keypoints plus 2 mm of noise seeded by the frame's name, in an identity hand frame."""

    def __init__(self, cfg):
        super().__init__()
        self.device = cfg["device"]

    def forward(self, data, flags):
        s, k = data["file_name"][0].split("_")[-1].split("/")
        g = torch.Generator(device="cuda").manual_seed(1000 * int(s) + int(k))
        kp = data["gt_hand_kp"].to(self.device) + 0.002 * torch.randn(1, 21, 3, device=self.device, generator=g)
        vis = torch.ones(1, 21, dtype=torch.bool, device=self.device)
        vis[0, [8, 20]] = int(k) % 2 == 0
        eye = {"rotation": torch.eye(3, device=self.device)[None], "translation": torch.zeros(1, 3, 1, device=self.device),
               "scale": torch.ones(1, device=self.device)}
        return {"pred_kp": kp, "pred_kp_vis_mask": vis, "pred_kp_handframe": kp.transpose(-1, -2).contiguous(),
                "init_kp_handframe": kp.transpose(-1, -2).contiguous(), "canon_pose": eye}

    def compute_loss(self, data, ret, flags):
        return {"hand_pred_kp_diff": (ret["pred_kp"] - data["gt_hand_kp"].to(self.device)).norm(dim=-1).mean()}, ret


def _tracker(hm, interaction):
    from models.track_network import HandTrackModel
    cfg = {"device": torch.device("cuda", 0), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
           "use_optimization": True, "use_pred_hand_shape": 1, "hand_particles": 256, "shape_particles": 256, "hand_model": hm,
           "hand_interaction_eval": interaction, "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": True, "contact_threshold": 0.006}}
    model = HandTrackModel(cfg, handnet=OracleNet, hand_model=hm).eval()
    assert model.optimizer.use_kernel()
    model.use_graph = False
    return model, cfg


def test_tracked_sequences_report_the_interaction_columns():
    from datasets.synthetic import SyntheticHandObjectSequences
    from models import eval_metrics
    from models.hand_model import SyntheticLBSHand
    hm = SyntheticLBSHand(num_betas=10)
    model, cfg = _tracker(hm, True)
    ds = SyntheticHandObjectSequences(cfg, 3, max(LENGTHS), res=41, stride=0.01, hand_beta=1.0)
    seqs = [ds[s][:n] for s, n in enumerate(LENGTHS)]
    for seq in seqs:  # (these sequences' mano_pose is the 45 joint angles alone: MANO_theta_diff, which expects 48, is not this test's)
        for d in seq:
            d["gt_hand_pose"].pop("mano_pose", None)
    with torch.no_grad():
        rets = model.forward_batch(copy.deepcopy(seqs), dict(FLAGS))
        got = model.compute_loss_batch(seqs, rets, dict(FLAGS))
        model.hand_interaction_eval = False
        plain = model.compute_loss_batch(seqs, rets, dict(FLAGS))
        model.hand_interaction_eval = True
        per_seq = [model.compute_loss(seq, r, dict(FLAGS))[0] for seq, r in zip(seqs, rets)]
    keys = eval_metrics.HAND_INTERACTION_KEYS
    tables = hm.skinning_tables()
    for q, (seq_in, r) in enumerate(zip(seqs, rets)):
        loss = got[q][0]
        assert list(loss) == list(plain[q][0]) + list(keys) and {k: loss[k] for k in plain[q][0]} == plain[q][0]
        assert [per_seq[q][k] for k in keys] == [loss[k] for k in keys]             # the per-sequence entry: the same call on one sequence
        # the torch route on the same results, in float64 on the CPU
        f64 = lambda x, *s: torch.cat([torch.as_tensor(t).detach().cpu().double().reshape(1, *s) for t in x])
        codes = {}
        for x in r:
            codes.setdefault(id(x["pred_beta"]), x["pred_beta"])
        frames = {"MANO_theta": f64([x["MANO_theta"] for x in r], 45), "global_rotation": f64([x["global_pose"]["rotation"] for x in r], 3, 3),
                  "global_translation": f64([x["global_pose"]["translation"] for x in r], 3),
                  "obj_rotation": f64([d["gt_obj_pose"]["rotation"] for d in seq_in], 3, 3),
                  "obj_translation": f64([d["gt_obj_pose"]["translation"] for d in seq_in], 3),
                  "pred_kp": f64([x["pred_kp"] for x in r], 21, 3), "beta": f64(list(codes.values()), 10),
                  "rest_of": torch.tensor([list(codes).index(id(x["pred_beta"])) for x in r])}
        vol, vs = seq_in[0]["sdf_volume"], float(seq_in[0]["voxel_scale"])
        rows, want, wkeys = eval_metrics.hand_interaction_metrics(frames, [0, len(r)], tables, [vol.cpu()], vs, contact_threshold=0.006, route="torch")
        assert tuple(wkeys) == keys
        want = want[0].numpy()
        print("sequence %d: %s" % (q, {k: (loss[k], float(w)) for k, w in zip(keys, want)}))
        for c, k in enumerate(keys):
            # the mean of n frames rounded to fp32 (2 U), on top of the per-frame bounds: equal values for the discrete and
            # voxel-valued columns, COL4_REL / COL6_REL, and for column 6 the geometry's own GEOM_TOL (the torch route poses
            # the hand itself; in millimetre columns the unit is 1e-3 m)
            rel = 2 * H.U + (H.COL4_REL if c == 4 else H.COL6_REL if c == 6 else 0.0)
            extra = C.GEOM_TOL if c == 6 else 0.0
            assert abs(loss[k] - want[c]) <= rel * abs(want[c]) + extra, (q, k, loss[k], want[c])
    assert any(got[q][0]["hand_contact_frames"] > 0 or got[q][0]["hand_pen_frames"] > 0 for q in range(3))  # the hands do touch the object
