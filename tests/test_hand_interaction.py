"""CPU: the torch route of eval_metrics.hand_interaction_metrics against a literal per-frame loop -- the hand model's own
forward(), oracle.sdf_oracle.nearest on its vertices, plain numpy reductions -- and the tracker's switch.

The loop and the route pose the hand in float64 from the same inputs.  forward() and the skinning tables differ by d (measured here
between forward() and lbs_forward_from_tables, neither of which is under test: 1e-15 m for the plain hand, about 1e-9 m for the MANO
one, whose tables hold the regressed joints in fp32; HandModel accepts tables up to TABLES_TOL = 1e-6 m).  The oracle then looks
the fp32-rounded vertices up with fp32 arithmetic and the route the float64 ones with float64 arithmetic, so a vertex within
2e-7 m + d of a voxel face could land on either side.  The scenes are seeded and none of their vertices sits that near a face
(asserted below): the discrete columns must then be equal, the columns that are voxel values agree to 1e-9 m and the keypoint
column to 1e-9 m + d."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_interact_cases as H  # noqa: E402

from models import eval_metrics  # noqa: E402
from models.hand_model import SyntheticLBSHand, SyntheticManoHand, lbs_forward_from_tables, rodrigues  # noqa: E402

THRESHOLD = 0.005


def _literal_rows(model, tables, fr, offsets, volumes, voxel_scale):
    F = fr["MANO_theta"].shape[0]
    verts, kps = [], []
    for f in range(F):
        beta = fr["beta"][fr["rest_of"][f]][None].double() if "beta" in fr else None
        with torch.no_grad():
            v, k = model.forward(th_pose_coeffs=torch.cat([fr["global_aa"][f].double(), fr["MANO_theta"][f].double()])[None],
                                 th_trans=fr["global_translation"][f][None].double(), th_betas=beta)
        verts.append(v[0])
        kps.append(k[0])
    verts, kps = torch.stack(verts), torch.stack(kps)
    with torch.no_grad():
        tv, tk = lbs_forward_from_tables(tables, torch.cat([fr["global_aa"], fr["MANO_theta"]], dim=1).double(), fr["global_translation"].double(),
                                         fr["beta"].double()[fr["rest_of"]] if "beta" in fr else None)
    d = max(float((tv - verts).abs().max()), float((tk - kps).abs().max()))
    assert d <= type(model).TABLES_TOL
    # no vertex within 2e-7 m + d of a voxel face: the fp32 rounding of a coordinate below 0.6 m (3e-8), of its difference to the object and
    # of the three products of the rotation (see the module docstring); a seed that puts one there is refused, not compared
    o = torch.matmul(verts - fr["obj_translation"].double()[:, None], fr["obj_rotation"].double()) / voxel_scale
    half = volumes[0].shape[0] // 2
    near = ((o - o.round()).abs() * voxel_scale < 2e-7 + d) & (o.abs() < half + 1)
    assert not near.any(), "a seeded vertex sits on a voxel face: %d" % int(near.sum())
    rows, counts, _ = H.rows_from_vertices(tables, verts.float().numpy(), kps.float().numpy(), fr, offsets, volumes, voxel_scale, THRESHOLD)
    rows[:, 6] = (kps - fr["pred_kp"].double()).norm(dim=-1).mean(dim=1).numpy()  # (the keypoints in float64, not rounded)
    return rows, counts, d


@pytest.mark.parametrize("kind,res,dtype", [("shaped", 151, torch.float16), ("shaped", 5, torch.float32), ("mano", 151, torch.float32),
                                            ("mano", 5, torch.float16)])
def test_torch_route_against_the_literal_loop(kind, res, dtype):
    model = SyntheticLBSHand(num_verts=130, num_betas=10) if kind == "shaped" else SyntheticManoHand(num_verts=130)
    tables = model.skinning_tables()
    assert tables is not None
    fr, offsets, volumes, voxel_scale = H.make_scene(tables, res, dtype, seed=res + (kind == "mano"))
    want, counts, d = _literal_rows(model, tables, fr, offsets, volumes, voxel_scale)
    f64 = {k: (v.double() if v.is_floating_point() else v) for k, v in fr.items() if k != "global_aa"}
    f64["global_rotation"] = rodrigues(fr["global_aa"].double())  # what forward() turns the axis-angle into
    rows, seq, keys = eval_metrics.hand_interaction_metrics(f64, offsets, tables, volumes, voxel_scale, contact_threshold=THRESHOLD, route="torch")
    assert tuple(keys) == eval_metrics.HAND_INTERACTION_KEYS and rows.shape == (6, 8) and seq.shape == (3, 8) and rows.dtype == torch.float64
    got = rows.numpy().copy()
    got[:, list(H.MM)] /= 1000.0
    for c in (2, 3, 7):
        assert (got[:, c] == want[:, c]).all(), (c, got[:, c], want[:, c])
    assert (got[:, 1] == counts / tables["rest_verts"].shape[0]).all(), (got[:, 1], counts)  # (the share in float64 here)
    for c in (0, 4, 5, 6):
        assert np.abs(got[:, c] - want[:, c]).max() <= 1e-9 + (d if c == 6 else 0.0), (c, got[:, c], want[:, c])
    if res == 151:  # the scene's frames are what the module says they are
        V = tables["rest_verts"].shape[0]
        assert counts[0] == 0 and want[0, 0] == 0 and want[0, 5] > 0          # no vertex inside
        assert want[1, 2] == 1 and want[1, 3] >= 1                             # the sphere on finger 0's tip region
        assert counts[4] == V and want[4, 1] == 1.0                            # every vertex inside
        assert counts[5] == 0
    s = seq.numpy()
    assert (s[1] == 0).all()
    assert np.allclose(s[0], rows[0:4].mean(dim=0).numpy(), rtol=1e-12, atol=0) and np.allclose(s[2], rows[4:6].mean(dim=0).numpy(), rtol=1e-12, atol=0)
    # without pred_kp the column is not valid and stays zero
    del f64["pred_kp"]
    rows2, _, keys2 = eval_metrics.hand_interaction_metrics(f64, offsets, tables, volumes, voxel_scale, contact_threshold=THRESHOLD, route="torch")
    assert "hand_model_kp_diff" not in keys2 and len(keys2) == 7 and (rows2[:, 6] == 0).all()
    assert torch.equal(rows2[:, [0, 1, 2, 3, 4, 5, 7]], rows[:, [0, 1, 2, 3, 4, 5, 7]])


def test_argument_checks():
    tables = SyntheticLBSHand(num_verts=44).skinning_tables()
    fr, offsets, volumes, voxel_scale = H.make_scene(tables, 5, torch.float32, seed=1)
    with pytest.raises(ValueError):
        eval_metrics.hand_interaction_metrics(fr, [0, 4, 3, 6], tables, volumes, voxel_scale, route="torch")
    with pytest.raises(ValueError):
        eval_metrics.hand_interaction_metrics(fr, offsets, tables, volumes[:2], voxel_scale, route="torch")
    with pytest.raises(ValueError):
        eval_metrics.hand_interaction_metrics(fr, offsets, tables, [None, None, volumes[2]], voxel_scale, route="torch")
    with pytest.raises(RuntimeError):
        eval_metrics.hand_interaction_metrics(fr, offsets, tables, volumes, voxel_scale, route="kernel")


# ---- the tracker's switch --------------------------------------------------------------------------------------------------------
class _NoTables(SyntheticLBSHand):
    def _lbs_tables(self):
        return None


def _tracker(interaction, hand, fused=True):
    from _netinit import make_cfg
    from models.hand_network import HandTrackNet
    from models.track_network import HandTrackModel
    cfg = make_cfg("cpu")
    cfg.update(fused_hand_eval=fused, hand_interaction_eval=interaction, opt={"contact_threshold": 0.007})
    return HandTrackModel(cfg, handnet=HandTrackNet, hand_model=hand)


def _tracked_io(tables, lengths=(3, 2)):
    """Two sequences as the tracker hands them to compute_loss_batch (tests/_hand_eval_cases), with the object's pose per frame
    and each sequence's volume in its first frame."""
    import _hand_eval_cases as E
    frames, offsets, _ = E.make_case(lengths, True, seed=3)
    fr, _, volumes, voxel_scale = H.make_scene(tables, 21, torch.float32, seed=9, lengths=lengths, radii=(0.04, 0.2))
    ios = []
    for q, (a, b) in enumerate(zip(offsets, offsets[1:])):
        data, rets = E.tracker_io({k: v[a:b] for k, v in frames.items()}, torch.zeros(6, 3))
        for i, (d, r) in enumerate(zip(data, rets)):
            f = a + i
            d["gt_obj_pose"] = {"rotation": fr["obj_rotation"][f][None], "translation": fr["obj_translation"][f].reshape(1, 3, 1)}
            r["MANO_theta"], r["pred_kp"] = fr["MANO_theta"][f][None], fr["pred_kp"][f][None]
            r["global_pose"] = {"rotation": fr["global_rotation"][f][None], "translation": fr["global_translation"][f].reshape(1, 3, 1)}
        data[0]["sdf_volume"], data[0]["voxel_scale"] = volumes[q], voxel_scale
        ios.append((data, rets))
    return ios, fr, offsets, volumes, voxel_scale


def test_compute_loss_keys_follow_the_switch(capsys):
    hand = SyntheticLBSHand(num_verts=130)
    tables = hand.skinning_tables()
    ios, fr, offsets, volumes, voxel_scale = _tracked_io(tables)
    flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": True}
    inputs, rets = [io[0] for io in ios], [io[1] for io in ios]
    off = _tracker(False, hand).compute_loss_batch(inputs, rets, dict(flags))
    on_model = _tracker(True, hand)
    on = on_model.compute_loss_batch(inputs, rets, dict(flags))
    want = {k: v for k, v in fr.items() if k not in ("global_aa", "beta", "rest_of")}
    _, seq, keys = eval_metrics.hand_interaction_metrics(want, offsets, tables, volumes, voxel_scale, contact_threshold=0.007, route="torch")
    for q in range(2):
        assert not set(off[q][0]) & set(eval_metrics.HAND_INTERACTION_KEYS)
        assert list(on[q][0]) == list(off[q][0]) + list(eval_metrics.HAND_INTERACTION_KEYS)
        assert {k: on[q][0][k] for k in off[q][0]} == off[q][0]
        for c, k in enumerate(keys):
            assert on[q][0][k] == float(seq[q, c]), (q, k)
    # the per-sequence entry with the fused evaluation off reports the same eight values
    single = _tracker(True, hand, fused=False)  # (the per-frame dictionary needs HandTrackNet's own inputs: only the new keys here)
    extra = single.hand_interaction_losses(inputs, rets)
    assert [extra[q][k] for q in range(2) for k in keys] == [on[q][0][k] for q in range(2) for k in keys]
    assert "left out" not in capsys.readouterr().out


def test_keys_are_dropped_with_a_reason_for_a_model_without_tables(capsys):
    hand = _NoTables(num_verts=130)
    assert hand.skinning_tables() is None
    ios, *_ = _tracked_io(SyntheticLBSHand(num_verts=130).skinning_tables())
    flags = {"track_flag": True, "test_flag": True, "save_flag": False, "IKNet_flag": True}
    model = _tracker(True, hand)
    from models.track_network import HandTrackModel
    HandTrackModel._said_interaction.clear()
    out = model.compute_loss_batch([io[0] for io in ios], [io[1] for io in ios], dict(flags))
    again = model.compute_loss_batch([io[0] for io in ios], [io[1] for io in ios], dict(flags))
    said = capsys.readouterr().out
    assert said.count("hand_interaction_eval") == 1 and "no skinning tables" in said
    for (loss, _), (loss2, _) in zip(out, again):
        assert "hand_pred_kp_diff" in loss and not set(loss) & set(eval_metrics.HAND_INTERACTION_KEYS) and loss == loss2
    # results without a pose: the other reason
    ios, *_ = _tracked_io(SyntheticLBSHand(num_verts=130).skinning_tables())
    for _, rets in ios:
        for r in rets:
            del r["MANO_theta"]
    model = _tracker(True, SyntheticLBSHand(num_verts=130))
    out = model.compute_loss_batch([io[0] for io in ios], [io[1] for io in ios], dict(flags))
    assert "no MANO_theta" in capsys.readouterr().out and not set(out[0][0]) & set(eval_metrics.HAND_INTERACTION_KEYS)
