"""CPU: the references and cases of tests/_hand_pose_cases.py, before tests/test_gpu_hand_pose_shapes.py rests on them.
The references are anchored to the imported reference's recorded outputs (tests/golden/hand_opt_sequence.npz, frame 0); every
case of the GPU test's table is checked to be a useful one, and to stay inside the energy rule's exclusion cap when its terms are
formed in float32 instead of float64 (the cap is a condition on the seeds, not a measurement of the kernel)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_pose_cases as C  # noqa: E402


def test_constants_are_the_suites_own():
    """The tolerances, weights and state layout this file's helper repeats are those of tests/test_gpu_hand_pose.py, the
    optimiser and include/pn2_ext.h."""
    import test_gpu_hand_pose as G
    from models.optimization_hand import gf_optimize_hand_pose
    assert (C.GEOM_TOL, C.E_TOL, C.KP_TOL, C.R_TOL, C.THETA_TOL) == (G.GEOM_TOL, G.E_TOL, G.KP_TOL, G.R_TOL, G.THETA_TOL)
    assert C.ENERGY_WEIGHT == G.ENERGY_WEIGHT and G.SIL_STEP == C.ENERGY_WEIGHT["sil_loss"] / 778
    opt = gf_optimize_hand_pose({"device": "cpu", "opt": {"energy_weight": dict(C.ENERGY_WEIGHT)}}, hand_model=C.SyntheticLBSHand(),
                                particle_size=4)
    assert (opt.scaling_coefficient2, opt.beta, opt.theta_scale) == (C.C2, C.BETA, C.THETA_SCALE)
    with open(os.path.join(C.ROOT, "include", "pn2_ext.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    layout = (f"state, 90 floats: [{C.S_R},{C.S_T}) curr_r row-major, [{C.S_T},{C.S_THETA}) curr_t, [{C.S_THETA},{C.S_SEARCH}) "
              f"curr_theta, [{C.S_SEARCH},{C.S_PREV}) search size, [{C.S_PREV},{C.S_PREV_OK}) previous search size, "
              f"[{C.S_PREV_OK}] previous success")
    assert layout in header
    assert C.pack_state(torch.eye(3), torch.zeros(3), torch.zeros(45), torch.ones(16)).shape == (90,)


def _first_edge_candidate(case, verts):
    """A candidate with a vertex on a pixel's edge across which the mask changes, and one with none."""
    lo, hi = C.silhouette_count_range(case, verts)
    return int(torch.nonzero(hi > lo)[0]), int(torch.nonzero(hi == lo)[0]), lo, hi


def test_the_energy_rule_binds():
    """A wrong energy fails whatever P is; a silhouette pixel is accepted only for a candidate that has a vertex on a pixel's
    edge, and only in the direction that vertex can move the count; a voxel's worth only between adjacent voxels' values."""
    step = C.ENERGY_WEIGHT["sil_loss"] / 70
    assert step > 10 * C.E_TOL
    for name in ("one-candidate", "ragged-5"):
        case = C.get_case(name)
        verts, kp = C.reference_geometry(case)
        terms = C.reference_terms(case, verts, kp)
        sil = C.ENERGY_WEIGHT["sil_loss"] / case.V
        for off in (3e-5, 1e-3, sil, -sil, 0.37 * sil, 1.0):
            wrong = terms["energy"].double().numpy().copy()
            wrong[-1] += off
            with pytest.raises(AssertionError, match="explains"):
                C.assert_energies(wrong, terms, case, verts, f"{name} with candidate {case.P - 1} off by {off:g}")
    case = C.get_case("limit-8192-fp16")
    verts, kp = C.reference_geometry(case)
    terms = C.reference_terms(case, verts, kp)
    on, none, lo, hi = _first_edge_candidate(case, verts)
    e = terms["energy"].double().numpy()
    count = int(round(float(terms["silhouette"][on]) * case.V))
    assert lo[on] <= count <= hi[on] and hi[on] - lo[on] <= 2
    for q, k, ok in ((on, int(hi[on]) - count, True), (on, int(lo[on]) - count, True), (on, int(hi[on]) - count + 1, False),
                     (on, int(lo[on]) - count - 1, False), (none, 1, False), (none, -1, False)):
        if k == 0:
            continue
        moved = e.copy()
        moved[q] += k * step
        if ok:
            C.assert_energies(moved, terms, case, verts, f"candidate {q} with {k:+d} pixels on an edge")
        else:
            with pytest.raises(AssertionError, match="explains"):
                C.assert_energies(moved, terms, case, verts, f"candidate {q} with {k:+d} pixels it cannot have")
    # voxels: a vertex moved onto a voxel's face may take the neighbour's value, and no other
    one = C.get_case("one-candidate")
    v1, k1 = C.reference_geometry(one)
    t1 = C.reference_terms(one, v1, k1)
    pens, attrs = C.sdf_term_alternatives(one, v1[0])
    assert pens == [float(t1["penetration"][0])] and attrs == [float(t1["attraction"][0])]
    o = (v1[0] - one.obj_t.double()) @ one.obj_r.double()
    deepest = int(C.sdf_torch.lookup(SimpleNamespace(obj_t=one.obj_t.double().reshape(1, 1, 3), obj_r=one.obj_r.double(),
                                                     volume_size=one.res, voxel_scale=one.voxel_scale, sdf_volume=one.volume),
                                     v1)[0][0].argmin())
    o[deepest, 0] = torch.floor(o[deepest, 0] / one.voxel_scale) * one.voxel_scale + 1e-7  # just inside its voxel's lower face
    moved = (o @ one.obj_r.double().t() + one.obj_t.double())[None]
    t2 = C.reference_terms(one, moved, k1)
    pens2, _ = C.sdf_term_alternatives(one, moved[0])
    assert len(pens2) == 2 and float(t2["penetration"][0]) in pens2
    other = [p for p in pens2 if p != float(t2["penetration"][0])][0]
    assert abs(other - float(t2["penetration"][0])) > 10 * C.E_TOL           # a voxel's difference is far above the tolerance
    shifted = t2["energy"].double().numpy() + (other - float(t2["penetration"][0]))
    C.assert_energies(shifted, t2, one, moved, "the deepest vertex looked up across the face it sits on")
    with pytest.raises(AssertionError, match="explains"):
        C.assert_energies(shifted + 0.5 * (other - float(t2["penetration"][0])), t2, one, moved, "half a voxel's difference more")


def test_reference_terms_reproduce_the_fixture_energies():
    case, g = C.fixture_case(0)
    verts, kp = C.reference_geometry(case)
    assert verts.shape == (768, 778, 3) and kp.shape == (768, 21, 3) and verts.dtype == torch.float64
    assert C.energy_cap(768) == 2
    for dt in (torch.float64, torch.float32):
        terms = C.reference_terms(case, verts.to(dt), kp.to(dt))
        assert terms["gate"] and bool((terms["penetration"] > 0).all())
        np.testing.assert_allclose(terms["penetration"].float().numpy(), g["e0_penetration"], rtol=0, atol=1e-6)
        C.assert_energies(g["e0_energy"], terms, case, verts.to(dt), f"the recorded energies vs reference_terms ({dt})")


def test_reference_update_reproduces_the_fixture_frame():
    case, g = C.fixture_case(0)
    state = case.state
    for it in range(5):
        at = C.with_state(case, state)
        energy = C.reference_terms(at, *C.reference_geometry(at))["energy"].float()
        new, trace = C.reference_update(state, case.pre, energy, C.C2, C.BETA, case.tables["comps"])
        assert trace.shape == (19,) and float(trace[0]) == float(energy[0]) and torch.equal(trace[3:], new[C.S_SEARCH:C.S_SEARCH + 16])
        state = new.float()
    dR = float((new[C.S_R:C.S_R + 9].view(3, 3) - torch.from_numpy(g["f0_R"]).double()).abs().max())
    dt = float((new[C.S_T:C.S_T + 3] - torch.from_numpy(g["f0_t"]).double().reshape(3)).abs().max())
    dth = float((new[C.S_THETA:C.S_THETA + 45] - torch.from_numpy(g["f0_theta"]).double().reshape(45)).abs().max())
    print(f"reference_update over frame 0: rotation {dR:.3e}, translation {dt:.3e}, pose code {dth:.3e}")
    assert dR <= C.R_TOL and dt <= C.KP_TOL and dth <= C.THETA_TOL


def test_reference_update_without_a_better_candidate():
    case = C.update_case(1)
    state = case.state.clone()
    state[C.S_PREV:C.S_PREV + 16] = 0.008
    new, trace = C.reference_update(state, case.pre, torch.tensor([0.25]), C.C2, C.BETA, case.tables["comps"])
    keep = [i for i in range(90) if not C.S_SEARCH <= i < C.S_PREV and i != C.S_PREV_OK]
    assert torch.equal(new[keep], state.double()[keep]) and float(new[C.S_PREV_OK]) == 0 and float(trace[2]) == 0
    want = 0.25 * C.C2 * 1e-3 / (4e-3) + 1e-3  # update_seach_size at a zero mean transform: s = 1e-3 in all 16, |s| = 4e-3
    assert torch.allclose(new[C.S_SEARCH:C.S_PREV], torch.full((16,), want, dtype=torch.float64), rtol=1e-12)
    # equal energies are not better
    new2, trace2 = C.reference_update(state, torch.zeros(3, 16), torch.tensor([0.25, 0.25, 0.3]), C.C2, C.BETA, case.tables["comps"])
    assert float(trace2[2]) == 0 and torch.equal(new2, new)


@pytest.mark.parametrize("K", [1, 3, 4])
def test_rewritten_skinning_tables(K):
    t2, t = C.skinning_tables_for(778, 2), C.skinning_tables_for(778, K)
    idx, w = t["skin_idx"], t["skin_w"]
    assert idx.shape == (778, K) and w.shape == (778, K) and int(idx.min()) >= 0 and int(idx.max()) <= 20
    assert float((w.sum(dim=1) - 1).abs().max()) <= 1e-6 and torch.equal(t["tips"], t2["tips"])
    g = torch.Generator().manual_seed(3)
    pose = torch.cat([torch.randn(4, 3, generator=g, dtype=torch.float64), torch.rand(4, 45, generator=g, dtype=torch.float64) - 0.5], dim=1)
    v2, _ = C.lbs_forward_from_tables(t2, pose, torch.zeros(4, 3, dtype=torch.float64))
    v, _ = C.lbs_forward_from_tables(t, pose, torch.zeros(4, 3, dtype=torch.float64))
    if K == 1:
        dom = t2["skin_w"].argmax(dim=1, keepdim=True)
        assert torch.equal(idx, t2["skin_idx"].gather(1, dom)) and bool((w == 1).all())
        return
    other = (idx[:, 2:] != idx[:, 1:2]).all(dim=1) & (w[:, 2:] > 0).all(dim=1)
    assert int(other.sum()) * 3 >= 778                                     # other joints, with weight, for at least a third
    assert sorted(idx[:, 2:].unique().tolist()) == list(range(21))        # every 5-bit value a joint can take, in the upper fields
    assert float((v[:, 1::2] - v2[:, 1::2]).abs().max()) <= 1e-7          # the odd vertices are where the K = 2 hand has them
    assert float((v[:, 0::2] - v2[:, 0::2]).abs().max()) >= 1e-3          # the even ones are not


@pytest.mark.parametrize("V", [1, 7, 21])
def test_every_finger_owns_a_tip_vertex_at_small_vertex_counts(V):
    t = C.skinning_tables_for(V, 2)
    offs = t["finger_offsets"].tolist()
    assert all(offs[f + 1] > offs[f] for f in range(5)) and int(t["tips"].max()) < V and offs[5] == t["tips"].numel()


@pytest.mark.parametrize("name", C.EVAL_CASES)
def test_every_table_case_is_a_useful_one(name):
    case = C.get_case(name)
    spec = C.eval_case_specs()[name]
    assert (case.P, case.V, case.K, case.res, case.volume.dtype) == (spec["P"], spec["V"], spec["K"], spec["res"], spec["vol_dtype"])
    assert case.pre.shape == (case.P, 16) and not case.pre[0].any() and case.mask.shape == (case.h, case.w)
    assert case.volume.shape == (case.res,) * 3 and bool(torch.isfinite(case.volume).all())
    assert float((case.pre[:, :3] * 0.005).pow(2).sum(dim=1).max()) < 0.01        # the quaternion argument stays positive
    offs = case.tables["finger_offsets"].tolist()
    assert all(offs[f + 1] > offs[f] for f in range(5))                           # every finger has a tip vertex
    verts, kp = C.reference_geometry(case)
    r64 = C.reference_terms(case, verts, kp)
    r32 = C.reference_terms(case, verts.float(), kp.float())
    e = r64["energy"].double()
    assert bool(torch.isfinite(e).all())
    if name == "gate-off":
        assert float(r64["penetration"][0]) == 0 and not r64["gate"] and torch.equal(r64["energy"], r64["base"])
        assert float(r64["attraction"].min()) > 100 * C.E_TOL                     # the term that must disappear is a large one
    else:
        assert float(r64["penetration"][0]) > 0.005 and r64["gate"]               # candidate 0 penetrates
    if case.P > 1:
        assert int((e < e[0] - 1e-4).sum()) >= 1 and int((e > e[0] + 1e-4).sum()) >= 1
    sil = r64["silhouette"]
    assert 0.1 < float(sil[0]) < 0.95 and int(case.mask.sum()) not in (0, case.mask.numel())
    if case.vis.all() or case.res == 1:
        assert float(r64["attraction"].abs().max()) == 0
    else:
        assert float(r64["attraction"].max()) > 10 * C.E_TOL                      # attraction is formed
    x = verts[..., 0] / verts[..., 2] * case.proj["fx"] + case.proj["cx"]
    y = verts[..., 1] / verts[..., 2] * case.proj["fy"] + case.proj["cy"]
    off = [int((x < 0).sum()), int((x >= case.w).sum()), int((y < 0).sum()), int((y >= case.h).sum())]
    if name in ("off-image", "behind-camera"):
        assert min(off) >= 100, off                                               # vertices beyond every edge of the image
    if name == "behind-camera":
        assert int((verts[..., 2] <= 0).sum()) >= 1000 and int((verts[..., 2] > 0).sum()) >= 1000
    # the exclusion cap holds between a float32 and a float64 evaluation of the terms
    C.assert_energies(r32["energy"].numpy(), r64, case, verts, f"{name}: float32 terms vs float64 terms")


def test_second_pass_counts_follow_the_compute_units():
    assert C.second_pass_counts(256) == [3072, 3073, 3077] and C.second_pass_counts(304) == [3648, 3649, 3653]
    assert C.second_pass_counts(1024) == [8187, 8188, 8192]
    a, b = C.get_case("second-pass+0"), C.get_case("second-pass+5")
    assert torch.equal(a.pre, b.pre[:a.P]) and torch.equal(a.state, b.state) and torch.equal(a.volume, b.volume)
    assert torch.equal(a.pred_kp, b.pred_kp) and torch.equal(a.mask, b.mask)


def test_update_cases_reach_their_branches():
    big = C.update_case(8192)
    e = C.reference_energies(big)
    for P in C.UPDATE_P:
        case = C.update_case(P)
        assert torch.equal(case.pre, big.pre[:P]) and torch.equal(case.state, big.state)
        better = int((e[:P] < e[0] - 1e-4).sum())
        assert (better == 0) if P == 1 else (better >= 1), (P, better)
    best, worst = C.branch_rows(big)
    # further from candidate 0 than any rounding or a few silhouette pixels (0.1 / 70 each) could bridge
    assert float(e[0] - e[best]) > 0.01 and float(e[worst] - e[0]) > 0.01
    one = C.single_row_case(big, 1025, best, 1024)
    assert one.pre.shape == (1025, 16) and int(one.pre.any(dim=1).sum()) == 1 and torch.equal(one.pre[1024], big.pre[best])
