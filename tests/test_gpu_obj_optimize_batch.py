"""GPU: the batched particle loop (hotrack_amd.sdf.obj_optimize_batch -> pn2s_obj_optimize_batch, hotrack_amd/csrc/sdf.hip):
S independent problems per launch.  Its oracle is the single-problem route (sdf.obj_optimize, pinned to the reference by
tests/test_gpu_sdf.py): both run the same device code in the same accumulation order, so every comparison with it is an
equality of bits, not a tolerance.  Small shapes: a 41^3 volume, at most 1000 points, 256 / 300 particles."""
import os

import numpy as np
import pytest
import torch

from _sdf_cases import _axis_angle, make_volume, object_points, random_pose

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES, STRIDE = 41, 0.01
SHAPES = ("sphere", "box", "capsule")
SIZES = (1, 255, 257, 1000, 64)   # one point; one short of / one over the block's 256 threads; several strides; a quarter block


@pytest.fixture(scope="module")
def sdf():
    from hotrack_amd import sdf as m
    return m


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _pre(p, seed=3):
    pre = np.random.default_rng(seed).standard_normal((p, 6)).astype(np.float32)
    pre[0] = 0
    return _d(pre)


@pytest.fixture(scope="module")
def world(sdf):
    """Volumes of three shapes in every layout, and five problems (cloud, initial pose) cycling through them.  Read-only."""
    vols = {}
    for dt in (np.float16, np.float32):
        lin = [_d(make_volume(RES, STRIDE, sh, dt)) for sh in SHAPES]
        vols[("linear", dt)] = lin
        vols[("corner", dt)] = [sdf.CornerVolume(v) for v in lin]
    probs = []
    for k, n in enumerate(SIZES):
        shape = SHAPES[k % 3]
        R0, t0 = random_pose(100 + k)
        cam = (object_points(200 + k, n, shape) @ R0.T + t0).astype(np.float32)
        rng = np.random.default_rng(300 + k)
        Ri = (R0.astype(np.float64) @ _axis_angle(rng.standard_normal(3), 0.04)).astype(np.float32)   # a few degrees / mm off
        ti = (t0 + rng.normal(0, 0.004, 3)).astype(np.float32)
        probs.append((_d(cam), _d(Ri), _d(ti)))
    return {"vols": vols, "probs": probs, "singles": {}}


def _single(sdf, world, k, vol, pre, iters, tag):
    """Problem k alone through sdf.obj_optimize -> (R bits, t bits); computed once per distinct request."""
    key = (k, tag, pre.shape[0], iters)
    if key not in world["singles"]:
        cam, R, t = world["probs"][k]
        Rs, ts = sdf.obj_optimize(cam, R, t, pre, vol, STRIDE, iterations=iters)
        world["singles"][key] = (_bits(Rs.reshape(3, 3)), _bits(ts.reshape(3)))
    return world["singles"][key]


def _stack(world, ks):
    return (torch.stack([world["probs"][k][1] for k in ks]), torch.stack([world["probs"][k][2] for k in ks]))


def _check_equal_singles(sdf, world, R, t, ks, vols, pre, iters, tag):
    for j, k in enumerate(ks):
        Rb, tb = _single(sdf, world, k, vols[j], pre, iters, tag)
        assert np.array_equal(_bits(R[j]), Rb), f"rotation of problem {k} (slot {j})"
        assert np.array_equal(_bits(t[j].reshape(3)), tb), f"translation of problem {k} (slot {j})"


@pytest.mark.parametrize("layout,dt", [("corner", np.float16), ("linear", np.float16), ("corner", np.float32)])
@pytest.mark.parametrize("iters", [0, 1, 4, 10])
@pytest.mark.parametrize("p", [256, 300])
def test_batch_equals_single_calls_bit_for_bit(sdf, world, p, iters, layout, dt):
    pre = _pre(p)
    ks = list(range(5))
    vols = [world["vols"][(layout, dt)][k % 3] for k in ks]
    R0, t0 = _stack(world, ks)
    R, t = sdf.obj_optimize_batch([world["probs"][k][0] for k in ks], R0, t0, pre, vols, STRIDE, iterations=iters)
    assert R.shape == (5, 3, 3) and t.shape == (5, 3, 1) and R.data_ptr() != R0.data_ptr()
    _check_equal_singles(sdf, world, R, t, ks, vols, pre, iters, (layout, dt))
    if iters == 0:
        assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(t.reshape(5, 3)), _bits(t0))
    else:
        assert not np.array_equal(_bits(R), _bits(R0))   # (the problems are live: something moved)


def test_batch_of_one_equals_single_and_the_reference_vectors(sdf):
    z = np.load(os.path.join(G, "sdf_optimize.npz"))
    _, stride = z["o0_meta"]
    args = (_d(z["o0_pcld"]), _d(z["o0_R_init"]), _d(z["o0_t_init"]), _d(z["o0_pre"]))
    vol = _d(z["o0_vol"])
    Rs, ts = sdf.obj_optimize(*args, vol, float(stride))
    R, t = sdf.obj_optimize_batch([args[0]], args[1].reshape(1, 3, 3), args[2].reshape(1, 3), args[3], [vol], float(stride))
    assert np.array_equal(_bits(R), _bits(Rs)) and np.array_equal(_bits(t), _bits(ts))
    np.testing.assert_allclose(R.cpu().numpy()[0], z["o0_R_ref"], rtol=0, atol=2e-5)            # gf_optimize_obj.optimize
    np.testing.assert_allclose(t.cpu().numpy().reshape(3), z["o0_t_ref"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("empty", ["empty tensor", "None"])
def test_inactive_problems_keep_their_pose(sdf, world, empty):
    pre, ks = _pre(300), list(range(5))
    vols = [world["vols"][("corner", np.float16)][k % 3] for k in ks]
    clouds = [world["probs"][k][0] for k in ks]
    for k in (1, 3):
        clouds[k] = torch.empty((0, 3), device="cuda") if empty == "empty tensor" else None
        vols[k] = None
    R0, t0 = _stack(world, ks)
    R, t = sdf.obj_optimize_batch(clouds, R0, t0, pre, vols, STRIDE, iterations=4)
    for k in (1, 3):
        assert np.array_equal(_bits(R[k]), _bits(R0[k])) and np.array_equal(_bits(t[k].reshape(3)), _bits(t0[k]))
    live = [0, 2, 4]
    _check_equal_singles(sdf, world, R[live], t[live], live, [vols[k] for k in live], pre, 4, ("corner", np.float16))
    # nothing active at all: the poses come back as they went in
    R, t = sdf.obj_optimize_batch([None] * 5, R0, t0, pre, [None] * 5, STRIDE, iterations=4)
    assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(t.reshape(5, 3)), _bits(t0))


def test_independent_outcomes_in_one_launch(sdf, world):
    """One problem takes the `success == False` branch (its cloud lies 10 m outside the volume: every point of every particle
    clamps to the same corner voxel, all energies are equal, none is better) between neighbours that converge as usual."""
    pre, tag = _pre(300), ("corner", np.float16)
    vols = [world["vols"][tag][k % 3] for k in range(3)]
    far = (world["probs"][3][0].cpu().numpy() * 0.01 + np.float32(10.0)).astype(np.float32)   # ~ (10, 10, 10) m, 1000 points
    Rf, tf = np.eye(3, dtype=np.float32), np.array([0.0, 0.0, 0.5], np.float32)
    R0, t0 = _stack(world, [0, 2])
    R0 = torch.stack([R0[0], _d(Rf), R0[1]])
    t0 = torch.stack([t0[0], _d(tf), t0[1]])
    clouds = [world["probs"][0][0], _d(far), world["probs"][2][0]]
    R, t = sdf.obj_optimize_batch(clouds, R0, t0, pre, [vols[0], vols[1], vols[2]], STRIDE, iterations=4)
    assert np.array_equal(_bits(R[1]), Rf.view(np.int32)) and np.array_equal(_bits(t[1].reshape(3)), tf.view(np.int32))
    Rs, ts = sdf.obj_optimize(_d(far), _d(Rf), _d(tf), pre, vols[1], STRIDE, iterations=4)
    assert np.array_equal(_bits(Rs.reshape(3, 3)), Rf.view(np.int32)) and np.array_equal(_bits(ts.reshape(3)), tf.view(np.int32))
    _check_equal_singles(sdf, world, R[[0, 2]], t[[0, 2]], [0, 2], [vols[0], vols[2]], pre, 4, tag)
    # a whole batch in which no particle differs from the current pose: every problem keeps its pose
    ks = list(range(5))
    R0, t0 = _stack(world, ks)
    R, t = sdf.obj_optimize_batch([world["probs"][k][0] for k in ks], R0, t0, torch.zeros((256, 6), device="cuda"),
                                  [world["vols"][tag][k % 3] for k in ks], STRIDE, iterations=3)
    assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(t.reshape(5, 3)), _bits(t0))


def test_order_independence(sdf, world):
    pre, tag = _pre(256), ("linear", np.float16)
    out = {}
    for ks in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1]):
        R0, t0 = _stack(world, ks)
        R, t = sdf.obj_optimize_batch([world["probs"][k][0] for k in ks], R0, t0, pre, [world["vols"][tag][k % 3] for k in ks],
                                      STRIDE, iterations=4)
        out[tuple(ks)] = {k: (_bits(R[j]), _bits(t[j])) for j, k in enumerate(ks)}
    a, b = out.values()
    for k in range(5):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), k


def test_reuse_of_work_and_cache(sdf, world):
    """The tickets are zero again after a call, so the same scratch serves the next one; with a cache dict the second call
    uploads nothing (same offsets tensor, same pointer table)."""
    pre, tag, ks = _pre(300), ("corner", np.float16), list(range(5))
    vols = [world["vols"][tag][k % 3] for k in ks]
    clouds = [world["probs"][k][0] for k in ks]
    R0, t0 = _stack(world, ks)
    need = 5 * ((16 + 300 + 15) // 16 * 16)
    work = torch.full((need + 7,), float("nan"), device="cuda")
    cache = {}
    first = sdf.obj_optimize_batch(clouds, R0, t0, pre, vols, STRIDE, iterations=4, work=work, cache=cache)
    held = {k: v[0] if isinstance(v, tuple) else v for k, v in cache.items()}
    assert len(held) == 2
    second = sdf.obj_optimize_batch(clouds, R0, t0, pre, vols, STRIDE, iterations=4, work=work, cache=cache)
    assert np.array_equal(_bits(first[0]), _bits(second[0])) and np.array_equal(_bits(first[1]), _bits(second[1]))
    assert len(cache) == 2 and all((v[0] if isinstance(v, tuple) else v) is held[k] for k, v in cache.items())
    assert torch.isnan(work[need:]).all()                                     # nothing is written past the s records
    _check_equal_singles(sdf, world, first[0], first[1], ks, vols, pre, 4, tag)
    # the packed form: one tensor and an offsets tensor on the device
    off = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int32, device="cuda")
    third = sdf.obj_optimize_batch(torch.cat(clouds), R0, t0, pre, vols, STRIDE, iterations=4, work=work, cloud_offsets=off)
    assert np.array_equal(_bits(first[0]), _bits(third[0])) and np.array_equal(_bits(first[1]), _bits(third[1]))


def test_poses_given_one_by_one_equal_the_stacked_form(sdf, world):
    """rotations / translations as two lists of S tensors (a tracker's per-sequence state) give the bits of the (S,3,3) / (S,3)
    form, as new tensors."""
    pre, tag, ks = _pre(300), ("corner", np.float16), list(range(5))
    vols = [world["vols"][tag][k % 3] for k in ks]
    clouds = [world["probs"][k][0] for k in ks]
    Rl = [world["probs"][k][1].reshape(1, 3, 3) for k in ks]
    tl = [world["probs"][k][2].reshape(1, 3, 1) for k in ks]
    R, t = sdf.obj_optimize_batch(clouds, Rl, tl, pre, vols, STRIDE, iterations=4)
    assert R.shape == (5, 3, 3) and t.shape == (5, 3, 1)
    _check_equal_singles(sdf, world, R, t, ks, vols, pre, 4, tag)
    assert all(torch.equal(Rl[k].reshape(3, 3), world["probs"][k][1]) for k in ks)     # the inputs are left alone
    with pytest.raises(ValueError):
        sdf.obj_optimize_batch(clouds, Rl, tl[:4], pre, vols, STRIDE, iterations=1)
    with pytest.raises(ValueError):
        sdf.obj_optimize_batch([], [], [], pre, [], STRIDE, iterations=1)


def test_capture_and_replay(sdf, world):
    pre, tag, ks = _pre(256), ("corner", np.float16), list(range(5))
    vols = [world["vols"][tag][k % 3] for k in ks]
    clouds = [world["probs"][k][0] for k in ks]
    R0, t0 = _stack(world, ks)
    work = torch.empty((5 * 272,), device="cuda")
    cache = {}
    eager = sdf.obj_optimize_batch(clouds, R0, t0, pre, vols, STRIDE, iterations=4, work=work, cache=cache)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (the offsets and the pointer table are in `cache`: the captured call uploads nothing)
        R, t = sdf.obj_optimize_batch(clouds, R0, t0, pre, vols, STRIDE, iterations=4, work=work, cache=cache)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(R), _bits(eager[0])) and np.array_equal(_bits(t), _bits(eager[1]))


def test_binding_errors(sdf, world):
    pre, ks = _pre(256), [0, 1, 2]
    lin16, lin32 = world["vols"][("linear", np.float16)], world["vols"][("linear", np.float32)]
    cor16 = world["vols"][("corner", np.float16)]
    clouds = [world["probs"][k][0] for k in ks]
    R0, t0 = _stack(world, ks)
    call = lambda **kw: sdf.obj_optimize_batch(kw.pop("clouds", clouds), kw.pop("R", R0), kw.pop("t", t0), kw.pop("pre", pre),
                                               kw.pop("vols", lin16), STRIDE, iterations=1, **kw)
    with pytest.raises(ValueError, match=r"volumes\[0\].*volumes\[2\].*differ"):       # mixed dtype
        call(vols=[lin16[0], lin16[1], lin32[2]])
    with pytest.raises(ValueError, match=r"volumes\[0\].*volumes\[1\].*differ"):       # mixed resolution
        call(vols=[lin16[0], _d(make_volume(21, 0.02, "box", np.float16)), lin16[2]])
    with pytest.raises(ValueError, match="differ"):                                    # mixed layout
        call(vols=[cor16[0], lin16[1], lin16[2]])
    with pytest.raises(ValueError, match="None"):                                      # a live problem without a volume
        call(vols=[lin16[0], None, lin16[2]])
    off = torch.tensor([0, 1, 256, 513], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="None"):                                      # packed clouds: no problem without one
        call(clouds=torch.cat(clouds), vols=[lin16[0], None, lin16[2]], cloud_offsets=off)
    with pytest.raises(RuntimeError, match="GPU"):                                     # no CPU path
        call(R=R0.cpu(), t=t0.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        call(vols=[lin16[0].cpu(), lin16[1], lin16[2]])
    with pytest.raises(ValueError, match=r"\(P,6\)"):
        call(pre=pre[:, :5])
    with pytest.raises(ValueError, match="work"):
        call(work=torch.empty((3 * 272 - 1,), device="cuda"))
    with pytest.raises(ValueError):
        call(clouds=clouds[:2])
    with pytest.raises(ValueError):
        call(vols=lin16[:2])
    with pytest.raises(ValueError):
        call(t=t0[:2])
