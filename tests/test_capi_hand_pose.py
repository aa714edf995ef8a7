"""CPU: argument validation of pn2x_hand_pose_energy / pn2x_hand_pose_opt and the pn2x_hand_pose_opt_supported query
(include/pn2_ext.h) -- everything is checked before any device work -- and of their Python bindings."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

ci, cl, vp = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
EINVAL, ENULL, ERANGE = -1, -2, -3
ONE = 16  # a fake, 16-byte aligned, non-null pointer
MANO_POINTERS = ("posedirs", "pose_mean", "kp_vertex")


def _records(ptr=ONE, mano=False, p=768, v=778, j=21, k=2, res=151, f16=1, scale=0.003, h=480, w=640, **change):
    """(setup, frame): the records of a valid call -- every required pointer `ptr`, with mano also the MANO part -- with `change`
    applied to whichever record has the field."""
    from hotrack_amd.ext import _HandPoseProblem, _HandPoseSetup
    setup = _HandPoseSetup(p=p, v=v, j=j, k=k, vol_f16=f16, res=res, theta_scale=30.0, voxel_scale=scale)
    for name, kind in _HandPoseSetup._fields_:
        if kind is vp and (mano or name not in MANO_POINTERS):
            setattr(setup, name, ptr)
    for name in _HandPoseSetup._WEIGHTS:
        setattr(setup, name, 1.0)
    frame = _HandPoseProblem(h=h, w=w, fx=1.0, fy=1.0, cx=1.0, cy=1.0)
    for name, kind in _HandPoseProblem._fields_:
        if kind is vp and name not in ("last_kp", "trace"):
            setattr(frame, name, ptr)
    for name, value in change.items():
        setattr(setup if hasattr(setup, name) else frame, name, value)
    return setup, frame


def _entries():
    from hotrack_amd.ext import _lib
    energy = lambda recs, offsets=None, energy=ONE: _lib.pn2x_hand_pose_energy(recs[0], recs[1], offsets, energy, None, None, None)
    opt = lambda recs, iterations=5, offsets=None: _lib.pn2x_hand_pose_opt(recs[0], recs[1], offsets, iterations, 0.1, 0.9, None)
    return _lib, energy, opt


def test_hand_pose_argument_validation_without_gpu(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    sup = lib.pn2x_hand_pose_opt_supported
    sup.argtypes = [ci] * 6
    assert sup(5120, 778, 21, 2, 10, 151) == 1 and sup(8192, 1024, 21, 4, 10, 201) == 1 and sup(1, 1, 21, 1, 10, 1) == 1
    assert sup(8193, 778, 21, 2, 10, 151) == 0 and sup(0, 778, 21, 2, 10, 151) == 0      # candidates
    assert sup(5120, 1025, 21, 2, 10, 151) == 0 and sup(5120, 0, 21, 2, 10, 151) == 0    # vertices
    assert sup(5120, 778, 20, 2, 10, 151) == 0 and sup(5120, 778, 22, 2, 10, 151) == 0   # the 21 keypoints
    assert sup(5120, 778, 21, 5, 10, 151) == 0 and sup(5120, 778, 21, 0, 10, 151) == 0   # weights per vertex
    assert sup(5120, 778, 21, 2, 12, 151) == 0                                           # pose components
    assert sup(5120, 778, 21, 2, 10, 150) == 0 and sup(5120, 778, 21, 2, 10, 1025) == 0  # volume
    wf = lib.pn2x_hand_pose_opt_work_floats
    wf.argtypes, wf.restype = [ci], cl
    assert wf(5120) == 4 * 5120 and wf(-1) == -1
    _, e, o = _entries()
    assert e(_records(p=0)) == EINVAL                 # p < 1
    assert e(_records(res=150)) == EINVAL             # even res
    assert e(_records(scale=0.0)) == EINVAL           # voxel_scale <= 0
    assert e(_records(f16=2)) == EINVAL
    assert e(_records(p=8193)) == ERANGE              # beyond the limits
    assert e(_records(j=20)) == ERANGE
    assert e(_records(k=5)) == ERANGE
    assert e(_records(ptr=None)) == ENULL             # NULL tables
    assert e(_records(state=None)) == ENULL           # NULL state
    assert o(_records(), iterations=-1) == EINVAL     # iterations < 0
    assert o(_records(), iterations=5000) == ERANGE
    assert o(_records(state=None, work=None), iterations=0) == 0   # no iterations: no-op
    assert o(_records(state=None)) == ENULL           # NULL state
    assert o(_records(ptr=None)) == ENULL
    assert o(_records(v=2000)) == ERANGE


def test_every_field_of_the_records_is_checked_once():
    """One violation per call, on both single-problem entries: each required pointer of either record, the frame's sizes, the
    record pointers themselves; what may be NULL is accepted up to the launch (no device here: a valid call is not made)."""
    from hotrack_amd.ext import _HandPoseProblem, _HandPoseSetup
    _, e, o = _entries()
    for call in (e, o):
        for name, kind in _HandPoseSetup._fields_:
            if kind is vp and name not in MANO_POINTERS:
                assert call(_records(**{name: None})) == ENULL, name
        for name, kind in _HandPoseProblem._fields_:
            if kind is vp and name not in ("last_kp", "trace"):
                assert call(_records(**{name: None})) == ENULL, name
        assert call(_records(h=0)) == EINVAL and call(_records(w=-4)) == EINVAL
        assert call(_records(h=1 << 16, w=1 << 15)) == ERANGE
        assert call((None, _records()[1])) == ENULL and call((_records()[0], None)) == ENULL
    assert e(_records(), energy=None) == ENULL
    # several at once: a bad value before a limit before a NULL pointer, and bad iterations before the frame's pointers
    assert e(_records(ptr=None, p=8193, res=150)) == EINVAL and e(_records(ptr=None, p=8193)) == ERANGE
    assert o(_records(ptr=None), iterations=-1) == EINVAL and o(_records(ptr=None), iterations=5000) == ERANGE
    assert o(_records(state=None, h=0)) == EINVAL
    # no iterations: the frame is not looked at and may be NULL; a bad setup is still refused
    assert o((_records()[0], None), iterations=0) == 0 and o(_records(h=0, mask=None), iterations=0) == 0
    assert o(_records(p=0), iterations=0) == EINVAL and o(_records(pre=None), iterations=0) == ENULL
    assert o((None, None), iterations=0) == ENULL
    # a record pointer no process can own (below 64 KiB) is refused, not read: a caller built against ABI version 3 passes p, v there
    from hotrack_amd.ext import _lib
    for fake in (1, 768, 8193, 65535):
        assert e((ctypes.cast(fake, ctypes.POINTER(_HandPoseSetup)), ctypes.cast(778, ctypes.POINTER(_HandPoseProblem)))) == EINVAL
        assert o((ctypes.cast(fake, ctypes.POINTER(_HandPoseSetup)), _records()[1])) == EINVAL
        assert o((_records()[0], ctypes.cast(fake, ctypes.POINTER(_HandPoseProblem)))) == EINVAL
        assert _lib.pn2x_hand_pose_opt_batch(ctypes.cast(fake, ctypes.POINTER(_HandPoseSetup)), 3, 3, ONE, 5, 0.1, 0.9, None) == EINVAL


def test_the_mano_half_is_validated_without_gpu():
    """A setup with posedirs set: its other MANO fields and `offsets` are required and checked; a plain setup reads none of them."""
    from hotrack_amd.ext import _lib
    _, e, o = _entries()
    for call in (e, o):
        for name in ("pose_mean", "kp_vertex"):
            assert call(_records(mano=True, **{name: None}), offsets=ONE) == ENULL, name
        assert call(_records(mano=True), offsets=None) == ENULL
        assert call(_records(mano=True, centre_root=2), offsets=ONE) == EINVAL
        assert call(_records(mano=True, centre_root=-1), offsets=ONE) == EINVAL
        assert call(_records(mano=True, posedirs=24), offsets=ONE) == EINVAL      # not 16-byte aligned
        assert call(_records(mano=True), offsets=24) == EINVAL
        assert call(_records(mano=True, centre_root=2, pose_mean=None), offsets=None) == EINVAL   # a bad value before a NULL pointer
        # a plain setup reads neither centre_root nor offsets: a value that a MANO setup answers with EINVAL leaves the call to
        # fail on its NULL state (a valid call cannot be made here: it would launch)
        assert call(_records(centre_root=7, state=None), offsets=24) == ENULL
        assert call(_records(centre_root=7, state=None), offsets=None) == ENULL
    assert o(_records(mano=True), iterations=0, offsets=None) == 0       # no iterations: offsets is not looked at
    assert o(_records(mano=True, centre_root=2), iterations=0, offsets=ONE) == EINVAL
    # a plain setup is accepted with its MANO fields and offsets NULL (accepted = the no-op's PN2_OK; the setup is checked first)
    assert o(_records(pose_mean=None, kp_vertex=None, centre_root=7), iterations=0, offsets=None) == 0
    setup = _records(mano=True)[0]
    assert _lib.pn2x_hand_pose_opt_batch(setup, 3, 3, ONE, 5, 0.1, 0.9, None) == EINVAL    # no batched MANO kernel
    assert _lib.pn2x_hand_pose_opt_batch(setup, 3, 3, ONE, 0, 0.1, 0.9, None) == EINVAL
    wf = _lib.pn2x_hand_pose_mano_work_floats
    assert wf(64, 778) == 64 * 2336 and wf(3, 5) == 3 * 16 and wf(-1, 5) == EINVAL and wf(5, -1) == EINVAL


def _cpu_call(P=64, res=151):
    from hotrack_amd import ext
    from models.hand_model import SyntheticLBSHand
    model = ext.hand_pose_model(SyntheticLBSHand().skinning_tables(), "cpu")
    z = torch.zeros
    return ext, dict(model=model, rest=ext.hand_pose_rest(model), theta_scale=30, pre=z(P, 16), state=z(ext.HAND_POSE_STATE_FLOATS),
                     pred_kp=z(21, 3), last_kp=None, vis_mask=z(21, dtype=torch.uint8), obj_r=torch.eye(3), obj_t=z(3),
                     volume=z(res, res, res, dtype=torch.float16), voxel_scale=0.003, mask=z(48, 64, dtype=torch.uint8),
                     proj={"fx": 60.0, "fy": 60.0, "cx": 32.0, "cy": 24.0},
                     weights={k: 1.0 for k in ext.HAND_POSE_WEIGHTS})


def test_bindings_refuse_cpu_tensors_and_unsupported_sizes():
    ext, kw = _cpu_call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.hand_pose_opt(iterations=5, scaling_coefficient2=0.1, beta=0.9, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.hand_pose_energy(**kw)
    ext, kw = _cpu_call(P=8200)
    with pytest.raises(ValueError, match="outside"):
        ext.hand_pose_opt(iterations=5, scaling_coefficient2=0.1, beta=0.9, **kw)
    ext, kw = _cpu_call(res=150)
    with pytest.raises(ValueError, match="outside"):
        ext.hand_pose_energy(**kw)
    assert ext.hand_pose_opt_supported(5120, 778, 21, 2) and not ext.hand_pose_opt_supported(5120, 778, 21, 2, 10, 150)


def test_bindings_refuse_a_vertex_that_serves_two_keypoints():
    """A model with MANO entries whose mano_ok is false is refused by the two entries before any device work (CPU tensors here)."""
    from models.hand_model import named_hand_model
    ext, kw = _cpu_call()
    tables = named_hand_model("synthetic_mano").skinning_tables()
    kpv = tables["kp_vertex"].clone()
    owned = [i for i, v in enumerate(kpv.tolist()) if v >= 0]
    kpv[owned[1]] = kpv[owned[0]]
    model = ext.hand_pose_model(dict(tables, kp_vertex=kpv), "cpu")
    assert model["mano"] and not model["mano_ok"]
    kw.update(model=model, rest=ext.hand_pose_rest(model))
    with pytest.raises(ValueError, match="one vertex serves two keypoints"):
        ext.hand_pose_energy(**kw)
    with pytest.raises(ValueError, match="one vertex serves two keypoints"):
        ext.hand_pose_opt(iterations=5, scaling_coefficient2=0.1, beta=0.9, **kw)
    good = ext.hand_pose_model(tables, "cpu")
    assert good["mano"] and good["mano_ok"]
    with pytest.raises(RuntimeError, match="no CPU path"):   # (the good model gets as far as the tensors)
        ext.hand_pose_energy(**dict(kw, model=good, rest=ext.hand_pose_rest(good)))
    with pytest.raises(ValueError, match="MANO entries"):
        ext.hand_pose_opt_batch(good, [None], torch.zeros(1, ext.HAND_POSE_STATE_FLOATS), 1, 0.1, 0.9)


def test_packed_skinning_table_round_trips():
    from hotrack_amd import ext
    from models.hand_model import SyntheticLBSHand
    t = SyntheticLBSHand().skinning_tables()
    m = ext.hand_pose_model(t, "cpu")
    pack = m["skin_pack"].long()
    assert torch.equal(pack & 31, t["skin_idx"][:, 0]) and torch.equal((pack >> 5) & 31, t["skin_idx"][:, 1])
    offs = t["finger_offsets"].tolist()
    for f in range(5):
        assert sorted(torch.nonzero((pack >> (20 + f)) & 1).flatten().tolist()) == sorted(set(t["tips"][offs[f]:offs[f + 1]].tolist()))
    assert m["fingers_ok"] and m["V"] == 778 and m["K"] == 2 and m["J"] == 21
