"""CPU: the argument validation of the batched hand-pose optimiser (include/pn2_ext.h: pn2x_hand_pose_opt_batch,
pn2x_hand_pose_problems_fill, pn2x_hand_pose_opt_batch_work_floats) -- bad sizes -1, NULL pointers -2, over a limit -3; no
iterations and a batch whose problems all sit out are no-ops -- before anything touches the device."""
import ctypes

from hotrack_amd.ext import _HandPoseProblem as Problem, _HandPoseSetup as Setup, _lib

vp = ctypes.c_void_p
EINVAL, ENULL, ERANGE = -1, -2, -3


def test_the_library_exports_the_batched_entry(hip_lib_path):
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("pn2x_hand_pose_opt_batch", "pn2x_hand_pose_problems_fill", "pn2x_hand_pose_opt_batch_work_floats"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(Problem) == 128


def test_work_floats():
    lib = _lib
    for p, s in ((1, 1), (5120, 1), (5120, 16), (260, 5), (0, 3), (3, 0), (8192, 65535)):
        assert lib.pn2x_hand_pose_opt_batch_work_floats(p, s) == s * lib.pn2x_hand_pose_opt_work_floats(p) == 4 * p * s, (p, s)
    assert lib.pn2x_hand_pose_opt_batch_work_floats(-1, 2) == EINVAL and lib.pn2x_hand_pose_opt_batch_work_floats(2, -1) == EINVAL


def test_hand_pose_opt_batch_argument_validation():
    lib = _lib
    one = vp(16)
    model = dict(parents=16, pose_block=16, skin_pack=16, skin_w=16, comps=16, pre=16)

    def call(p=256, v=70, j=21, k=2, f16=1, res=17, scale=0.01, s=3, active=3, problems=one, iterations=5, **ptr):
        setup = Setup(p=p, v=v, j=j, k=k, vol_f16=f16, res=res, theta_scale=30.0, voxel_scale=scale, w_sil=0.1, w_pen=1.0, w_vis=10.0,
                      w_invis=0.0, w_temporal=1.0, w_attr=0.05, **dict(model, **ptr))
        return lib.pn2x_hand_pose_opt_batch(setup, s, active, problems, iterations, 0.1, 0.9, None)

    # bad sizes: what pn2x_hand_pose_opt rejects, and s < 1, active outside [0, s]
    assert call(s=0) == EINVAL and call(s=-2) == EINVAL and call(active=-1) == EINVAL and call(active=4) == EINVAL
    assert call(p=0) == EINVAL and call(v=0) == EINVAL and call(j=0) == EINVAL and call(k=0) == EINVAL and call(iterations=-1) == EINVAL
    assert call(res=0) == EINVAL and call(res=16) == EINVAL and call(f16=2) == EINVAL and call(f16=-1) == EINVAL
    assert call(scale=0.0) == EINVAL and call(scale=-0.01) == EINVAL and call(scale=float("nan")) == EINVAL
    # over a limit
    assert call(s=65536, active=1) == ERANGE and call(iterations=4097) == ERANGE
    assert call(p=8193) == ERANGE and call(v=1025) == ERANGE and call(j=20) == ERANGE and call(k=5) == ERANGE and call(res=1025) == ERANGE
    # NULL: each shared pointer, and the table when there is work to do
    for name in model:
        assert call(**{name: None}) == ENULL, name
    assert call(problems=None) == ENULL
    # no iterations, or nobody active: OK, nothing launched, the table not needed
    assert call(iterations=0, problems=None) == 0 and call(iterations=0) == 0
    assert call(active=0) == 0 and call(active=0, problems=None, iterations=0) == 0
    assert call(s=65535, active=0) == 0
    assert call(iterations=0, s=0) == EINVAL and call(iterations=0, pre=None) == ENULL   # (a no-op does not excuse a bad argument)
    assert lib.pn2x_hand_pose_opt_batch(None, 3, 3, one, 5, 0.1, 0.9, None) == ENULL      # the setup record itself


def test_problems_fill_argument_validation():
    lib = _lib
    one = vp(16)

    def recs(n=3, **change):
        r = (Problem * n)()
        for q in range(n):
            for name, _ in Problem._fields_[:12]:
                setattr(r[q], name, 16)
            r[q].h, r[q].w, r[q].fx, r[q].fy, r[q].active = 12, 16, 600.0, 600.0, 1
        for name, value in change.items():
            setattr(r[n - 1], name, value)
        return r

    assert lib.pn2x_hand_pose_problems_fill(one, 0, recs(), None) == EINVAL
    assert lib.pn2x_hand_pose_problems_fill(one, 65536, recs(), None) == ERANGE
    assert lib.pn2x_hand_pose_problems_fill(None, 3, recs(), None) == ENULL
    assert lib.pn2x_hand_pose_problems_fill(one, 3, None, None) == ENULL
    assert lib.pn2x_hand_pose_problems_fill(one, 3, recs(h=0), None) == EINVAL
    assert lib.pn2x_hand_pose_problems_fill(one, 3, recs(w=-4), None) == EINVAL
    assert lib.pn2x_hand_pose_problems_fill(one, 3, recs(h=1 << 16, w=1 << 15), None) == ERANGE
    for name in ("state", "work", "rest_joints", "rest_verts", "pred_kp", "vis_mask", "obj_r", "obj_t", "vol", "mask"):
        assert lib.pn2x_hand_pose_problems_fill(one, 3, recs(**{name: None}), None) == ENULL, name
