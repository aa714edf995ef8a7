"""CPU: the argument validation of the particle loop's two entries (include/pn2_sdf.h: pn2s_obj_opt, pn2s_obj_optimize,
pn2s_obj_optimize_batch, pn2s_obj_optimize_batch_work_floats) -- bad sizes -1, NULL record or pointers -2, over a limit -3, scratch too
small -4, an empty batch is a no-op -- before anything touches the device."""
import ctypes

vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


class ObjOpt(ctypes.Structure):
    _fields_ = ([(n, vp) for n in ("pcld", "cloud_off", "pre_sampled", "volume", "vols", "poses", "work")] + [("work_floats", cl)] +
                [(n, cf) for n in ("bbox_min", "stride", "clamp_lo", "clamp_hi", "c1", "c2", "beta")] +
                [(n, ci) for n in ("problems", "p", "n", "iterations", "res", "vol_fmt", "pad_")])


def _lib(path):
    lib = ctypes.CDLL(path)
    lib.pn2s_obj_optimize_batch_work_floats.argtypes = [ci, ci]
    lib.pn2s_obj_optimize_batch_work_floats.restype = cl
    for name in ("pn2s_obj_optimize", "pn2s_obj_optimize_batch"):
        getattr(lib, name).argtypes = [ctypes.POINTER(ObjOpt), vp]
        getattr(lib, name).restype = ci
    return lib


def _record(p):
    return (16 + p + 15) // 16 * 16   # the single entry's layout (16 header floats + p energies), padded to 16 floats


def test_record_size():
    assert ctypes.sizeof(ObjOpt) == 120   # as include/pn2_sdf.h documents and sdf.hip asserts


def test_work_floats(hip_lib_path):
    lib = _lib(hip_lib_path)
    for s, p in ((1, 1), (1, 256), (5, 300), (32, 2048), (3, 0), (4, 1 << 20)):
        assert lib.pn2s_obj_optimize_batch_work_floats(s, p) == s * _record(p), (s, p)
    assert _record(1) == 32 and _record(256) == 272 and _record(300) == 320 and _record(2048) == 2064
    assert lib.pn2s_obj_optimize_batch_work_floats(0, 2048) == 0
    assert lib.pn2s_obj_optimize_batch_work_floats(65535, 1 << 20) == 65535 * _record(1 << 20)   # no 32-bit overflow
    assert lib.pn2s_obj_optimize_batch_work_floats(-1, 8) == -1 and lib.pn2s_obj_optimize_batch_work_floats(2, -1) == -1


def test_obj_optimize_batch_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    one = 16
    big = 1 << 40

    def call(s=4, p=256, iterations=10, pcld=one, off=one, pre=one, vols=one, fmt=3, res=201, stride=0.002, poses=one, work=one,
             floats=big):
        r = ObjOpt(pcld=pcld, cloud_off=off, pre_sampled=pre, vols=vols, poses=poses, work=work, work_floats=floats, bbox_min=-0.2,
                   stride=stride, clamp_lo=-0.05, clamp_hi=0.05, c1=0.02, c2=2.0, beta=0.9, problems=s, p=p, iterations=iterations,
                   res=res, vol_fmt=fmt)
        return lib.pn2s_obj_optimize_batch(ctypes.byref(r), None)

    assert lib.pn2s_obj_optimize_batch(None, None) == -2                                              # a NULL record
    for count in (4, 65535, -1):                             # a count where the record is now (a positional caller): refused, not read
        assert lib.pn2s_obj_optimize_batch(ctypes.cast(vp(count), ctypes.POINTER(ObjOpt)), None) == -1
        assert lib.pn2s_obj_optimize(ctypes.cast(vp(count), ctypes.POINTER(ObjOpt)), None) == -1
    assert call(s=-1) == -1 and call(p=0) == -1 and call(p=-5) == -1 and call(iterations=-1) == -1    # bad sizes
    assert call(fmt=-1) == -1 and call(fmt=4) == -1                                                   # bad volume format
    assert call(res=1) == -1 and call(res=0) == -1 and call(res=-3) == -1 and call(res=1025) == -1    # as pn2s_obj_optimize
    assert call(stride=0.0) == -1 and call(stride=-0.002) == -1 and call(stride=float("nan")) == -1
    assert call(s=0) == 0                                                                             # no problems: a no-op ...
    assert call(s=0, pcld=None, off=None, pre=None, vols=None, poses=None, work=None, floats=0) == 0   # ... that reads nothing
    assert call(s=0, p=0) == -1 and call(s=0, fmt=7) == -1                     # (an empty batch does not excuse a bad argument)
    for name in ("pcld", "off", "pre", "vols", "poses", "work"):                                      # each required pointer
        assert call(**{name: None}) == -2, name
    assert call(s=65536, p=1) == -3                                            # s over PN2S_OPT_BATCH_MAX (the grid's y extent)
    assert call(s=1, p=(1 << 20) + 1) == -3                                    # p over 2^20
    assert call(s=2049, p=2048) == -3 and call(s=5, p=1 << 20) == -3           # s * p over 2^22 workgroups per launch
    assert call(s=2048, p=2048, floats=0) == -4                                # (exactly 2^22 is inside the limit)
    assert call(floats=4 * _record(256) - 1) == -4 and call(floats=0) == -4 and call(floats=-1) == -4  # scratch too small


def test_obj_optimize_argument_validation(hip_lib_path):
    """The single entry: the same checks through the same launch function, with problems == 1, n >= 1 and `volume`."""
    lib = _lib(hip_lib_path)
    one = 16

    def call(problems=1, p=256, n=1024, iterations=10, pcld=one, pre=one, volume=one, fmt=3, res=201, stride=0.002, poses=one, work=one,
             floats=16 + 256):
        r = ObjOpt(pcld=pcld, pre_sampled=pre, volume=volume, poses=poses, work=work, work_floats=floats, bbox_min=-0.2, stride=stride,
                   clamp_lo=-0.05, clamp_hi=0.05, c1=0.02, c2=2.0, beta=0.9, problems=problems, p=p, n=n, iterations=iterations, res=res,
                   vol_fmt=fmt)
        return lib.pn2s_obj_optimize(ctypes.byref(r), None)

    assert lib.pn2s_obj_optimize(None, None) == -2                                                    # a NULL record
    assert call(problems=0) == -1 and call(problems=2) == -1 and call(problems=-1) == -1              # one problem, no no-op
    assert call(n=0) == -1 and call(n=-7) == -1 and call(p=0) == -1 and call(p=-5) == -1 and call(iterations=-1) == -1
    assert call(fmt=-1) == -1 and call(fmt=4) == -1
    assert call(res=1) == -1 and call(res=0) == -1 and call(res=-3) == -1 and call(res=1025) == -1
    assert call(stride=0.0) == -1 and call(stride=-0.002) == -1 and call(stride=float("nan")) == -1 and call(stride=float("inf")) == -1
    for name in ("pcld", "pre", "volume", "poses", "work"):                                           # each required pointer
        assert call(**{name: None}) == -2, name
    assert call(p=(1 << 20) + 1, floats=1 << 40) == -3                                                # p over 2^20
    assert call(floats=16 + 256 - 1) == -4 and call(floats=0) == -4 and call(floats=-1) == -4         # pn2s_obj_optimize_work_floats(p)
    assert call(p=0, pcld=None) == -1 and call(p=(1 << 20) + 1, pcld=None) == -3                      # a value, then a limit, then NULL
