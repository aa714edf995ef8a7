"""CPU: the argument validation of the mesh -> signed-distance entries (include/pn2_sdf.h: pn2s_mesh_sdf_points,
pn2s_mesh_sdf_volume, pn2s_mesh_sdf_work_floats) -- bad sizes -1, NULL pointers -2, over a limit -3, scratch too small -4, an
empty request is a no-op -- before anything touches the device."""
import ctypes

vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def _lib(path):
    lib = ctypes.CDLL(path)
    lib.pn2s_mesh_sdf_work_floats.argtypes = [ci]
    lib.pn2s_mesh_sdf_work_floats.restype = cl
    lib.pn2s_mesh_sdf_points.argtypes = [ci, vp, ci, vp, ci, vp, vp, vp, vp, cl, vp]
    lib.pn2s_mesh_sdf_points.restype = ci
    lib.pn2s_mesh_sdf_volume.argtypes = [ci, vp, ci, vp, ci, cf, cf, vp, ci, vp, cl, vp]
    lib.pn2s_mesh_sdf_volume.restype = ci
    return lib


def test_work_floats(hip_lib_path):
    lib = _lib(hip_lib_path)
    assert lib.pn2s_mesh_sdf_work_floats(-1) == -1
    assert lib.pn2s_mesh_sdf_work_floats(0) == 4                       # the header: the face-index flag, 16-byte alignment
    assert lib.pn2s_mesh_sdf_work_floats(12) == 4 + 20 * 12            # one 80-byte record per triangle
    assert lib.pn2s_mesh_sdf_work_floats(1 << 24) == 4 + 20 * (1 << 24)


def test_mesh_sdf_points_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    one = vp(16)
    big = 1 << 30

    def call(m=8, nv=8, nf=12, pts=one, verts=one, faces=one, out=one, wn=one, work=one, floats=big):
        return lib.pn2s_mesh_sdf_points(m, pts, nv, verts, nf, faces, out, wn, work, floats, None)

    assert call(m=-1) == -1 and call(nv=-1) == -1 and call(nf=-1) == -1            # negative sizes
    assert call(nv=0) == -1 and call(nf=0) == -1                                   # queries against an empty mesh
    assert call(m=0) == 0                                                          # no queries: a no-op ...
    assert call(m=0, pts=None, verts=None, faces=None, out=None, wn=None, work=None, floats=0) == 0   # ... that reads nothing
    for name in ("pts", "verts", "faces", "out", "work"):                          # each required pointer
        assert call(**{name: None}) == -2, name
    assert call(nv=(1 << 24) + 1) == -3 and call(nf=(1 << 24) + 1) == -3           # over the limits
    assert call(floats=4 + 20 * 12 - 1) == -4 and call(floats=0) == -4             # scratch too small
    assert call(work=vp(20)) == -1                                                 # scratch not 16-byte aligned


def test_mesh_sdf_volume_argument_validation(hip_lib_path):
    lib = _lib(hip_lib_path)
    one = vp(16)
    big = 1 << 30

    def call(nv=8, nf=12, res=25, stride=0.0167, clamp=0.1, verts=one, faces=one, out=one, f16=1, work=one, floats=big):
        return lib.pn2s_mesh_sdf_volume(nv, verts, nf, faces, res, stride, clamp, out, f16, work, floats, None)

    assert call(nv=-1) == -1 and call(nf=-1) == -1 and call(nv=0) == -1 and call(nf=0) == -1
    assert call(res=24) == -1 and call(res=200) == -1                              # even
    assert call(res=1) == -1 and call(res=0) == -1 and call(res=-3) == -1          # <= 1
    assert call(stride=0.0) == -1 and call(stride=-0.002) == -1 and call(stride=float("nan")) == -1
    assert call(clamp=0.0) == -1 and call(clamp=-0.1) == -1 and call(clamp=float("nan")) == -1
    for name in ("verts", "faces", "out", "work"):
        assert call(**{name: None}) == -2, name
        assert call(f16=0, **{name: None}) == -2, name
    assert call(res=1025) == -3 and call(nf=(1 << 24) + 1) == -3
    assert call(floats=4 + 20 * 12 - 1) == -4
