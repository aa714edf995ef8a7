"""Python binding of include/pn2_sdf.h -- the particle optimisers' SDF-volume lookups.  GPU tensors only.

Mirrors, function for function, the reference methods it replaces:
  distance          gf_optimize_obj.Distance                     network/models/optimization_obj.py:184-228
  particle_energy   gf_optimize_obj.evaluate                     :230-237
  obj_optimize      the particle loop of gf_optimize_obj.optimize :253-301
  query_sdf         gf_optimize_hand_pose.query_sdf              network/models/optimization_hand.py:252-262
  penetration_loss  ... .get_penetration_loss(query_sdf(hand))   :264-268 (fused with the lookup)
  mesh_signed_distance / mesh_sdf_volume   load_obj_oracle (mesh -> volume; kaolin there)   optimization_obj.py:163-182
  volume_mesh       gf_optimize_obj.sdf2mesh (volume -> mesh; marching cubes over the decoder there)   :399-405
  tsdf_integrate    no counterpart: depth frames fused into a volume, where update_shape refits a DeepSDF latent   :345-403
  tsdf_integrate_batch   the same for the volumes of S sequences tracked in lockstep, one launch
  volume_raycast    no counterpart: a volume rendered to depth and normal maps at tracked poses (the raycast), one launch
  raycast_compare   the rendered frames against the observed ones: overlap counts and depth residual sums, one launch
  obj_refine / obj_refine_batch   no counterpart: the tracked pose refined by damped Gauss-Newton on the volume, one launch
"""
from __future__ import annotations

import ctypes

import torch

from . import pointnet2_hip as _native

_lib = _native._lib
_vp, _ci, _cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_lib.pn2s_trilinear.argtypes = [_ci, _vp, _vp, _ci, _ci, _cf, _cf, _cf, _cf, _vp, _vp]
_lib.pn2s_particle_energy.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _cf, _cf, _cf, _cf, _vp, _vp]
_lib.pn2s_obj_optimize_work_floats.argtypes = [_ci]
_lib.pn2s_nearest.argtypes = [_ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _cf, _vp, _vp, _vp, _vp]
for _n in ("pn2s_trilinear", "pn2s_particle_energy", "pn2s_obj_optimize_work_floats", "pn2s_nearest"):
    getattr(_lib, _n).restype = _ci

_lib.pn2s_build_corner_volume.argtypes = [_vp, _ci, _ci, _vp, _vp]
_lib.pn2s_build_corner_volume.restype = _ci
_lib.pn2s_corner_volume_elems.argtypes = [_ci]
_lib.pn2s_corner_volume_elems.restype = ctypes.c_long
_lib.pn2s_obj_optimize_batch_work_floats.argtypes = [_ci, _ci]
_lib.pn2s_obj_optimize_batch_work_floats.restype = ctypes.c_long


class _ObjOpt(ctypes.Structure):
    """pn2s_obj_opt (120 bytes)."""
    _fields_ = ([(n, _vp) for n in ("pcld", "cloud_off", "pre_sampled", "volume", "vols", "poses", "work")] + [("work_floats", ctypes.c_long)] +
                [(n, _cf) for n in ("bbox_min", "stride", "clamp_lo", "clamp_hi", "c1", "c2", "beta")] +
                [(n, _ci) for n in ("problems", "p", "n", "iterations", "res", "vol_fmt", "pad_")])


assert ctypes.sizeof(_ObjOpt) == 120
for _n in ("pn2s_obj_optimize", "pn2s_obj_optimize_batch"):
    getattr(_lib, _n).argtypes = [ctypes.POINTER(_ObjOpt), _vp]
    getattr(_lib, _n).restype = _ci

BBOX_MIN = -0.2  # optimization_obj.py:186
CLAMP = (-0.05, 0.05)  # optimization_obj.py:227
_f32 = torch.float32


class CornerVolume:
    """Corner-layout copy of an SDF volume for the trilinear entries (include/pn2_sdf.h: pn2s_build_corner_volume):
    cell i holds the eight corner values Distance() fetches for base index i, so a lookup is one 16-byte load.
    Bit-identical results, ~3x faster lookups, 8x the memory; build once per object and pass it wherever a
    `sdf_volume` is accepted by distance / particle_energy / obj_optimize."""

    def __init__(self, sdf_volume: torch.Tensor):
        pv, f16, res = _linear_volume(sdf_volume)
        self.res, self.f16, self.source = res, f16, sdf_volume
        self.data = torch.empty((res ** 3, 8), dtype=sdf_volume.dtype, device=sdf_volume.device)
        assert _lib.pn2s_corner_volume_elems(res) == self.data.numel()
        with torch.cuda.device(sdf_volume.device):
            rc = _lib.pn2s_build_corner_volume(pv, f16, res, self.data.data_ptr(), _native._stream(sdf_volume))
        _native._check(rc, "sdf.CornerVolume")


def _volume(vol):
    """-> (device pointer, vol_fmt, res) for a linear volume tensor or a CornerVolume."""
    if isinstance(vol, CornerVolume):
        return vol.data.data_ptr(), 2 + vol.f16, vol.res
    return _linear_volume(vol)


def _linear_volume(vol: torch.Tensor):
    """Validate an SDF volume: (res,res,res) or flat res^3, fp16 or fp32, contiguous, on the GPU."""
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise RuntimeError("sdf volume must be a GPU (HIP) tensor -- hotrack_amd has no CPU path")
    if vol.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"sdf volume must be float16 or float32, got {vol.dtype}")
    if not vol.is_contiguous():
        raise ValueError("sdf volume must be contiguous")
    res = vol.shape[0] if vol.dim() == 3 else round(vol.numel() ** (1.0 / 3.0))
    if res ** 3 != vol.numel() or (vol.dim() == 3 and tuple(vol.shape) != (res, res, res)):
        raise ValueError(f"sdf volume must hold res^3 elements, got shape {tuple(vol.shape)}")
    return vol.data_ptr(), int(vol.dtype == torch.float16), res


def distance(V: torch.Tensor, sdf_volume: torch.Tensor, voxel_scale: float, bbox_min: float = BBOX_MIN, clamp=CLAMP) -> torch.Tensor:
    """Trilinear SDF at V (M,3) object-frame points -> (M,) fp32, clamped (== gf_optimize_obj.Distance)."""
    pv, f16, res = _volume(sdf_volume)
    if V.dim() != 2 or V.shape[1] != 3:
        raise ValueError(f"V must be (M,3), got {tuple(V.shape)}")
    V = V.contiguous()
    m = V.shape[0]
    pV = _native._ptr(V, "V", _f32, m * 3)
    out = torch.empty((m,), dtype=_f32, device=V.device)
    with torch.cuda.device(V.device):
        rc = _lib.pn2s_trilinear(m, pV, pv, f16, res, bbox_min, voxel_scale, clamp[0], clamp[1],
                                 out.data_ptr(), _native._stream(V))
    _native._check(rc, "sdf.distance")
    return out


def particle_energy(pcld: torch.Tensor, r: torch.Tensor, t: torch.Tensor, sdf_volume: torch.Tensor, voxel_scale: float,
                    bbox_min: float = BBOX_MIN, clamp=CLAMP) -> torch.Tensor:
    """sdf_energy (P,) = mean_n |Distance((pcld - t_p) @ r_p)|  (== the second output of gf_optimize_obj.evaluate;
    the first is 500x this).  pcld (N,3) or (1,N,3); r (P,3,3); t (P,3) or (P,3,1)."""
    pv, f16, res = _volume(sdf_volume)
    pcld = pcld.reshape(-1, 3).contiguous()
    P = r.shape[0]
    r = r.contiguous()
    t = t.reshape(P, 3).contiguous()
    n = pcld.shape[0]
    ptrs = (_native._ptr(pcld, "pcld", _f32, n * 3), _native._ptr(r, "r", _f32, P * 9), _native._ptr(t, "t", _f32, P * 3))
    out = torch.empty((P,), dtype=_f32, device=pcld.device)
    with torch.cuda.device(pcld.device):
        rc = _lib.pn2s_particle_energy(P, n, *ptrs, pv, f16, res, bbox_min, voxel_scale, clamp[0], clamp[1],
                                       out.data_ptr(), _native._stream(pcld))
    _native._check(rc, "sdf.particle_energy")
    return out


def _pose12(rotation, translation):
    """One pose as the kernels take it: 12 floats, the rotation (3,3) row-major, then the translation (3); a new tensor."""
    return torch.cat([rotation.reshape(9).to(_f32), translation.reshape(3).to(_f32)]).contiguous()


def _pose_rows(who, rotations, translations):
    """S poses -> (S, (S,12) tensor as _pose12's rows), from two lists of S tensors (3,3)|(1,3,3) and (3,)|(1,3,1) -- a tracker's
    state, held one by one and assembled by ONE concatenation -- or from (S,3,3) and (S,3)|(S,3,1)."""
    if isinstance(rotations, (list, tuple)):
        S = len(rotations)
        if S == 0 or len(translations) != S:
            raise ValueError(f"{who}: rotations and translations must be two lists of S >= 1 tensors, got {S} and {len(translations)}")
        pose = torch.cat([x.reshape(1, n).to(_f32) for R, t in zip(rotations, translations) for x, n in ((R, 9), (t, 3))], dim=1).view(S, 12)
    else:
        S = rotations.shape[0]
        if rotations.numel() != 9 * S or translations.numel() != 3 * S:
            raise ValueError(f"{who}: rotations (S,3,3) and translations (S,3)|(S,3,1), got {tuple(rotations.shape)} and {tuple(translations.shape)}")
        pose = torch.cat([rotations.reshape(S, 9).to(_f32), translations.reshape(S, 3).to(_f32)], dim=1).contiguous()
    _native._ptr(pose, "rotations/translations", _f32, 12 * S)
    return S, pose


def _pack_clouds(who, pclds, S, device, cache):
    """A list of S clouds (n_k,3)|(1,n_k,3), an empty one or None marking an inactive problem -> (packed (sum n_k,3), sizes, active:
    the problems with points, the int32 device tensor of the S + 1 offsets).  With a `cache` dict the offsets of a repeated list
    of sizes are uploaded once.  Nothing active: (None, sizes, [], None)."""
    if len(pclds) != S:
        raise ValueError(f"{who}: pclds must hold S = {S} clouds, got {len(pclds)}")
    clouds = [None if c is None or c.numel() == 0 else c.reshape(-1, 3) for c in pclds]
    sizes = tuple(0 if c is None else c.shape[0] for c in clouds)
    active = [k for k, n in enumerate(sizes) if n]
    if not active:
        return None, sizes, active, None
    packed = (clouds[active[0]] if len(active) == 1 else torch.cat([clouds[k] for k in active])).contiguous()
    key = ("off", str(device), sizes)
    off = None if cache is None else cache.get(key)
    if off is None:
        acc = [0]
        for n in sizes:
            acc.append(acc[-1] + n)
        off = torch.tensor(acc, dtype=torch.int32, device=device)
        if cache is not None:
            cache[key] = off
    return packed, sizes, active, off


def _obj_opt(entry, who, pose, pre_sampled_particle, work, need_floats, fmt, res, voxel_scale, iterations, c1, c2, beta, bbox_min, clamp, **own):
    """What obj_optimize and obj_optimize_batch share: the particles and the work buffer checked, pn2s_obj_opt filled (`own`: the
    fields that are one entry's own) and `entry` called on the poses' device and stream."""
    pre = pre_sampled_particle.contiguous()
    if pre.dim() != 2 or pre.shape[1] != 6:
        raise ValueError("pre_sampled_particle must be (P,6)")
    P = pre.shape[0]
    need = need_floats(P)
    if work is None:
        work = torch.empty((need,), dtype=_f32, device=pose.device)
    elif work.numel() < need or work.dtype != _f32 or not work.is_cuda or not work.is_contiguous():
        raise ValueError(f"work must be a contiguous float32 GPU tensor of >= {need} elements")
    r = _ObjOpt(p=P, iterations=iterations, res=res, vol_fmt=fmt, bbox_min=bbox_min, stride=voxel_scale, clamp_lo=clamp[0],
                clamp_hi=clamp[1], c1=c1, c2=c2, beta=beta, work_floats=work.numel(), **own)
    r.pre_sampled, r.poses, r.work = _native._ptr(pre, "pre_sampled_particle", _f32, P * 6), pose.data_ptr(), work.data_ptr()
    with torch.cuda.device(pose.device):
        rc = entry(ctypes.byref(r), _native._stream(pose))
    _native._check(rc, who)


def obj_optimize(pcld: torch.Tensor, rotation: torch.Tensor, translation: torch.Tensor, pre_sampled_particle: torch.Tensor,
                 sdf_volume: torch.Tensor, voxel_scale: float, iterations: int = 10, scaling_coefficient1: float = 0.02,
                 scaling_coefficient2: float = 2.0, beta: float = 0.9, bbox_min: float = BBOX_MIN, clamp=CLAMP, work=None):
    """The particle loop of gf_optimize_obj.optimize on the device, no host synchronisation.
    pcld (N,3)|(1,N,3); rotation (3,3)|(1,3,3); translation (3,)|(1,3,1); pre_sampled_particle (P,6), row 0 == 0.
    Returns (rotation (1,3,3), translation (1,3,1)) as new tensors."""
    pv, fmt, res = _volume(sdf_volume)
    pcld = pcld.reshape(-1, 3).contiguous()
    n = pcld.shape[0]
    p_pcld = _native._ptr(pcld, "pcld", _f32, n * 3)
    pose = _pose12(rotation, translation)
    _native._ptr(pose, "rotation/translation", _f32, 12)
    _obj_opt(_lib.pn2s_obj_optimize, "sdf.obj_optimize", pose, pre_sampled_particle, work, _lib.pn2s_obj_optimize_work_floats, fmt, res,
             voxel_scale, iterations, scaling_coefficient1, scaling_coefficient2, beta, bbox_min, clamp, problems=1, n=n, pcld=p_pcld, volume=pv)
    return pose[:9].view(1, 3, 3), pose[9:].view(1, 3, 1)


def _volume_table(volumes, active, device, cache):
    """-> (device int64 tensor of the S volume pointers, vol_fmt, res).  Every volume given must share one layout, dtype and
    resolution; None (a NULL entry) is allowed where the problem is inactive.  With a `cache` dict the table of a list of
    the same volume objects is uploaded once."""
    key = ("vols", str(device), tuple(map(id, volumes)))
    hit = None if cache is None else cache.get(key)
    if hit is None:
        ptrs, first = [], None
        for k, v in enumerate(volumes):
            if v is None:
                ptrs.append(0)
                continue
            pv, fmt, res = _volume(v)
            if first is None:
                first = (k, fmt, res)
            elif (fmt, res) != first[1:]:
                what = lambda f, r: "%s %s res %d" % ("corner" if f >= 2 else "linear", "float16" if f & 1 else "float32", r)
                raise ValueError(f"volumes[{first[0]}] ({what(*first[1:])}) and volumes[{k}] ({what(fmt, res)}) differ: "
                                 "a batch shares one layout, dtype and resolution")
            ptrs.append(pv)
        if first is None:
            raise ValueError("volumes holds no volume")
        # (the volumes are kept with the table: the key's ids stay theirs)
        hit = (torch.tensor(ptrs, dtype=torch.int64, device=device), first[1], first[2], list(volumes))
        if cache is not None:
            cache[key] = hit
    for k in active:
        if volumes[k] is None:
            raise ValueError(f"volumes[{k}] is None but problem {k} has a cloud (or the clouds are packed: every problem needs one)")
    return hit[:3]


def obj_optimize_batch_work_floats(S: int, P: int) -> int:
    """Floats of scratch obj_optimize_batch needs for S problems of P particles (pn2s_obj_optimize_batch_work_floats)."""
    need = _lib.pn2s_obj_optimize_batch_work_floats(S, P)
    if need < 0:
        raise ValueError(f"S and P must not be negative, got {S} and {P}")
    return need


def obj_optimize_batch(pclds, rotations, translations, pre_sampled_particle: torch.Tensor, volumes,
                       voxel_scale: float, iterations: int = 10, scaling_coefficient1: float = 0.02,
                       scaling_coefficient2: float = 2.0, beta: float = 0.9, bbox_min: float = BBOX_MIN, clamp=CLAMP, work=None,
                       cloud_offsets=None, cache=None):
    """obj_optimize for S independent problems with ONE set of launches (include/pn2_sdf.h: pn2s_obj_optimize_batch); every
    problem's result is bit-for-bit what obj_optimize returns for it alone.
    pclds: a list of S clouds (n_k,3)|(1,n_k,3) -- an empty one, or None, marks an INACTIVE problem, whose pose comes back
      unchanged -- or one packed (sum n_k,3) tensor with `cloud_offsets`, an int32 GPU tensor of S+1 offsets in points that
      lie inside it (cloud_offsets[k+1] <= cloud_offsets[k]: inactive).  The offsets stay on the device, so on this route the
      caller answers for them and EVERY problem needs a volume (None is refused: which slices are empty is not known here);
    rotations (S,3,3) and translations (S,3)|(S,3,1), or two lists of S tensors (3,3)|(1,3,3) and (3,)|(1,3,1);
    pre_sampled_particle (P,6), row 0 == 0, shared;
    volumes: S CornerVolumes or S linear volume tensors of one layout, dtype and resolution (all read with `voxel_scale`);
      None is allowed for an inactive problem of the list form;
    work: >= pn2s_obj_optimize_batch_work_floats(S,P) floats, or None;
    cache: a dict the caller keeps between calls: the offsets of a repeated list of cloud sizes and the pointer table of a
      repeated list of volumes are then uploaded once (a steady-state call uploads nothing; required for graph capture).
    Returns (rotations (S,3,3), translations (S,3,1)) as new tensors."""
    S, pose = _pose_rows("obj_optimize_batch", rotations, translations)
    device = pose.device
    out = pose[:, :9].view(S, 3, 3), pose[:, 9:].reshape(S, 3, 1)
    if len(volumes) != S:
        raise ValueError(f"volumes must hold S = {S} entries, got {len(volumes)}")
    if cloud_offsets is None:
        packed, sizes, active, off = _pack_clouds("obj_optimize_batch", pclds, S, device, cache)
        total = sum(sizes)
    else:
        if not isinstance(pclds, torch.Tensor) or pclds.dim() != 2 or pclds.shape[1] != 3:
            raise ValueError("with cloud_offsets, pclds must be one packed (N,3) tensor")
        packed, off, total = pclds.contiguous(), cloud_offsets, pclds.shape[0]
        active = range(S)  # (which slices are empty is known on the device only: no problem may go without a volume)
    if total == 0:
        return out
    table, fmt, res = _volume_table(volumes, active, device, cache)
    if packed.device != device or pre_sampled_particle.device != device:
        raise RuntimeError(f"the clouds, poses and particles are on different devices ({packed.device}, {device}, {pre_sampled_particle.device})")
    _obj_opt(_lib.pn2s_obj_optimize_batch, "sdf.obj_optimize_batch", pose, pre_sampled_particle, work, lambda P: obj_optimize_batch_work_floats(S, P),
             fmt, res, voxel_scale, iterations, scaling_coefficient1, scaling_coefficient2, beta, bbox_min, clamp, problems=S, vols=table.data_ptr(),
             pcld=_native._ptr(packed, "pclds", _f32, total * 3), cloud_off=_native._ptr(off, "cloud_offsets", torch.int32, S + 1))
    return out


def query_sdf(hand: torch.Tensor, obj_r: torch.Tensor, obj_t: torch.Tensor, sdf_volume: torch.Tensor, voxel_scale: float,
              with_penetration: bool = False, with_index: bool = False):
    """Nearest-voxel SDF of hand (B,N,3) in the object frame (== gf_optimize_hand_pose.query_sdf), dtype of the
    volume.  with_penetration: also the fused get_penetration_loss (B,).  with_index: also the flat voxel index."""
    pv, f16, res = _linear_volume(sdf_volume)
    if hand.dim() != 3 or hand.shape[2] != 3:
        raise ValueError(f"hand must be (B,N,3), got {tuple(hand.shape)}")
    hand = hand.contiguous()
    B, N, _ = hand.shape
    obj_r = obj_r.reshape(3, 3).to(_f32).contiguous()
    obj_t = obj_t.reshape(3).to(_f32).contiguous()
    ptrs = (_native._ptr(hand, "hand", _f32, B * N * 3), _native._ptr(obj_r, "obj_r", _f32, 9), _native._ptr(obj_t, "obj_t", _f32, 3))
    sdf = torch.empty((B, N), dtype=sdf_volume.dtype, device=hand.device)
    pen = torch.empty((B,), dtype=sdf_volume.dtype, device=hand.device) if with_penetration else None
    idx = torch.empty((B, N), dtype=torch.int32, device=hand.device) if with_index else None
    with torch.cuda.device(hand.device):
        rc = _lib.pn2s_nearest(B, N, *ptrs, pv, f16, res, voxel_scale,
                               None if idx is None else idx.data_ptr(), sdf.data_ptr(), None if pen is None else pen.data_ptr(),
                               _native._stream(hand))
    _native._check(rc, "sdf.query_sdf")
    ret = (sdf,)
    if with_penetration:
        ret += (pen,)
    if with_index:
        ret += (idx,)
    return ret[0] if len(ret) == 1 else ret


# ---- mesh -> signed distance (hotrack_amd/csrc/mesh_sdf.hip) ------------------------------------------------------------------
_cl = ctypes.c_long
_lib.pn2s_mesh_sdf_work_floats.argtypes = [_ci]
_lib.pn2s_mesh_sdf_work_floats.restype = _cl
_lib.pn2s_mesh_sdf_points.argtypes = [_ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _cl, _vp]
_lib.pn2s_mesh_sdf_points.restype = _ci
_lib.pn2s_mesh_sdf_volume.argtypes = [_ci, _vp, _ci, _vp, _ci, _cf, _cf, _vp, _ci, _vp, _cl, _vp]
_lib.pn2s_mesh_sdf_volume.restype = _ci


def _mesh(verts: torch.Tensor, faces: torch.Tensor):
    """Validate a mesh: verts (nv,3) float32, faces (nf,3) int32, contiguous, on one GPU -> (nv, verts pointer, nf, faces pointer)."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"verts must be (nv,3) and faces (nf,3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError("the mesh is empty")
    nv, nf = verts.shape[0], faces.shape[0]
    pv, pf = _native._ptr(verts, "verts", _f32, nv * 3), _native._ptr(faces, "faces", torch.int32, nf * 3)
    if faces.device != verts.device:
        raise RuntimeError(f"verts and faces are on different devices ({verts.device}, {faces.device})")
    return nv, pv, nf, pf


def _mesh_work(nf: int, device) -> torch.Tensor:
    return torch.empty((_lib.pn2s_mesh_sdf_work_floats(nf),), dtype=_f32, device=device)


def _mesh_faces_ok(work: torch.Tensor, what: str) -> None:
    """The one read-back per call: the kernel's face-index check (include/pn2_sdf.h).  Raises before the caller sees the output."""
    if int(work[:1].view(torch.int32).item()) != 0:
        raise ValueError(f"{what}: a face index lies outside [0, number of vertices)")


def mesh_signed_distance(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, return_winding: bool = False):
    """Signed distance (M,) fp32 of points (M,3) to the triangle mesh (verts (nv,3) fp32, faces (nf,3) int32): exact
    point-triangle minimum over all faces, negative where the generalised winding number exceeds 0.5; unclamped.
    return_winding: also the winding numbers (M,).  Synchronises once (the face-index check)."""
    nv, pv, nf, pf = _mesh(verts, faces)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (M,3), got {tuple(points.shape)}")
    m = points.shape[0]
    pp = _native._ptr(points, "points", _f32, m * 3)
    if points.device != verts.device:
        raise RuntimeError(f"points and the mesh are on different devices ({points.device}, {verts.device})")
    out = torch.empty((m,), dtype=_f32, device=verts.device)
    wn = torch.empty((m,), dtype=_f32, device=verts.device) if return_winding else None
    if m:
        work = _mesh_work(nf, verts.device)
        with torch.cuda.device(verts.device):
            rc = _lib.pn2s_mesh_sdf_points(m, pp, nv, pv, nf, pf, out.data_ptr(), None if wn is None else wn.data_ptr(),
                                           work.data_ptr(), work.numel(), _native._stream(verts))
        _native._check(rc, "sdf.mesh_signed_distance")
        _mesh_faces_ok(work, "sdf.mesh_signed_distance")
    return (out, wn) if return_winding else out


def mesh_sdf_volume(verts: torch.Tensor, faces: torch.Tensor, res: int = 201, voxel_scale: float = 0.002, clamp: float = 0.1,
                    dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """(res,res,res) SDF volume of the mesh, indexed [ix,iy,iz] with voxel centre ((ix,iy,iz) - res//2) * voxel_scale (the grid
    of the reference's volume_ind, optimization_obj.py:133-143), clamped to +-clamp and rounded once to `dtype` (float16, the
    reference's storage type, or float32).  One build per object: synchronises once (the face-index check)."""
    nv, pv, nf, pf = _mesh(verts, faces)
    if dtype not in (torch.float16, torch.float32):
        raise TypeError(f"dtype must be float16 or float32, got {dtype}")
    res = int(res)
    out = torch.empty((res, res, res) if res > 0 else (0,), dtype=dtype, device=verts.device)
    work = _mesh_work(nf, verts.device)
    with torch.cuda.device(verts.device):
        rc = _lib.pn2s_mesh_sdf_volume(nv, pv, nf, pf, res, float(voxel_scale), float(clamp), out.data_ptr(), int(dtype == torch.float16),
                                       work.data_ptr(), work.numel(), _native._stream(verts))
    _native._check(rc, "sdf.mesh_sdf_volume")
    _mesh_faces_ok(work, "sdf.mesh_sdf_volume")
    return out


# ---- signed distance volume -> mesh (hotrack_amd/csrc/sdf_mesh.hip) -------------------------------------------------------------
_lib.pn2s_volume_mesh_work_bytes.argtypes = [_ci]
_lib.pn2s_volume_mesh_work_bytes.restype = _cl
_lib.pn2s_volume_mesh_count.argtypes = [_vp, _ci, _ci, _cf, _cf, _vp, _cl, _vp]
_lib.pn2s_volume_mesh_count.restype = _ci
_lib.pn2s_volume_mesh_emit.argtypes = [_vp, _ci, _ci, _cf, _cf, _vp, _cl, _ci, _ci, _vp, _vp, _vp]
_lib.pn2s_volume_mesh_emit.restype = _ci
VOLUME_MESH_MAX_RES = 512


def volume_mesh_work_bytes(res: int) -> int:
    """Bytes of scratch volume_mesh needs at resolution res (pn2s_volume_mesh_work_bytes): an int32 and a byte per voxel."""
    need = _lib.pn2s_volume_mesh_work_bytes(int(res))
    if need < 0:
        raise ValueError(f"res must lie in [2, {VOLUME_MESH_MAX_RES}], got {res}")
    return need


def volume_mesh(sdf_volume: torch.Tensor, voxel_scale: float, level: float = 0.0):
    """The level set of a (res,res,res) fp16 / fp32 SDF volume as a welded, outward-oriented triangle mesh (marching tetrahedra;
    include/pn2_sdf.h: pn2s_volume_mesh_count / pn2s_volume_mesh_emit) -> (verts float32 (nv,3), faces int32 (nf,3)) on the
    volume's device, in the grid of mesh_sdf_volume (voxel centre ((ix,iy,iz) - res//2) * voxel_scale).  The order of vertices
    and triangles is fixed by the algorithm; a volume with no crossing returns (0,3) / (0,3).  Synchronises once (the two counts)."""
    if isinstance(sdf_volume, torch.Tensor) and sdf_volume.dim() != 3:
        raise ValueError(f"sdf volume must be (res,res,res), got shape {tuple(sdf_volume.shape)}")
    pv, f16, res = _linear_volume(sdf_volume)
    voxel_scale, level = float(voxel_scale), float(level)
    if not (voxel_scale > 0 and voxel_scale != float("inf")) or level != level or abs(level) == float("inf"):
        raise ValueError(f"voxel_scale must be finite and > 0 and level finite, got {voxel_scale} and {level}")
    need = volume_mesh_work_bytes(res)
    device = sdf_volume.device
    work = torch.empty((need // 4 + 1,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        st = _native._stream(sdf_volume)
        rc = _lib.pn2s_volume_mesh_count(pv, f16, res, voxel_scale, level, work.data_ptr(), work.numel() * 4, st)
        _native._check(rc, "sdf.volume_mesh")
        nv, nf = work[:2].tolist()  # the one read-back
        verts = torch.empty((nv, 3), dtype=_f32, device=device)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=device)
        rc = _lib.pn2s_volume_mesh_emit(pv, f16, res, voxel_scale, level, work.data_ptr(), work.numel() * 4, nv, nf,
                                        verts.data_ptr() if nv else None, faces.data_ptr() if nf else None, st)
        _native._check(rc, "sdf.volume_mesh")
    return verts, faces


# ---- the argument checks the frame entries share; `who` is the caller's name, the prefix of every message -----------------------
_FRAMES = ("depth", "seg", "intrinsics", "rotation", "translation")   # the per-frame arrays, as the records and the messages name them
_TSDF_TENSORS, _RAYCAST_TENSORS = ("volume", "weight") + _FRAMES, ("volume",) + _FRAMES[2:]
_VOLUME_DTYPES, _RAW_DTYPES, _INF = (torch.float16, torch.float32), (torch.uint16, torch.int16), float("inf")


def _contiguous_tensors(who, names, tensors):
    for name, t in zip(names, tensors):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")


def _on_one_gpu(who, module, device, names, tensors):
    for i, t in enumerate(tensors):
        if not t.is_cuda or t.device != device:   # (names may be a function: a long list is then named only to say which one)
            name = (names() if callable(names) else names)[i]
            if not t.is_cuda:
                raise RuntimeError(f"{who}: {name} must be a GPU (HIP) tensor -- hotrack_amd has no CPU path (got device {t.device}); "
                                   f"network/models/{module}.{who}_torch runs anywhere")
            raise ValueError(f"{who}: tensors on {device} and {t.device}")


def _cubic_volume(who, volume, max_res, layout=""):
    """A (res,res,res) fp16 / fp32 volume in the linear layout with 2 <= res <= max_res -> res."""
    if volume.dtype not in _VOLUME_DTYPES:
        raise TypeError(f"{who}: the volume must be float16 or float32, got {volume.dtype}")
    shape = volume.shape
    if len(shape) != 3 or not shape[0] == shape[1] == shape[2]:
        raise ValueError(f"{who}: the volume must be (res,res,res){layout}, got {tuple(shape)}")
    res = shape[0]
    if not 2 <= res <= max_res:
        raise ValueError(f"{who}: res must lie in [2, {max_res}], got {res}")
    return res


def _observed_frames(who, depth, seg, obj_class, depth_scale, rendered=None):
    """The observed frames as hotrack_amd/csrc/frame_device.h defines them (the depth encoding, the depth / segment image pair, the
    class), and a rendered image of their size if one is given -> (F, H, W, Hs, Ws, C, f, depth is raw counts)."""
    if depth.dim() != 3 or depth.shape[0] < 1:
        raise ValueError(f"{who}: depth must be (F,H,W) with F >= 1, got {tuple(depth.shape)}")
    F, H, W = depth.shape
    if rendered is not None and (rendered.dtype != _f32 or rendered.shape != depth.shape):
        raise ValueError(f"{who}: rendered must be float32 {tuple(depth.shape)}, got {rendered.dtype} {tuple(rendered.shape)}")
    raw = depth.dtype in _RAW_DTYPES   # (int16: the same 16 bits, for a torch without uint16 arithmetic)
    if raw == (depth_scale is None) or (not raw and depth.dtype != _f32):
        raise TypeError(f"{who}: depth is fp32 metres, or uint16 counts with a depth_scale (got {depth.dtype}, "
                        f"depth_scale = {depth_scale})")
    if raw and not 0 < float(depth_scale) < _INF:
        raise ValueError(f"{who}: depth_scale must be finite and > 0, got {depth_scale}")
    if seg.dtype != torch.uint8 or seg.dim() != 4 or seg.shape[0] != F:
        raise ValueError(f"{who}: seg must be uint8 (F,Hs,Ws,C) with F = {F}, got {seg.dtype} {tuple(seg.shape)}")
    _, Hs, Ws, C = seg.shape
    if min(H, W, Hs, Ws) < 1 or H % Hs or W % Ws or H // Hs != W // Ws or C not in (1, 3) or H * W >= 1 << 29 or F > 65535:
        raise ValueError(f"{who}: depth {H} x {W}, seg {Hs} x {Ws} x {C}: one integer factor between the two images, "
                         "C 1 or 3, H W < 2^29, at most 65535 frames")
    channel, value = int(obj_class[0]), int(obj_class[1])
    if not (0 <= channel < C and 0 <= value <= 255):
        raise ValueError(f"{who}: obj_class = (channel, value) with channel in [0, {C}) and value in [0, 255], got {tuple(obj_class)}")
    return F, H, W, Hs, Ws, C, H // Hs, raw


def _pose_frames(who, F, intrinsics, rotation, translation):
    for name, t, shape in (("intrinsics", intrinsics, (F, 4)), ("rotation", rotation, (F, 3, 3)), ("translation", translation, (F, 3))):
        if t.dtype != _f32 or t.shape != shape:
            raise ValueError(f"{who}: {name} must be float32 {shape}, got {t.dtype} {tuple(t.shape)}")


def _finite_positive(who, names, values):
    for name, x in zip(names, values):
        if not 0 < float(x) < _INF:
            raise ValueError(f"{who}: {name} must be finite and > 0, got {x}")


def _frame_pointers(r, F, depth, seg, sizes, poses):
    """Fills the record's per-frame pointers: depth and seg (sizes = (H W, Hs Ws C) elements a frame) and poses = (K, R, t), each unless None."""
    if depth is not None:
        r.depth, r.seg = _native._ptr(depth, "depth", depth.dtype, F * sizes[0]), _native._ptr(seg, "seg", torch.uint8, F * sizes[1])
    if poses is not None:
        r.intrinsics = _native._ptr(poses[0], "intrinsics", _f32, F * 4)
        r.rotation, r.translation = _native._ptr(poses[1], "rotation", _f32, F * 9), _native._ptr(poses[2], "translation", _f32, F * 3)


# ---- depth frames fused into a signed distance volume (hotrack_amd/csrc/tsdf_fuse.hip) ------------------------------------------
class _TsdfFrames(ctypes.Structure):
    """pn2s_tsdf_frames (128 bytes)."""
    _fields_ = ([(n, _vp) for n in ("volume", "weight", "depth", "seg", "intrinsics", "rotation", "translation")] +
                [("depth_scale", ctypes.c_double)] + [(n, _cf) for n in ("voxel_scale", "trunc", "carve_weight", "max_weight")] +
                [(n, _ci) for n in ("res", "vol_f16", "frames", "h", "w", "hs", "ws", "c", "depth_u16", "flip_yz", "channel", "value")])


assert ctypes.sizeof(_TsdfFrames) == 128
_lib.pn2s_tsdf_integrate.argtypes = [ctypes.POINTER(_TsdfFrames), _vp]
_lib.pn2s_tsdf_integrate.restype = _ci
TSDF_MAX_RES = 512


def tsdf_check(volume, weight, voxel_scale, depth, seg, intrinsics, rotation, translation, trunc, obj_class, depth_scale,
               carve_weight, max_weight):
    """The argument checks of tsdf_integrate, which mirror pn2s_tsdf_integrate's (include/pn2_sdf.h) and raise; shared with the
    torch route (network/models/shape_fusion.py), so both refuse the same calls.  Devices are not looked at here.
    -> (res, F, H, W, Hs, Ws, C, f, depth is raw counts)."""
    who = "tsdf_integrate"
    _contiguous_tensors(who, _TSDF_TENSORS, (volume, weight, depth, seg, intrinsics, rotation, translation))
    res = _cubic_volume(who, volume, TSDF_MAX_RES)
    if weight.dtype != _f32 or weight.shape != volume.shape:
        raise ValueError(f"tsdf_integrate: weight must be float32 {tuple(volume.shape)}, got {weight.dtype} {tuple(weight.shape)}")
    frames = _observed_frames(who, depth, seg, obj_class, depth_scale)
    _pose_frames(who, frames[0], intrinsics, rotation, translation)
    _finite_positive(who, ("trunc", "voxel_scale", "max_weight"), (trunc, voxel_scale, max_weight))
    if not 0 <= float(carve_weight) < _INF:
        raise ValueError(f"tsdf_integrate: carve_weight must be finite and >= 0, got {carve_weight}")
    return (res,) + frames


def tsdf_integrate(volume: torch.Tensor, weight: torch.Tensor, voxel_scale: float, depth: torch.Tensor, seg: torch.Tensor,
                   intrinsics: torch.Tensor, rotation: torch.Tensor, translation: torch.Tensor, *, trunc: float, obj_class=(1, 255),
                   depth_scale: float = None, flip_yz: bool = False, carve_weight: float = 1.0, max_weight: float = 64.0):
    """Integrates F tracked depth frames, in order, into an SDF volume IN PLACE with one launch (include/pn2_sdf.h:
    pn2s_tsdf_integrate; the rule is stated at the head of hotrack_amd/csrc/tsdf_fuse.hip): per voxel the weighted running
    average of the truncated signed distances the frames observed.
    volume (res,res,res) float16 / float32, voxel centre ((ix,iy,iz) - res//2) * voxel_scale;  weight (res,res,res) float32;
    depth (F,H,W) fp32 metres, or uint16 / int16 raw counts with depth_scale;  seg (F,Hs,Ws,C) uint8, H = f Hs, W = f Ws;
    intrinsics (F,4) fx, fy, cx, cy;  rotation (F,3,3), translation (F,3): the tracked poses (cloud_obj = (pcld - t) @ R);
    obj_class: (channel, value) of the object's segment byte; every other valid pixel only carves free space, with carve_weight.
    All tensors contiguous on one GPU.  Runs on the current stream, no host sync.  -> (volume, weight), the same tensors."""
    res, F, H, W, Hs, Ws, C, _, raw = tsdf_check(volume, weight, voxel_scale, depth, seg, intrinsics, rotation, translation, trunc,
                                                 obj_class, depth_scale, carve_weight, max_weight)
    _on_one_gpu("tsdf_integrate", "shape_fusion", volume.device, _TSDF_TENSORS, (volume, weight, depth, seg, intrinsics, rotation, translation))
    r = _TsdfFrames(res=res, vol_f16=int(volume.dtype == torch.float16), frames=F, h=H, w=W, hs=Hs, ws=Ws, c=C, depth_u16=int(raw),
                    flip_yz=int(bool(flip_yz)), channel=int(obj_class[0]), value=int(obj_class[1]),
                    depth_scale=0.0 if depth_scale is None else float(depth_scale), voxel_scale=float(voxel_scale), trunc=float(trunc),
                    carve_weight=float(carve_weight), max_weight=float(max_weight))
    r.volume, r.weight = _native._ptr(volume, "volume", volume.dtype, res ** 3), _native._ptr(weight, "weight", _f32, res ** 3)
    _frame_pointers(r, F, depth, seg, (H * W, Hs * Ws * C), (intrinsics, rotation, translation))
    with torch.cuda.device(volume.device):
        rc = _lib.pn2s_tsdf_integrate(ctypes.byref(r), _native._stream(volume))
    _native._check(rc, "sdf.tsdf_integrate")
    return volume, weight


class _TsdfGroup(ctypes.Structure):
    """pn2s_tsdf_group (144 bytes)."""
    _fields_ = ([(n, _vp) for n in ("volumes", "weights", "frame_off", "depth", "seg", "intrinsics", "rotation", "translation")] +
                [("depth_scale", ctypes.c_double)] + [(n, _cf) for n in ("voxel_scale", "trunc", "carve_weight", "max_weight")] +
                [(n, _ci) for n in ("res", "vol_f16", "sequences", "frames", "h", "w", "hs", "ws", "c", "depth_u16", "flip_yz", "channel",
                                    "value", "pad_")])


assert ctypes.sizeof(_TsdfGroup) == 144
_lib.pn2s_tsdf_integrate_batch.argtypes = [ctypes.POINTER(_TsdfGroup), _vp]
_lib.pn2s_tsdf_integrate_batch.restype = _ci
TSDF_BATCH_MAX = 65535  # PN2S_TSDF_BATCH_MAX


def tsdf_batch_check(volumes, weights, voxel_scale, depth, seg, intrinsics, rotation, translation, frame_counts, trunc, obj_class,
                     depth_scale, carve_weight, max_weight):
    """The argument checks of tsdf_integrate_batch, shared with the torch route (network/models/shape_fusion.py), so both refuse
    the same calls: the lists' lengths, the counts, tsdf_check for every active sequence on its slice of the frames, one res and
    dtype, no storage shared between two active sequences.  Devices are not looked at here.
    -> (offsets: S + 1 ints, active: the sequences with frames)."""
    S = len(frame_counts)
    if len(volumes) != S or len(weights) != S:
        raise ValueError(f"tsdf_integrate_batch: volumes, weights and frame_counts must be lists of one length S, got {len(volumes)}, "
                         f"{len(weights)} and {S}")
    if S > TSDF_BATCH_MAX:
        raise ValueError(f"tsdf_integrate_batch: at most {TSDF_BATCH_MAX} sequences in one launch, got {S}")
    off = [0]
    for k, n in enumerate(frame_counts):
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"tsdf_integrate_batch: frame_counts[{k}] must be a non-negative int, got {n!r}")
        if (volumes[k] is None) != (weights[k] is None):
            raise ValueError(f"tsdf_integrate_batch: volumes[{k}] and weights[{k}] must both be given or both be None")
        if volumes[k] is None and n:
            raise ValueError(f"tsdf_integrate_batch: sequence {k} has {n} frames but no volume (None marks a sequence that sits out: "
                             "its count must be 0)")
        off.append(off[-1] + n)
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise ValueError("tsdf_integrate_batch: depth must be a (F,H,W) tensor holding the frames of all sequences")
    if off[-1] != depth.shape[0]:
        raise ValueError(f"tsdf_integrate_batch: frame_counts sum to {off[-1]}, the packed arrays hold F = {depth.shape[0]} frames")
    first, spans = None, []
    for k in range(S):
        v, w = volumes[k], weights[k]
        if v is None:
            continue
        if frame_counts[k]:
            a, b = off[k], off[k + 1]
            tsdf_check(v, w, voxel_scale, *(x[a:b] if isinstance(x, torch.Tensor) else x for x in (depth, seg, intrinsics, rotation, translation)),
                       trunc, obj_class, depth_scale, carve_weight, max_weight)
            for t in (v, w):
                spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), k))
        elif not (isinstance(v, torch.Tensor) and isinstance(w, torch.Tensor)):
            raise TypeError(f"tsdf_integrate_batch: volumes[{k}] and weights[{k}] must be tensors or None")
        if first is None:
            first = k
        elif (tuple(v.shape), v.dtype) != (tuple(volumes[first].shape), volumes[first].dtype):
            raise ValueError(f"tsdf_integrate_batch: volumes[{first}] ({tuple(volumes[first].shape)} {volumes[first].dtype}) and volumes[{k}] "
                             f"({tuple(v.shape)} {v.dtype}) differ: a group shares one res and dtype")
    spans.sort()
    for (_, end, i), (start, _, j) in zip(spans, spans[1:]):
        if start < end:
            if i == j:
                raise ValueError(f"tsdf_integrate_batch: sequence {i}'s volume and weights share storage")
            raise ValueError(f"tsdf_integrate_batch: sequences {min(i, j)} and {max(i, j)} share volume or weight storage: two "
                             "workgroups would write one voxel")
    return off, [k for k in range(S) if frame_counts[k]]


def tsdf_integrate_batch(volumes, weights, voxel_scale: float, depth: torch.Tensor, seg: torch.Tensor, intrinsics: torch.Tensor,
                         rotation: torch.Tensor, translation: torch.Tensor, frame_counts, *, trunc: float, obj_class=(1, 255),
                         depth_scale: float = None, flip_yz: bool = False, carve_weight: float = 1.0, max_weight: float = 64.0,
                         cache=None):
    """tsdf_integrate for the S volumes of a group of sequences with ONE launch (include/pn2_sdf.h: pn2s_tsdf_integrate_batch):
    sequence k integrates its frame_counts[k] frames, in order, into volumes[k] / weights[k] IN PLACE, with the bits tsdf_integrate
    gives for them alone.
    volumes, weights: lists of S tensors of one res and dtype (as tsdf_integrate's), None for a sequence that sits out;
    frame_counts: S non-negative ints, 0 for a sequence that sits out (its tensors, if given, keep every byte);
    depth (F,H,W), seg (F,Hs,Ws,C), intrinsics (F,4), rotation (F,3,3), translation (F,3): the sequences' frames packed in sequence
      order, F = sum(frame_counts); everything else is shared by the group and as in tsdf_integrate.
    No two active sequences may share volume or weight storage.  All tensors contiguous on one GPU.
    cache: a dict the caller keeps between calls: the pointer and offset table of a repeated (tensors, counts) is uploaded once.
    Runs on the current stream, no host sync.  -> (volumes, weights), the same lists."""
    off, active = tsdf_batch_check(volumes, weights, voxel_scale, depth, seg, intrinsics, rotation, translation, frame_counts, trunc,
                                   obj_class, depth_scale, carve_weight, max_weight)
    if not active:
        return volumes, weights
    S, F, v0 = len(frame_counts), off[-1], volumes[active[0]]
    device, res = v0.device, v0.shape[0]
    given = [k for k in range(S) if volumes[k] is not None]
    _on_one_gpu("tsdf_integrate_batch", "shape_fusion", device, lambda: [f"{n}[{k}]" for n in ("volumes", "weights") for k in given] + list(_FRAMES),
                [volumes[k] for k in given] + [weights[k] for k in given] + [depth, seg, intrinsics, rotation, translation])
    _, H, W = depth.shape
    _, Hs, Ws, C = seg.shape
    raw = depth.dtype in _RAW_DTYPES
    # one table: S volume pointers, S weight pointers, then the S + 1 offsets as int32 (a sitting-out sequence's tensors are not
    # checked beyond res and dtype, and never read: its entries stay NULL)
    key = ("tsdf", str(device), tuple(None if volumes[k] is None else (id(volumes[k]), id(weights[k])) for k in range(S)),
           tuple(frame_counts))
    hit = None if cache is None else cache.get(key)
    if hit is None:
        on = set(active)
        words = [volumes[k].data_ptr() if k in on else 0 for k in range(S)] + [weights[k].data_ptr() if k in on else 0 for k in range(S)]
        host = torch.cat([torch.tensor(words, dtype=torch.int64), torch.tensor(off + [0] * (S % 2 == 0), dtype=torch.int32).view(torch.int64)])
        # (pinned and asynchronous: no host synchronisation; the tensors are kept with the table: the key's ids stay theirs)
        hit = (host.pin_memory().to(device, non_blocking=True), list(volumes), list(weights))
        if cache is not None:
            if len(cache) > 64:
                cache.clear()
            cache[key] = hit
    table = hit[0]
    r = _TsdfGroup(res=res, vol_f16=int(v0.dtype == torch.float16), sequences=S, frames=F, h=H, w=W, hs=Hs, ws=Ws, c=C,
                   depth_u16=int(raw), flip_yz=int(bool(flip_yz)), channel=int(obj_class[0]), value=int(obj_class[1]),
                   depth_scale=0.0 if depth_scale is None else float(depth_scale), voxel_scale=float(voxel_scale), trunc=float(trunc),
                   carve_weight=float(carve_weight), max_weight=float(max_weight))
    r.volumes, r.weights, r.frame_off = table.data_ptr(), table.data_ptr() + 8 * S, table.data_ptr() + 16 * S
    _frame_pointers(r, F, depth, seg, (H * W, Hs * Ws * C), (intrinsics, rotation, translation))
    with torch.cuda.device(device):
        rc = _lib.pn2s_tsdf_integrate_batch(ctypes.byref(r), _native._stream(v0))
    _native._check(rc, "sdf.tsdf_integrate_batch")
    return volumes, weights


# ---- an SDF volume rendered to depth and normal maps (hotrack_amd/csrc/sdf_raycast.hip) -----------------------------------------
class _Raycast(ctypes.Structure):
    """pn2s_raycast (96 bytes)."""
    _fields_ = ([(n, _vp) for n in ("volume", "intrinsics", "rotation", "translation", "depth", "normal")] +
                [(n, _cf) for n in ("voxel_scale", "step_scale", "min_step")] +
                [(n, _ci) for n in ("res", "vol_f16", "frames", "h", "w", "flip_yz", "refine", "max_steps", "pad_")])


class _RaycastFrames(ctypes.Structure):
    """pn2s_raycast_frames (80 bytes)."""
    _fields_ = ([(n, _vp) for n in ("rendered", "depth", "seg", "out")] + [("depth_scale", ctypes.c_double), ("occl_margin", _cf)] +
                [(n, _ci) for n in ("frames", "h", "w", "hs", "ws", "c", "depth_u16", "channel", "value")])


assert ctypes.sizeof(_Raycast) == 96 and ctypes.sizeof(_RaycastFrames) == 80
_lib.pn2s_volume_raycast.argtypes = [ctypes.POINTER(_Raycast), _vp]
_lib.pn2s_volume_raycast.restype = _ci
_lib.pn2s_raycast_compare.argtypes = [ctypes.POINTER(_RaycastFrames), _vp]
_lib.pn2s_raycast_compare.restype = _ci
RAYCAST_MAX_RES = 512
# A choice, not a measurement: a non-object pixel counts as an occluder of the model when its depth is more than this in front of
# the rendered one.  1 cm is above what the tracker's pose error and a depth sensor's noise move a surface by (millimetres) and
# below the thickness of a finger, so a hand on the object is counted and a background pixel grazing the silhouette is not.
OCCL_MARGIN = 0.01


def raycast_check(volume, voxel_scale, intrinsics, rotation, translation, hw, step_scale, min_step, refine, max_steps):
    """The argument checks of volume_raycast, which mirror pn2s_volume_raycast's (include/pn2_sdf.h) and raise; shared with the torch
    route (network/models/volume_render.py), so both refuse the same calls.  Devices are not looked at here.
    -> (res, F, H, W, max_steps) with max_steps = 8 * res when None was given."""
    who = "volume_raycast"
    _contiguous_tensors(who, _RAYCAST_TENSORS, (volume, intrinsics, rotation, translation))
    res = _cubic_volume(who, volume, RAYCAST_MAX_RES, " in the linear layout")
    if intrinsics.dim() != 2 or intrinsics.shape[0] < 1:
        raise ValueError(f"volume_raycast: intrinsics must be (F,4) with F >= 1, got {tuple(intrinsics.shape)}")
    F = intrinsics.shape[0]
    _pose_frames(who, F, intrinsics, rotation, translation)
    H, W = int(hw[0]), int(hw[1])
    if H < 1 or W < 1 or H * W >= 1 << 29 or H > 8 * 65535 or F > 65535:
        raise ValueError(f"volume_raycast: an image of {H} x {W}, {F} frames: sizes >= 1, H W < 2^29, H <= 8 * 65535, at most 65535 frames")
    _finite_positive(who, ("voxel_scale", "step_scale", "min_step"), (voxel_scale, step_scale, min_step))
    if int(refine) != refine or not 0 <= int(refine) <= 16:
        raise ValueError(f"volume_raycast: refine must be an integer in [0, 16], got {refine}")
    max_steps = 8 * res if max_steps is None else max_steps
    if int(max_steps) != max_steps or not 1 <= int(max_steps) < 1 << 31:
        raise ValueError(f"volume_raycast: max_steps must be an integer >= 1, got {max_steps}")
    return res, F, H, W, int(max_steps)


def volume_raycast(volume: torch.Tensor, voxel_scale: float, intrinsics: torch.Tensor, rotation: torch.Tensor, translation: torch.Tensor,
                   hw, flip_yz: bool = False, normals: bool = True, step_scale: float = 1.0, min_step: float = 0.5, refine: int = 8,
                   max_steps: int = None):
    """Renders an SDF volume at F poses with one launch (include/pn2_sdf.h: pn2s_volume_raycast; the rule is stated at the head of
    hotrack_amd/csrc/sdf_raycast.hip): the inverse of tsdf_integrate's geometry, the ray parameter being the depth.
    volume (res,res,res) float16 / float32, linear layout;  intrinsics (F,4) fx, fy, cx, cy;  rotation (F,3,3), translation (F,3): the
    tracked poses (cloud_obj = (pcld - t) @ R);  hw = (H, W);  step_scale / min_step (voxels): the march's step is
    max(s * step_scale, min_step * voxel_scale) along the ray;  refine: bisections of the bracket;  max_steps: None = 8 * res.
    All tensors contiguous on one GPU.  Runs on the current stream, no host sync.
    -> (depth (F,H,W) float32, 0 = no hit;  normal (F,H,W,3) float32 unit vectors in the camera frame, or None with normals=False)."""
    res, F, H, W, max_steps = raycast_check(volume, voxel_scale, intrinsics, rotation, translation, hw, step_scale, min_step, refine,
                                            max_steps)
    _on_one_gpu("volume_raycast", "volume_render", volume.device, _RAYCAST_TENSORS, (volume, intrinsics, rotation, translation))
    depth = torch.empty((F, H, W), dtype=_f32, device=volume.device)
    normal = torch.empty((F, H, W, 3), dtype=_f32, device=volume.device) if normals else None
    r = _Raycast(res=res, vol_f16=int(volume.dtype == torch.float16), frames=F, h=H, w=W, flip_yz=int(bool(flip_yz)), refine=int(refine),
                 max_steps=max_steps, voxel_scale=float(voxel_scale), step_scale=float(step_scale), min_step=float(min_step))
    r.volume = _native._ptr(volume, "volume", volume.dtype, res ** 3)
    _frame_pointers(r, F, None, None, None, (intrinsics, rotation, translation))
    r.depth, r.normal = depth.data_ptr(), None if normal is None else normal.data_ptr()
    with torch.cuda.device(volume.device):
        rc = _lib.pn2s_volume_raycast(ctypes.byref(r), _native._stream(volume))
    _native._check(rc, "sdf.volume_raycast")
    return depth, normal


def raycast_compare_check(rendered, depth, seg, obj_class, depth_scale, occl_margin):
    """The argument checks of raycast_compare (pn2s_raycast_compare's, raised), shared with the torch route.
    -> (F, H, W, Hs, Ws, C, f, depth is raw counts)."""
    _contiguous_tensors("raycast_compare", ("rendered", "depth", "seg"), (rendered, depth, seg))
    frames = _observed_frames("raycast_compare", depth, seg, obj_class, depth_scale, rendered)
    if not 0 <= float(occl_margin) < _INF:
        raise ValueError(f"raycast_compare: occl_margin must be finite and >= 0, got {occl_margin}")
    return frames


def raycast_compare(rendered: torch.Tensor, depth: torch.Tensor, seg: torch.Tensor, obj_class=(1, 255), depth_scale: float = None,
                    occl_margin: float = OCCL_MARGIN) -> torch.Tensor:
    """Compares F rendered frames with the observed ones in one launch (include/pn2_sdf.h: pn2s_raycast_compare).
    rendered (F,H,W) float32 (volume_raycast's depth);  depth (F,H,W) and seg (F,Hs,Ws,C), obj_class, depth_scale: as tsdf_integrate's.
    -> (F,4) float32: |A n B|, |A u B|, the sum over A n B of |D - Z| and |Occ|, with A the object's pixels with valid depth, Occ the
    other valid pixels more than occl_margin in front of a model hit, B the model's hits outside Occ.  No host sync."""
    F, H, W, Hs, Ws, C, _, raw = raycast_compare_check(rendered, depth, seg, obj_class, depth_scale, occl_margin)
    _on_one_gpu("raycast_compare", "volume_render", rendered.device, ("rendered", "depth", "seg"), (rendered, depth, seg))
    out = torch.empty((F, 4), dtype=_f32, device=rendered.device)
    r = _RaycastFrames(frames=F, h=H, w=W, hs=Hs, ws=Ws, c=C, depth_u16=int(raw), channel=int(obj_class[0]), value=int(obj_class[1]),
                       depth_scale=0.0 if depth_scale is None else float(depth_scale), occl_margin=float(occl_margin))
    r.rendered, r.out = _native._ptr(rendered, "rendered", _f32, F * H * W), out.data_ptr()
    _frame_pointers(r, F, depth, seg, (H * W, Hs * Ws * C), None)
    with torch.cuda.device(rendered.device):
        rc = _lib.pn2s_raycast_compare(ctypes.byref(r), _native._stream(rendered))
    _native._check(rc, "sdf.raycast_compare")
    return out


# ---- the tracked pose refined by Gauss-Newton on the volume (hotrack_amd/csrc/sdf_refine.hip) -----------------------------------
class _Refine(ctypes.Structure):
    """pn2s_refine (88 bytes)."""
    _fields_ = ([(n, _vp) for n in ("pcld", "cloud_off", "volume", "vols", "poses", "stats", "trace")] +
                [(n, _cf) for n in ("bbox_min", "stride", "band")] + [(n, _ci) for n in ("problems", "n", "res", "vol_fmt", "iters")])


assert ctypes.sizeof(_Refine) == 88
for _n in ("pn2s_obj_refine", "pn2s_obj_refine_batch"):
    getattr(_lib, _n).argtypes = [ctypes.POINTER(_Refine), _vp]
    getattr(_lib, _n).restype = _ci
REFINE_MAX_ITERS, REFINE_TRACE_ROW, REFINE_BATCH_MAX = 64, 72, 65535   # PN2S_REFINE_*
REFINE_ITERS, REFINE_BAND = 8, 0.02   # the band: the reference's inlier distance for the object surface (optimization_obj.py:314)


def refine_check(pcld, rotation, translation, iters, band, voxel_scale):
    """The argument checks of obj_refine, which mirror pn2s_obj_refine's (include/pn2_sdf.h) and raise; shared with the torch route
    (network/models/pose_refine.py), so both refuse the same calls.  Devices and the volume are not looked at here.  -> n"""
    who = "obj_refine"
    for name, x in (("pcld", pcld), ("rotation", rotation), ("translation", translation)):
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(x).__name__}")
    if pcld.numel() < 3 or pcld.numel() % 3 or pcld.shape[-1] != 3:
        raise ValueError(f"obj_refine: pcld must be (N,3) or (1,N,3) with N >= 1, got {tuple(pcld.shape)}")
    if rotation.numel() != 9 or translation.numel() != 3:
        raise ValueError(f"obj_refine: rotation must hold 9 and translation 3 elements, got {tuple(rotation.shape)} and {tuple(translation.shape)}")
    if int(iters) != iters or not 0 <= int(iters) <= REFINE_MAX_ITERS:
        raise ValueError(f"obj_refine: iters must be an integer in [0, {REFINE_MAX_ITERS}], got {iters}")
    _finite_positive(who, ("band", "voxel_scale"), (band, voxel_scale))
    return pcld.numel() // 3


def _corner_volume(who, volume):
    if not isinstance(volume, CornerVolume):
        raise TypeError(f"{who}: the volume must be a hotrack_amd.sdf.CornerVolume (the kernel reads the corner layout), got {type(volume).__name__}")
    return volume


def obj_refine(pcld: torch.Tensor, rotation: torch.Tensor, translation: torch.Tensor, volume: CornerVolume, voxel_scale: float,
               iters: int = REFINE_ITERS, band: float = REFINE_BAND, trace: bool = False, bbox_min: float = BBOX_MIN):
    """`iters` damped Gauss-Newton steps on sum_j w_j phi(R^T (p_j - t))^2 from (rotation, translation), ONE launch, no host sync
    (include/pn2_sdf.h: pn2s_obj_refine; the rule is at the head of hotrack_amd/csrc/sdf_refine.hip).
    pcld (N,3)|(1,N,3); rotation (3,3)|(1,3,3); translation (3,)|(1,3,1); volume: a CornerVolume.
    -> (rotation (1,3,3), translation (1,3,1), stats (8,)[, trace (iters + 1, REFINE_TRACE_ROW)]) as new tensors; stats = initial cost,
    final cost, initial and final weighted count, accepted steps, final lambda, 0, 0.  The final cost is never above the initial."""
    n = refine_check(pcld, rotation, translation, iters, band, voxel_scale)
    vol = _corner_volume("obj_refine", volume)
    _on_one_gpu("obj_refine", "pose_refine", vol.data.device, ("pcld", "rotation", "translation"), (pcld, rotation, translation))
    pcld = pcld.reshape(-1, 3).contiguous()
    dev = pcld.device
    pose = _pose12(rotation, translation)
    stats = torch.empty((8,), dtype=_f32, device=dev)
    tr = torch.empty((int(iters) + 1, REFINE_TRACE_ROW), dtype=_f32, device=dev) if trace else None
    r = _Refine(problems=1, n=n, res=vol.res, vol_fmt=2 + vol.f16, iters=int(iters), bbox_min=float(bbox_min), stride=float(voxel_scale),
                band=float(band))
    r.pcld, r.volume = _native._ptr(pcld, "pcld", _f32, n * 3), vol.data.data_ptr()
    r.poses, r.stats, r.trace = pose.data_ptr(), stats.data_ptr(), None if tr is None else tr.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.pn2s_obj_refine(ctypes.byref(r), _native._stream(pcld))
    _native._check(rc, "sdf.obj_refine")
    out = (pose[:9].view(1, 3, 3), pose[9:].view(1, 3, 1), stats)
    return out + (tr,) if trace else out


def obj_refine_batch(pclds, rotations, translations, volumes, voxel_scale: float, iters: int = REFINE_ITERS, band: float = REFINE_BAND,
                     trace: bool = False, bbox_min: float = BBOX_MIN, cache=None):
    """obj_refine for S independent problems with ONE launch (pn2s_obj_refine_batch); every problem's result is bit for bit what
    obj_refine returns for it alone.  pclds: a list of S clouds, an empty one or None marking an INACTIVE problem (its pose comes back
    unchanged, its stats and trace rows are zero);  rotations / translations: two lists of S tensors, or (S,3,3) and (S,3)|(S,3,1);
    volumes: S CornerVolumes of one dtype and resolution, None allowed for an inactive problem;  cache: as obj_optimize_batch's.
    -> (rotations (S,3,3), translations (S,3,1), stats (S,8)[, trace (S, iters + 1, REFINE_TRACE_ROW)])."""
    S, pose = _pose_rows("obj_refine_batch", rotations, translations)
    if len(pclds) != S or len(volumes) != S or S > REFINE_BATCH_MAX:
        raise ValueError(f"obj_refine_batch: pclds and volumes must hold S = {S} <= {REFINE_BATCH_MAX} entries, got {len(pclds)} and {len(volumes)}")
    if int(iters) != iters or not 0 <= int(iters) <= REFINE_MAX_ITERS:
        raise ValueError(f"obj_refine_batch: iters must be an integer in [0, {REFINE_MAX_ITERS}], got {iters}")
    _finite_positive("obj_refine_batch", ("band", "voxel_scale"), (band, voxel_scale))
    dev = pose.device
    stats = torch.zeros((S, 8), dtype=_f32, device=dev)
    tr = torch.zeros((S, int(iters) + 1, REFINE_TRACE_ROW), dtype=_f32, device=dev) if trace else None
    out = (pose[:, :9].view(S, 3, 3), pose[:, 9:].reshape(S, 3, 1), stats)
    out = out + (tr,) if trace else out
    packed, sizes, active, off = _pack_clouds("obj_refine_batch", pclds, S, dev, cache)
    if not active:
        return out
    for k in active:
        _corner_volume(f"obj_refine_batch: volumes[{k}]", volumes[k])
    _on_one_gpu("obj_refine_batch", "pose_refine", dev, ("pclds", "poses"), (packed, pose))
    table, fmt, res = _volume_table(volumes, active, dev, cache)
    r = _Refine(problems=S, n=0, res=res, vol_fmt=fmt, iters=int(iters), bbox_min=float(bbox_min), stride=float(voxel_scale), band=float(band))
    r.pcld, r.cloud_off = _native._ptr(packed, "pclds", _f32, sum(sizes) * 3), _native._ptr(off, "cloud_offsets", torch.int32, S + 1)
    r.vols, r.poses, r.stats, r.trace = table.data_ptr(), pose.data_ptr(), stats.data_ptr(), None if tr is None else tr.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.pn2s_obj_refine_batch(ctypes.byref(r), _native._stream(pose))
    _native._check(rc, "sdf.obj_refine_batch")
    return out
