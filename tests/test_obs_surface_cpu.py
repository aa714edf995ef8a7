"""CPU: what the observed-surface feature checks without a device -- the layout of ObservedSurface.shape_update_samples (the
hand-over point of a later shape refit; reference update_shape, optimization_obj.py:362-369), the config default of
opt.accumulate_surface and its command-line flag, and the argument checks of ext.cloud_normals / pn2x_cloud_normals."""
import argparse
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "network"))


def _surface(M=50, seed=0):
    from models.obs_surface import ObservedSurface
    g = torch.Generator().manual_seed(seed)
    s = ObservedSurface(M)
    s.points = torch.randn((M, 3), generator=g) * 0.05
    n = torch.randn((M, 3), generator=g)
    s.normals = n / n.norm(dim=1, keepdim=True)
    s.normals[3] = 0   # (a point whose normal could not be estimated)
    s.frames = 1
    return s


def test_shape_update_samples_layout():
    s, M = _surface(), 50
    xyz, sdf_gt = s.shape_update_samples(torch.Generator().manual_seed(1))
    assert xyz.shape == (3 * M, 3) and sdf_gt.shape == (3 * M, 1) and xyz.dtype == torch.float32
    mu_pos, zero, mu_neg = sdf_gt[:M], sdf_gt[M:2 * M], -sdf_gt[2 * M:]
    assert (zero == 0).all()
    assert (mu_pos >= 0).all() and (mu_pos < 0.1).all() and (mu_neg >= 0).all() and (mu_neg < 0.05).all()
    assert mu_pos.max() > 0.05 and mu_neg.max() > 0.025   # (drawn over the whole range, not a constant)
    assert torch.equal(xyz[:M], s.points + s.normals * mu_pos)       # outside
    assert torch.equal(xyz[M:2 * M], s.points)                        # on
    assert torch.equal(xyz[2 * M:], s.points - s.normals * mu_neg)   # inside
    assert torch.equal(xyz[3], s.points[3]) and torch.equal(xyz[2 * M + 3], s.points[3])   # zero normal: the point itself
    again = s.shape_update_samples(torch.Generator().manual_seed(1))
    assert torch.equal(again[0], xyz) and torch.equal(again[1], sdf_gt)


def test_shape_update_samples_clamp(monkeypatch):
    """sdf_gt is clamped at +-0.2 (the reference's clamp_dist); offsets above it still move the point by the full offset."""
    s = _surface(8)
    monkeypatch.setattr(torch, "rand", lambda shape, **kw: torch.full(shape, 3.0, dtype=kw.get("dtype")))
    xyz, sdf_gt = s.shape_update_samples()
    assert torch.equal(sdf_gt[:8], torch.full((8, 1), 0.2)) and torch.equal(sdf_gt[16:], -(torch.full((8, 1), 3.0) * 0.05))
    assert torch.equal(xyz[:8], s.points + s.normals * (torch.full((8, 1), 3.0) * 0.1))


def test_surface_arguments():
    from models.obs_surface import ObservedSurface
    for bad in (dict(M=2), dict(M=2049), dict(M=64, k=2), dict(M=64, k=65), dict(M=64, orient="up"), dict(M=64, keep_dist=0.0)):
        with pytest.raises(ValueError):
            ObservedSurface(**bad)
    with pytest.raises(RuntimeError, match="before start"):
        ObservedSurface(64).add(torch.zeros((64, 3)), None, None, 0.002)


def test_selection_keys_are_unique_and_put_unusable_points_last():
    from models.obs_surface import KEY_RANGE, selection_keys
    draws = torch.tensor([5, 5, 0, KEY_RANGE - 1, 5])
    usable = torch.tensor([True, False, False, True, True])
    keys = selection_keys(draws, usable)
    assert keys.unique().numel() == 5 and keys.dtype == torch.int64
    assert torch.argsort(keys).tolist() == [0, 4, 3, 2, 1]
    assert torch.argsort(selection_keys(draws)).tolist() == [2, 0, 1, 4, 3]


def test_config_default_and_flag(tmp_path, monkeypatch):
    monkeypatch.setenv("HOTRACK_DATA_ROOT", str(tmp_path))
    from configs.config import get_config
    from parse_args import add_args
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    off = get_config(p.parse_args(["--config", "objopt_test_HO3D.yml"]), save=False)
    assert off["opt"]["accumulate_surface"] is False and off["opt"]["contact_threshold"] == 0.005
    on = get_config(p.parse_args(["--config", "objopt_test_HO3D.yml", "--accumulate_obj_surface"]), save=False)
    assert on["opt"]["accumulate_surface"] is True


def test_cloud_normals_argument_checks_in_words():
    from hotrack_amd import ext
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ext.cloud_normals([[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"\(B,N,3\)"):
        ext.cloud_normals(z(100, 3))
    with pytest.raises(ValueError, match="3 to 2048 points"):
        ext.cloud_normals(z(1, 2049, 3))
    with pytest.raises(ValueError, match="3 to 2048 points"):
        ext.cloud_normals(z(1, 2, 3))
    for k in (2, 65):
        with pytest.raises(ValueError, match="3 to 64 neighbours"):
            ext.cloud_normals(z(1, 100, 3), k=k)
    with pytest.raises(ValueError, match="at most 65535 clouds"):
        ext.cloud_normals(z(65536, 3, 3))
    with pytest.raises(ValueError, match="orient"):
        ext.cloud_normals(z(1, 100, 3), orient="camera")
    with pytest.raises(TypeError, match="float32"):
        ext.cloud_normals(z(1, 100, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"valid must be \(1,100\)"):
        ext.cloud_normals(z(1, 100, 3), valid=z(100, dtype=torch.bool))
    with pytest.raises(TypeError, match="bool or uint8"):
        ext.cloud_normals(z(1, 100, 3), valid=z(1, 100))
    with pytest.raises(ValueError, match=r"viewpoint must be \(1,3\) or \(3,\)"):
        ext.cloud_normals(z(1, 100, 3), viewpoint=z(2, 3))
    with pytest.raises(RuntimeError, match="GPU"):   # everything else is in order: the library has no CPU path
        ext.cloud_normals(z(1, 100, 3))


def test_c_entry_refuses_bad_arguments_before_any_device_work():
    from hotrack_amd import ext
    lib = ext._lib
    assert (ext.CLOUD_NORMALS_MAX_B, ext.CLOUD_NORMALS_MAX_N, ext.CLOUD_NORMALS_MAX_K) == (65535, 2048, 64)   # read from the library
    one = ctypes.c_void_p(64)   # never dereferenced: every call below is refused by the host-side check
    call = lambda b, n, k, o, pts=one, view=one, nrm=one, var=one: lib.pn2x_cloud_normals(b, n, k, o, pts, None, view, nrm, var, None)
    EINVAL, ENULL, ERANGE = -1, -2, -3
    for args in ((0, 100, 30, 0), (1, 2, 30, 0), (1, 2049, 30, 0), (1, 100, 2, 0), (1, 100, 65, 0), (1, 100, 30, -1), (1, 100, 30, 3)):
        assert call(*args) == EINVAL, args
    assert call(65536, 100, 30, 0) == ERANGE
    for kw in ({"pts": None}, {"view": None}, {"nrm": None}, {"var": None}):
        assert call(1, 100, 30, 1, **kw) == ENULL, kw
