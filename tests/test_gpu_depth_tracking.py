"""GPU: the trackers on frames that carry a depth image instead of their cloud (HandTrackModel / ObjTrackModel_Optimization ->
DepthFrontEnd.fill).  A 3-frame synthetic hand-object sequence and an object sequence are rendered at 120 x 160; tracking the
depth frames gives the bits of tracking the same frames with hand_points / obj_points / background_mask pre-filled from
DepthFrontEnd.clouds -- the hook adds nothing but the call -- and frames that have their clouds never reach the front end.
num_points as the configs have it (512 for the hand, 1024 for the object); a 41^3 volume, 256 candidate hands."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "network"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
H, W = 120, 160
K = dict(fx=150.0, fy=150.0, cx=80.0, cy=60.0)
HAND_RADIUS = 0.15
ENERGY_WEIGHT = {"penetrate_sum_loss": 1, "sil_loss": 0.1, "attraction_loss": 0.05, "vis_regu_loss": 10, "invis_regu_loss": 0,
                 "temporal_smooth": 1}
FLAGS = {"track_flag": True, "test_flag": True, "save_flag": False}


class CloudNet(torch.nn.Module):
    """Stands in for HandTrackNet: ground-truth keypoints, 2 mm of noise seeded by the frame's name, and a pull towards the
    cloud's centroid, so that the cloud it is handed shows in every output."""

    def __init__(self, cfg):
        super().__init__()
        self.device = cfg["device"]

    def forward(self, data, flags):
        s, k = data["file_name"][0].split("_")[-1].split("/")
        g = torch.Generator(device="cuda").manual_seed(1000 * int(s) + int(k))
        gt = data["gt_hand_kp"].to(self.device)
        pull = data["hand_points"].to(self.device).float().mean(dim=-2, keepdim=True) - gt.mean(dim=-2, keepdim=True)
        kp = gt + 0.002 * torch.randn(1, 21, 3, device=self.device, generator=g) + 0.05 * pull
        return {"pred_kp": kp, "pred_kp_vis_mask": torch.ones(1, 21, dtype=torch.bool, device=self.device)}


def _depth_frame(fr, hand_pts, obj_pts, hand_centre, obj_centre):
    """The frame with its clouds and mask replaced by a rendered 120 x 160 depth frame."""
    from datasets.synthetic import render_depth_frame
    depth, seg, _, _ = render_depth_frame(hand_pts, obj_pts, K, H, W, splat=1)
    out = {k: v for k, v in fr.items() if k not in ("hand_points", "obj_points", "background_mask")}
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).reshape(1, 3)
    out.update(depth=torch.from_numpy(depth)[None], seg=torch.from_numpy(seg)[None], intrinsics=dict(K), hand_centre=f(hand_centre),
               obj_centre=f(obj_centre), projection={"w": [W], "h": [H], **{k: [v] for k, v in K.items()}})
    return out


def _prefilled(frames, front):
    """The same frames with the clouds and the mask filled in beforehand, by the front end called directly."""
    out = []
    for fr in copy.deepcopy(frames):
        dev = front.device
        got = front.clouds({"depth": fr["depth"].to(dev), "seg": fr["seg"].to(dev), "hand_centre": fr["hand_centre"].to(dev),
                            "obj_centre": fr["obj_centre"].to(dev),
                            "intrinsics": torch.tensor([[K["fx"], K["fy"], K["cx"], K["cy"]]], device=dev)})
        fr.update(hand_points=got["hand_points"], obj_points=got["obj_points"], background_mask=got["background_mask"][0])
        out.append(fr)
    return out


def _bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.int32)


def _calls():
    from hotrack_amd import ext
    return ext.DEPTH_FRAME_CALLS


def test_hand_tracker_on_depth_frames():
    from datasets.synthetic import SyntheticHandObjectSequences, capsule_surface
    from models.frame_frontend import DepthFrontEnd
    from models.hand_model import SyntheticLBSHand
    from models.track_network import HandTrackModel

    def cfg(hm):
        return {"device": torch.device("cuda", 0), "num_points": 512, "hand_jitter_cfg": {"rand_scale": 0.004}, "obj_category": ["bottle"],
                "use_optimization": True, "hand_particles": 256, "hand_model": hm, "opt": {"energy_weight": dict(ENERGY_WEIGHT), "fused_pose": True}}

    def model():
        hm = SyntheticLBSHand()
        m = HandTrackModel(cfg(hm), handnet=CloudNet, hand_model=hm).eval()
        m.use_graph = False
        return m

    seq = SyntheticHandObjectSequences(cfg(SyntheticLBSHand()), 1, 3, res=41, stride=0.01)[0]
    rng = np.random.default_rng(5)
    frames = []
    for fr in seq:
        Ro, to = fr["gt_obj_pose"]["rotation"].reshape(3, 3).numpy(), fr["gt_obj_pose"]["translation"].reshape(3).numpy()
        frames.append(_depth_frame(fr, fr["hand_points"][0].numpy(), capsule_surface(rng, 2048) @ Ro.T + to, fr["gt_hand_kp"][0, 9].numpy(), to))
    filled = _prefilled(frames, DepthFrontEnd(512, device=torch.device("cuda", 0)))
    with torch.no_grad():
        before = _calls()
        ref = model()(filled, dict(FLAGS))
        assert _calls() == before, "frames that carry their clouds reached the front end"
        got = model()(frames, dict(FLAGS))
        assert _calls() == before + len(frames)
    for k, (a, b) in enumerate(zip(got, ref)):
        for name, x, y in [(f, a[f], b[f]) for f in ("pred_kp", "MANO_theta", "baseline_pred_kp")] + \
                          [("global_pose." + f, a["global_pose"][f], b["global_pose"][f]) for f in ("rotation", "translation")]:
            assert np.array_equal(_bits(x), _bits(y)), f"frame {k} {name}"
        assert np.array_equal(_bits(frames[k]["hand_points"]), _bits(filled[k]["hand_points"]))
        assert np.array_equal(frames[k]["background_mask"].cpu().numpy(), filled[k]["background_mask"].cpu().numpy())
        kp = a["pred_kp"].reshape(21, 3)
        assert torch.isfinite(kp).all()
        centre = frames[k]["hand_centre"].to(kp.device).reshape(1, 3)
        assert float((kp - centre).norm(dim=-1).max()) < HAND_RADIUS, f"frame {k}"


def test_object_tracker_on_depth_frames():
    from datasets.synthetic import SyntheticObjectSequences
    from models.frame_frontend import DepthFrontEnd
    from models.optimization_obj import gf_optimize_obj
    from models.track_network import ObjTrackModel_Optimization
    cfg = {"device": torch.device("cuda", 0), "data_cfg": {"dataset_name": "HO3D"}, "opt": {"updateobjshape": False},
           "num_points": 1024, "obj_category": ["bottle"], "obj_jitter_cfg": {"r": 5, "t": 0.03}, "track": "obj_opt"}

    def model():
        m = ObjTrackModel_Optimization(cfg)
        m.optimizer = gf_optimize_obj(cfg, seed=7)
        return m

    seq = SyntheticObjectSequences(cfg, 1, 3, res=41, stride=0.01)[0]
    frames = []
    for fr in seq:
        t = fr["gt_obj_pose"]["translation"].reshape(3).numpy()
        frames.append(_depth_frame(fr, None, fr["obj_points"][0].numpy(), t, t))
    filled = _prefilled(frames, DepthFrontEnd(1024, device=torch.device("cuda", 0)))
    with torch.no_grad():
        before = _calls()
        ref = model()(filled, dict(FLAGS))
        assert _calls() == before, "frames that carry their clouds reached the front end"
        got = model()(frames, dict(FLAGS))
        assert _calls() == before + len(frames)
        batch = model().forward_batch([copy.deepcopy([{k: v for k, v in fr.items() if k != "obj_points"} for fr in frames])], dict(FLAGS))[0]
    for k, (a, b, c) in enumerate(zip(got, ref, batch)):
        for name in ("rotation", "translation"):
            assert torch.isfinite(a[name]).all()
            assert np.array_equal(_bits(a[name]), _bits(b[name])), f"frame {k} {name}"
            assert np.array_equal(_bits(a[name]), _bits(c[name])), f"forward_batch frame {k} {name}"
        assert np.array_equal(_bits(frames[k]["obj_points"]), _bits(filled[k]["obj_points"]))
        gt = seq[k]["gt_obj_pose"]["translation"].reshape(3).to(a["translation"].device)
        assert float((a["translation"].reshape(3) - gt).norm()) < 0.25   # inside the crop ball it was built from
