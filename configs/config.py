"""YAML composition + command-line overrides (counterpart of the reference's configs/config.py:31-99):
all_config/<cfg> -> data_config/<data_config> -> pointnet_config/<pointnet_cfg.*>; any key can be
overridden from the CLI, nested keys with '/' (e.g. --network/backbone_out_dim 384).

Differences: the output root defaults to ./data but is created if missing (the reference asserts it
exists), no MANO directory is required (no MANO layer on this path), and `device` is the local rank's
GPU under torchrun."""
from __future__ import annotations

import os
from os.path import join as pjoin

import torch
import yaml

BASE = os.path.dirname(os.path.abspath(__file__))


def overwrite_config(cfg, key, key_path, value):
    cur = key_path[0]
    if len(key_path) == 1:
        old = cfg.get(cur)
        if old != value:
            print(f"{key} (originally {old}) overwritten by arg {value}")
            cfg[cur] = value
    else:
        overwrite_config(cfg.setdefault(cur, {}), key, key_path[1:], value)


def _load(*parts):
    with open(pjoin(BASE, *parts), "r") as f:
        return yaml.safe_load(f)


def peek_track(args):
    """The `track` value get_config will arrive at, from the command line or else the main YAML alone: nothing is created,
    composed or loaded (entry points check flag combinations with it before any work)."""
    track = getattr(args, "track", None)
    return track if track is not None else _load("all_config", args.config).get("track")


def get_config(args, save=True):
    cfg = _load("all_config", args.config)
    cli = dict(vars(args))
    cli.pop("config")
    for key, item in cli.items():
        if item is not None and key not in ("mode_name", "debug", "debug_save", "save", "num_workers", "synthetic_frames", "max_iters", "seq_batch"):
            overwrite_config(cfg, key, key.split("/"), item)
    if not isinstance(cfg.get("opt"), dict):
        cfg["opt"] = {}
    cfg["opt"].setdefault("fused_pose", False)  # hand-pose particle optimiser on the device-resident route (--fused_hand_pose)
    cfg.setdefault("fused_hand_eval", False)  # tracked hand sequences evaluated in two launches (--fused_hand_eval)
    cfg.setdefault("hand_interaction_eval", False)  # hand-object penetration / contact columns (--hand_interaction_eval)
    cfg["opt"].setdefault("contact_threshold", 0.005)  # metres: a fingertip region this near the surface is in contact
    cfg["opt"].setdefault("accumulate_surface", False)  # obj_opt: keep the observed surface of each sequence (--accumulate_obj_surface)
    cfg["opt"].setdefault("extract_mesh", False)  # obj_opt: extract the mesh of each sequence's SDF volume (--extract_obj_mesh)
    cfg["opt"].setdefault("fuse_depth", False)  # obj_opt: fuse the tracked depth frames into the sequence's volume (--fuse_obj_depth)
    cfg["opt"].setdefault("lockstep_fuse", False)  # fuse_depth inside lockstep groups: a volume copy per sequence (--lockstep_fuse)
    cfg["opt"].setdefault("fuse_every", 10)  # frames between flushes (the reference refits its shape every tenth frame)
    cfg["opt"].setdefault("fuse_trunc", 5.0)  # truncation distance, in voxels
    cfg["opt"].setdefault("fuse_prior_weight", 8.0)  # weight of the handed-over model, in frames
    cfg["opt"].setdefault("render_model", False)  # obj_opt: render each sequence's volume at the tracked poses (--render_obj_model)
    cfg["opt"].setdefault("render_occl_margin", 0.01)  # metres: a non-object pixel this far in front of the model occludes it (a choice)
    data_cfg = _load("data_config", cfg["data_config"])
    cfg["pointnet"] = {k: _load("pointnet_config", v) for k, v in cfg["pointnet_cfg"].items()}

    root = os.environ.get("HOTRACK_DATA_ROOT", "data")
    cfg["root_dir"] = root
    cfg["save_dir"] = pjoin(root, "exps", cfg.get("save_dir", cfg["experiment_dir"]), "results")
    cfg["experiment_dir"] = pjoin(root, "exps", cfg["experiment_dir"])
    os.makedirs(cfg["save_dir"], exist_ok=True)
    os.makedirs(cfg["experiment_dir"], exist_ok=True)
    if save and int(os.environ.get("RANK", "0")) == 0:
        with open(pjoin(cfg["experiment_dir"], "config.yml"), "w") as f:
            yaml.safe_dump({k: v for k, v in cfg.items()}, f, default_flow_style=False)

    cat = cfg["obj_category"][0] if isinstance(cfg["obj_category"], list) else cfg["obj_category"]
    cfg["num_parts"] = data_cfg[cat]["num_parts"]
    cfg["obj_sym"] = data_cfg[cat]["sym"]
    cfg["data_cfg"] = data_cfg
    cfg["data_cfg"]["basepath"] = pjoin(root, data_cfg["basepath"])
    if torch.cuda.is_available():
        local = int(os.environ.get("LOCAL_RANK", cfg.get("cuda_id", 0)))
        cfg["device"] = torch.device("cuda", local % torch.cuda.device_count())  # (% only matters for the shared-GPU self-test)
    else:
        cfg["device"] = "cpu"
    if isinstance(cfg.get("hand_model"), str):  # the same instance poses the synthetic sequences and drives the optimisers
        from models.hand_model import named_hand_model
        cfg["hand_model"] = named_hand_model(cfg["hand_model"])
    if cfg.get("track") == "hand_IKNet":  # IKNet runs when its checkpoint and a hand model exist (recorded as cfg["use_iknet"])
        from models.iknet import resolve_use_iknet
        resolve_use_iknet(cfg)
    print("Running on ", cfg["device"])
    return cfg
