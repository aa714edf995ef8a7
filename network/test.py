"""python network/test.py --config handtracknet_test_SimGrasp.yml [--num_points 1024]

Same entry point as the reference's network/test.py: per-sequence tracking (batch 1, frame t seeded by
frame t-1), prints data / network frames-per-second like the reference (test.py:65-98) -- here with an
explicit device synchronisation so the network time is real.  Enables the fused inference backend.
--seq_batch S (track: obj_opt only): S sequences at a time in lockstep, one batched optimiser call per frame step; with
--fuse_obj_depth it needs --lockstep_fuse (a volume copy per sequence; one fusion launch per flush for the whole group).
--render_obj_model (track: obj_opt, --from_depth): every sequence's volume rendered at its tracked poses and compared with the
observed frames -- "Test model_depth_residual(mm) / model_silhouette_iou / model_occluded_ratio" lines that need no ground truth;
with --save the last frame's maps as PNGs."""
import argparse
import logging
import os
import sys
import time

# (bench.py raises GPU_MAX_HW_QUEUES to 8 because its serving loop keeps four batches in flight on four HIP streams; this entry
# point tracks one sequence at batch 1 on ONE stream, where the runtime's default queue mapping changes nothing.  A service
# that runs several of these loops in one process sets GPU_MAX_HW_QUEUES >= its stream count in its environment.)
import torch

base_dir = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, base_dir)
sys.path.insert(0, os.path.join(base_dir, ".."))

from configs.config import get_config, peek_track  # noqa: E402
from datasets.synthetic import get_dataloader  # noqa: E402
from parse_args import add_args, check_seq_batch  # noqa: E402
from trainer import Trainer  # noqa: E402


def main(args):
    seq_batch = getattr(args, "seq_batch", 1)
    check_seq_batch(seq_batch, peek_track(args))  # (before any work: no directory, no model)
    cfg = get_config(args, save=False)
    if seq_batch > 1 and cfg["opt"].get("fuse_depth") and not cfg["opt"].get("lockstep_fuse"):
        raise SystemExit("--fuse_obj_depth with --seq_batch %d needs --lockstep_fuse: every sequence of a group then owns a copy of the "
                         "volume, its weights and its corner layout (201^3 fp16: about 49 MB plus 130 MB per sequence)" % seq_batch)
    logger = logging.getLogger("TestModel")
    logger.setLevel(logging.INFO)
    if torch.cuda.is_available():
        from hotrack_amd import fused
        from models import pointnet_utils
        pointnet_utils.set_fused_backend(fused)
    loader = get_dataloader(cfg, args.mode_name, length=args.synthetic_frames)
    trainer = Trainer(cfg, logger, len(loader))
    trainer.resume(len(loader))
    if seq_batch > 1:
        return main_seq_batch(args, loader, trainer, seq_batch)
    t_data = t_net = 0.0
    frames = 0
    acc = {}
    zero = time.time()
    for i, data in enumerate(loader):
        n = len(data) if isinstance(data, list) else 1
        frames += n
        start = time.time()
        t_data += start - zero
        loss, _ = trainer.test(data, save_flag=args.save)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t_net += time.time() - start
        print(f"Trajectory {i}: {n} frames, network {n / (time.time() - start):8.2f} FPS")
        for k, v in loss.items():
            acc[k] = acc.get(k, 0.0) + float(v)
        zero = time.time()
    print(f"Overall, {frames:8} frames")
    print(f"Data Preprocessing: {t_data:8.2f}s {frames / max(t_data, 1e-9):8.2f}FPS")
    print(f"Network Forwarding: {t_net:8.2f}s {frames / max(t_net, 1e-9):8.2f}FPS")
    for k, v in acc.items():
        print("Test {} is {}".format(k, v / max(len(loader), 1)))


def main_seq_batch(args, loader, trainer, seq_batch):
    """--seq_batch S: groups of S sequences (the last one may be smaller), each tracked in lockstep by Trainer.test_batch; the
    same lines as the loop above, one Trajectory line per sequence."""
    t_data = t_net = 0.0
    frames = 0
    acc = {}
    done = 0
    zero = time.time()

    def run(group):
        nonlocal t_data, t_net, frames, done, zero
        start = time.time()
        t_data += start - zero
        results = trainer.test_batch(group, save_flag=args.save)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        took = time.time() - start
        t_net += took
        total = sum(len(d) if isinstance(d, list) else 1 for d in group)
        for data, (loss, _) in zip(group, results):
            n = len(data) if isinstance(data, list) else 1
            frames += n
            print(f"Trajectory {done}: {n} frames, network {total / took:8.2f} FPS (group of {len(group)})")
            done += 1
            for k, v in loss.items():
                acc[k] = acc.get(k, 0.0) + float(v)
        zero = time.time()

    group = []
    for data in loader:
        group.append(data)
        if len(group) == seq_batch:
            run(group)
            group = []
    if group:
        run(group)
    print(f"Overall, {frames:8} frames")
    print(f"Data Preprocessing: {t_data:8.2f}s {frames / max(t_data, 1e-9):8.2f}FPS")
    print(f"Network Forwarding: {t_net:8.2f}s {frames / max(t_net, 1e-9):8.2f}FPS")
    for k, v in acc.items():
        print("Test {} is {}".format(k, v / max(len(loader), 1)))


if __name__ == "__main__":
    p = add_args(argparse.ArgumentParser())
    p.add_argument("--mode_name", default="test")
    main(p.parse_args())
