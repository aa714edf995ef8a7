"""Per-sequence hand tracking with HandTrackNet (counterpart of HandTrackModel.forward,
reference track_network.py:139-226, HandTrackNet-only branch :214-217).

Frame t is initialised from frame t-1: the previous prediction, expressed relative to the previous
cloud's centroid, is re-attached to the current cloud's centroid ("important for fast motion",
:163,:217).  The palm template comes from the sequence's first frame (the reference builds it from a
MANO layer, which needs licensed assets; the tracking logic is otherwise the same) -- or, with hand shape estimation
(`use_pred_hand_shape`), from the hand model's rest hand at the estimated shape code."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import pointnet_utils


class _FrontEndSlot:
    """A tracker's depth front end, built on first use: a frame that carries `depth` and lacks the tracker's cloud is completed by
    DepthFrontEnd.fill (models/frame_frontend.py); a frame that has the cloud is not touched."""

    def __init__(self, cfg):
        self.cfg = {"num_points": cfg.get("num_points", 1024), "device": cfg["device"], "depth_frontend": cfg.get("depth_frontend")}
        self.front = None

    def complete(self, data, cloud_key):
        if cloud_key in data or "depth" not in data:
            return
        if self.front is None:
            from .frame_frontend import DepthFrontEnd
            self.front = DepthFrontEnd.from_cfg(self.cfg)
        self.front.fill(data)


class _HandSequence:
    """One hand sequence being tracked: everything HandTrackModel carries from a frame to the next.  `forward` drives one,
    `forward_batch` one per sequence of its group: `step` runs a frame up to the pose optimiser, the caller runs the optimiser
    (`optimize`, or one `optimize_batch` for the group), `settle` takes its result.  `volume` / `voxel_scale` (the sequence's
    own volume), `beta` (the hand model's registered shape) and `history` (the shape optimiser's bone lengths so far) are the
    group's: `forward` keeps them in the optimisers themselves."""

    def __init__(self, model, frames, flag_dict, graph_ok, ik_graph_ok):
        self.model, self.flag_dict, self.graph_ok, self.ik_graph_ok = model, flag_dict, graph_ok, ik_graph_ok
        self.rets = []
        self.last_kp = self.prev_theta = self.shape_code = self.palm = self.volume = self.voxel_scale = None
        self.beta = getattr(getattr(model.optimizer, "mano_layer_right", None), "registered_beta", None)
        self.history = None if model.opt_shape is None else model.opt_shape.old_pred_length
        if model.opt_shape is not None:  # the zero shape's rest hand until the first estimate (:150-152)
            self.palm = model._shaped_palm_template(torch.zeros((1, model.opt_shape.optimize_dim), device=model.device))
        elif len(frames):
            self.palm = frames[0]["gt_hand_pose"]["palm_template"].to(model.device).float()

    def step(self, i, data):
        """Frame i up to the pose optimiser -> (ret, the cloud's centre, optimize()'s arguments by name and in its positional
        order; None where the pose optimiser does not run)."""
        m = self.model
        data["pred_palm_template"] = self.palm
        m._front_end.complete(data, "hand_points")
        points = data["hand_points"].to(m.device, non_blocking=True).float()
        centre = points.mean(dim=-2, keepdim=True)
        if self.last_kp is not None:
            data["jittered_hand_kp"] = self.last_kp + centre  # stays on the device: no host sync between frames
        if self.graph_ok:
            ret = m._graph_step(points, data["jittered_hand_kp"].to(m.device).float(), self.palm, self.flag_dict)
        else:
            ret = m.handnet(data, self.flag_dict)
        if not m.use_optimization and m.IKnet is None:
            return ret, centre, None
        ret["baseline_pred_kp"] = ret["pred_kp"].clone()
        if not m.use_optimization:  # IKNet's pose drives the hand model (track_network.py:196-200, hand_network.py:313-318)
            m._iknet(ret, data, self.palm, self.ik_graph_ok)
            ret["pred_kp"] = m.IKnet.pose_keypoints(ret["raw_quat"], ret["global_pose"], data.get("pred_beta"))
            return ret, centre, None
        # track_network.py:142-156, :203-211
        if m.opt_shape is not None:  # :174-193: the template takes effect from the next frame on
            if m._shape_due(i):
                self.shape_code = m.opt_shape.optimize(ret["baseline_pred_kp"], use_old=m.shape_mode == 3).clone()
                self.palm = m._shaped_palm_template(self.shape_code)
            data["pred_beta"] = self.shape_code
            ret["pred_beta"] = self.shape_code
        if m.IKnet is not None:
            theta0, pose0 = m._iknet(ret, data, self.palm, self.ik_graph_ok)
        else:  # (without IKNet: the stand-in for its two outputs)
            theta0, pose0 = m._pose_init(ret["baseline_pred_kp"], self.prev_theta)
        obj_pose = data["pred_obj_pose"] if (m.use_pred_obj_pose and "pred_obj_pose" in data) else data["gt_obj_pose"]
        return ret, centre, dict(init_mano=theta0, init_hand_pose=pose0, init_kp=ret["baseline_pred_kp"], last_frame_kp=self.last_kp,
                                 vis_mask=ret["pred_kp_vis_mask"], init_obj_pose=obj_pose, hand_shape=data.get("pred_beta"),
                                 projection=data["projection"], background_mask=data["background_mask"])

    def settle(self, ret, centre, optimum):
        """Ends the frame `step` began.  optimum: the pose optimiser's (keypoints, pose code, rotation, translation), or None."""
        if optimum is not None:
            kp, theta, rot, trans = optimum
            ret["pred_kp"], ret["MANO_theta"] = kp, theta
            ret["global_pose"] = {"rotation": rot.unsqueeze(0), "translation": trans.unsqueeze(-1)}
            self.prev_theta = theta
        self.last_kp = (ret["pred_kp"] - centre).clone()
        self.rets.append(ret)


class HandTrackModel(nn.Module):
    """hand_model (models/hand_model.HandModel, e.g. a MANO layer with the reference's call signature): enables the
    hand-pose particle optimisation of the reference's `use_optimization` branch (track_network.py:142-156, :203-211) on
    top of the HandTrackNet tracking loop.  In the reference that branch sits behind IKNet, which supplies the initial
    MANO pose code and global pose.  With `IKnet` (models/iknet.IKNet, needs a hand model) it does here too, and without the
    optimisation IKNet's pose drives the hand model's keypoints (`pred_kp`); without an IKNet those two inputs come from a
    stand-in with the same role (`_pose_init`): the pose code of the previous frame's optimum and the rigid fit of the hand
    model's keypoints to HandTrackNet's prediction (device Kabsch).  Everything downstream -- visibility mask, candidate
    evaluation, update rule, what is fed to the next frame -- is the reference's."""

    def __init__(self, cfg, handnet, IKnet=None, hand_model=None):
        super().__init__()
        self.device = cfg["device"]
        self.handnet = handnet(cfg)
        # IKNet (models/iknet.py; reference track_network.py:165-211): HandTrackNet's keypoints -> MANO pose code + global pose,
        # which seed the pose optimiser (use_optimization) or drive the hand model's keypoints (pred_kp) -- needs a hand model
        self.IKnet = None
        if IKnet is not None:
            if hand_model is None:
                raise ValueError("HandTrackModel: IKNet needs a hand model")
            self.IKnet = IKnet if isinstance(IKnet, nn.Module) else IKnet(cfg, hand_model=hand_model)
            print("[Hand Tracking] Use IKNet: True")
        self.use_graph = True  # GPU + fused backend: one captured HIP graph per (N, keypoints) shape, replayed per frame
        self._graphs = {}
        self._front_end = _FrontEndSlot(cfg)  # frames that carry a depth image instead of hand_points (models/frame_frontend.py)
        self.use_optimization = bool(cfg.get("use_optimization", False)) and hand_model is not None
        self.use_pred_obj_pose = bool(cfg.get("use_pred_obj_pose", False))
        self.sym = cfg.get("obj_sym", -1)  # rot_diff_rad's symmetry mode for the obj_pred_* metrics (compute_loss)
        # compute_loss through compute_loss_batch: every frame's dictionary from two launches (eval_metrics.hand_sequence_metrics)
        self.fused_hand_eval = bool(cfg.get("fused_hand_eval", False))
        # compute_loss / compute_loss_batch also report how the tracked hands sit against the object (eval_metrics.hand_interaction_metrics:
        # penetration depth and share, fingers in contact, tip gap); contact_threshold [m] is a choice, not a measurement
        self.hand_interaction_eval = bool(cfg.get("hand_interaction_eval", False))
        self.contact_threshold = float((cfg.get("opt") or {}).get("contact_threshold", 0.005))
        self.__dict__["_interaction_hand"] = hand_model  # (not a submodule of this one: the optimiser / IKNet own it)
        self.optimizer = None
        if self.use_optimization:
            from .optimization_hand import gf_optimize_hand_pose
            self.optimizer = gf_optimize_hand_pose(cfg, hand_model=hand_model, particle_size=int(cfg.get("hand_particles", 5120)))
            if self.optimizer.fused and self.optimizer.use_kernel():
                print("[Hand Tracking] hand-pose optimisation on the device-resident route (opt.fused_pose): "
                      "2 launches per iteration, no host sync")
        # shape-code estimation from HandTrackNet's keypoints (reference track_network.py:130-134, :174-193):
        # use_pred_hand_shape 1 = on frame 0, 2 = every 10 frames, 3 = every 10 frames over the bone lengths of all earlier
        # calls.  It runs where the reference's IKNet branch runs here (use_optimization with a hand model) and needs a
        # hand model with a shape space; otherwise the loop is unchanged and says why.
        mode = cfg.get("use_pred_hand_shape", 0)
        self.shape_mode = int(mode) if mode not in (None, False, True) else int(bool(mode))
        if self.shape_mode not in (0, 1, 2, 3):
            raise ValueError(f"use_pred_hand_shape: 0/False, 1, 2 or 3, got {mode!r}")
        self.opt_shape = None
        if self.shape_mode:
            why = ("use_optimization is off or there is no hand model" if not self.use_optimization else
                   "the hand model has no shape space (num_betas = 0)" if getattr(hand_model, "num_betas", 0) == 0 else None)
            if why is None:
                from .optimization_hand import gf_optimize_hand_shape
                self.opt_shape = gf_optimize_hand_shape(cfg, hand_model=self.optimizer.mano_layer_right,
                                                        particle_size=int(cfg.get("shape_particles", 5120)))
                print(f"[Hand Tracking] hand shape estimation: use_pred_hand_shape = {self.shape_mode} "
                      f"({'GPU kernel' if self.opt_shape.use_kernel() else 'torch route'})")
            else:
                print(f"[Hand Tracking] hand shape estimation skipped (use_pred_hand_shape = {self.shape_mode}): {why}")

    # A captured graph bakes in the pointers of the BN-folded weights FastEval built at capture time: anything that can
    # change the weights (checkpoint load, fine-tuning, .to()/.float()) drops the captured graphs.
    def train(self, mode: bool = True):
        if mode or mode != self.training:  # eval() on a model already in eval mode (Trainer.test per sequence) keeps the graphs
            self._graphs.clear()
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._graphs.clear()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._graphs.clear()
        return super().load_state_dict(*a, **k)

    def invalidate_graphs(self):
        """Call after editing parameters in place outside train() / load_state_dict() / .to()."""
        self._graphs.clear()

    # ------------------------------------------------------------------------------------
    def _graph_step(self, points, kp_init, palm_template, flag_dict):
        """One tracking step as a replay of a captured HIP graph (static input / output buffers): a frame is
        ~75 short kernels, so per-launch host cost would otherwise dominate the frame latency."""
        key = (tuple(points.shape), tuple(kp_init.shape), tuple(palm_template.shape), bool(flag_dict.get("IKNet_flag", False)))
        g = self._graphs.get(key)
        if g is None:
            buf = {"hand_points": points.clone(), "jittered_hand_kp": kp_init.clone(), "pred_palm_template": palm_template.clone()}
            with torch.no_grad():
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):  # warm-up: library handles, folded-weight caches, constant tensors
                        self.handnet(buf, flag_dict)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = self.handnet(buf, flag_dict)
            g = self._graphs[key] = (graph, buf, out)
        graph, buf, out = g
        buf["hand_points"].copy_(points, non_blocking=True)
        buf["jittered_hand_kp"].copy_(kp_init, non_blocking=True)
        buf["pred_palm_template"].copy_(palm_template, non_blocking=True)
        graph.replay()
        return {k: (v.clone() if torch.is_tensor(v) else {kk: vv.clone() for kk, vv in v.items()}) for k, v in out.items()}

    def _iknet_step(self, kp, palm_template, graph_ok):
        """IKNet on HandTrackNet's keypoints (1,21,3): (raw_quat, MANO_theta, canon_pose, init_kp_handframe).  On the kernel
        route with graphs on it is a replay of a captured graph keyed by shape next to HandTrackNet's (same invalidation rules;
        a change of IKNet's weights re-captures): the palm fit and seven launches, no host sync."""
        ik = self.IKnet
        if not (graph_ok and ik.kernel_route(kp)):
            return ik.solve(kp, palm_template)
        key = ("iknet", tuple(kp.shape), tuple(palm_template.shape))
        folded = ik.folded_weights()
        g = self._graphs.get(key)
        if g is None or g[3] is not folded:
            buf = (kp.clone(), palm_template.clone())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ik.solve(*buf)  # warm-up: constants, library handles
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = ik.solve(*buf)
            g = self._graphs[key] = (graph, buf, out, folded)
        graph, buf, out, _ = g
        buf[0].copy_(kp, non_blocking=True)
        buf[1].copy_(palm_template, non_blocking=True)
        graph.replay()
        raw, theta, canon, kp_hf = out
        return raw.clone(), theta.clone(), {k: v.clone() for k, v in canon.items()}, kp_hf.clone()

    def _pose_init(self, pred_kp, prev_theta):
        """Stand-in for IKNet's two outputs (see the class docstring): MANO_theta (1,45) and global_pose."""
        from hotrack_amd import ext
        hm = self.optimizer.mano_layer_right
        theta = prev_theta if prev_theta is not None else torch.zeros((1, hm.num_pose), device=pred_kp.device)
        with torch.no_grad():
            _, kp0 = hm.forward(th_pose_coeffs=torch.cat([torch.zeros((1, 3), device=pred_kp.device), theta], dim=1),
                                th_trans=torch.zeros((1, 3), device=pred_kp.device), use_registed_beta=True)
            R, t = ext.kabsch(kp0.contiguous(), pred_kp.contiguous())  # pred ~ R kp0 + t
        return theta, {"rotation": R.reshape(1, 3, 3), "translation": t.reshape(1, 3, 1)}

    def _shaped_palm_template(self, shape_code):
        """Palm keypoints of the rest hand with `shape_code` (1, num_betas) (reference handkp2palmkp of the shaped rest hand)."""
        from .hand_utils import handkp2palmkp
        hm = self.opt_shape.mano_layer_right
        with torch.no_grad():
            _, kp = hm.forward(th_pose_coeffs=torch.zeros((1, 3 + hm.num_pose), device=self.device),
                               th_trans=torch.zeros((1, 3), device=self.device), th_betas=shape_code)
        return handkp2palmkp(kp).float()

    def _shape_due(self, i):
        return (self.shape_mode == 1 and i == 0) or (self.shape_mode in (2, 3) and i % 10 == 0)

    def _begin_tracking(self, flag_dict):
        """What a tracking call sets before its first frame -> (graph_ok, ik_graph_ok): may HandTrackNet / IKNet replay graphs."""
        flag_dict["track_flag"] = True
        assert flag_dict["test_flag"]
        flag_dict["opt_flag"] = self.use_optimization
        if self.use_optimization or self.IKnet is not None:
            flag_dict["IKNet_flag"] = True  # HandTrackNet also returns the keypoint visibility mask (hand_network.py:149-155)
        # (IKNet's graph needs no fused HandTrackNet backend: its own kernels and the device Kabsch)
        ik_graph_ok = self.use_graph and not self.training and not torch.is_grad_enabled() and torch.device(self.device).type == "cuda"
        return ik_graph_ok and pointnet_utils.fused_backend() is not None, ik_graph_ok

    def _sequence_volume(self, frame0, built):
        """Loads the volume of a sequence whose first frame is `frame0` into the pose optimiser -> (volume on the device,
        voxel_scale).  `built` maps id(volume tensor) to its device copy: sequences of a group that hand over one tensor share it
        (the optimiser then keeps the volume loaded last: optimize_batch reads each call's own)."""
        opt = self.optimizer
        if "sdf_volume" in frame0:
            src, scale = frame0["sdf_volume"], frame0.get("voxel_scale")
            if id(src) in built:
                return built[id(src)][1], opt.voxel_scale if scale is None else float(scale)
            opt.load_volume(src, scale)
            built[id(src)] = (src, opt.sdf_volume)
        elif not _load_mesh_volume(opt, frame0, self.device) and opt.sdf_volume is None:
            raise RuntimeError("use_optimization: no SDF volume (decoding it from a DeepSDF latent needs the checkpoints); "
                               "put 'sdf_volume' / 'voxel_scale', or the object's mesh as 'obj_mesh' ({'vertices', 'faces'}) "
                               "or 'obj_mesh_path', into the sequence's first frame")
        return opt.sdf_volume, opt.voxel_scale

    def forward(self, input, flag_dict):
        seq = _HandSequence(self, input, flag_dict, *self._begin_tracking(flag_dict))
        if self.use_optimization:
            self._sequence_volume(input[0], {})
        for i, data in enumerate(input):
            ret, centre, call = seq.step(i, data)
            seq.settle(ret, centre, None if call is None else self.optimizer.optimize(*call.values()))
        return seq.rets

    def forward_batch(self, inputs, flag_dict):
        """`forward` for S sequences in lockstep.  At frame index t every sequence that still has a frame t runs its own
        HandTrackNet step, shape estimate and IKNet / `_pose_init` -- `_HandSequence.step`, which is what `forward` runs, on that
        sequence's own carried state -- and then ONE `gf_optimize_hand_pose.optimize_batch` call serves all of
        them: per iteration one evaluation launch over a (candidates, sequence) grid and one update launch with a workgroup per
        sequence, instead of S times two.  (A hand model with MANO entries runs that call in lockstep only with
        cfg['opt']['lockstep_mano']; without it optimize_batch runs optimize() per sequence.)  Sequences shorter than the longest
        sit out once they have ended.  All volumes must
        share one resolution, dtype and voxel_scale.  Returns a list of S `ret_dict_lst`, each what `forward` returns for that
        sequence alone on a tracker in this one's state at the call.  Without `use_optimization` it is `forward` per sequence."""
        if not self.use_optimization:
            return [self.forward(seq, flag_dict) for seq in inputs]
        graph_flags = self._begin_tracking(flag_dict)
        opt, shape, hm = self.optimizer, self.opt_shape, self.optimizer.mano_layer_right
        has_reg = hasattr(hm, "registered_beta")
        S = len(inputs)
        seqs, built = [_HandSequence(self, seq, flag_dict, *graph_flags) for seq in inputs], {}
        for st, seq in zip(seqs, inputs):
            if len(seq):
                st.volume, st.voxel_scale = self._sequence_volume(seq[0], built)
        for t in range(max((len(seq) for seq in inputs), default=0)):
            live = [k for k in range(S) if t < len(inputs[k])]
            calls, steps = [None] * S, {}
            for k in live:
                # the hand model's registered shape and the shape optimiser's history belong to shared objects: each sequence
                # puts its own in for its step and takes the history back
                st = seqs[k]
                if has_reg:
                    hm.registered_beta = st.beta
                if shape is not None:
                    shape.old_pred_length = st.history
                ret, centre, call = st.step(t, inputs[k][t])
                if shape is not None:
                    st.history = shape.old_pred_length
                steps[k] = (ret, centre)
                calls[k] = dict(call, sdf_volume=st.volume, voxel_scale=st.voxel_scale)
            outs = opt.optimize_batch(calls)
            for k in live:
                seqs[k].settle(*steps[k], outs[k])
                if calls[k]["hand_shape"] is not None and getattr(hm, "num_betas", 0) > 0:  # what optimize() registers
                    seqs[k].beta = torch.as_tensor(calls[k]["hand_shape"]).reshape(1, -1).to(self.device).float()
        return [st.rets for st in seqs]

    def _iknet(self, ret, data, palm_template, graph_ok):
        data["baseline_pred_kp"] = ret["baseline_pred_kp"]
        raw, theta, canon, _ = self._iknet_step(ret["baseline_pred_kp"], palm_template, graph_ok)
        ret["raw_quat"], ret["MANO_theta"], ret["global_pose"] = raw, theta, canon
        return theta, canon

    _said_interaction = set()

    def _interaction_volume(self, frame0, built):
        """The SDF volume forward() / forward_batch() load for a sequence whose first frame is `frame0` -> (volume on the device,
        voxel_scale), or (None, None).  `built` maps id(volume tensor) to its device copy: sequences that hand over one tensor
        share it."""
        opt = self.optimizer
        size, scale0 = (opt.volume_size, opt.voxel_scale) if opt is not None else (151, 0.003)
        if "sdf_volume" in frame0:
            src = frame0["sdf_volume"]
            if id(src) not in built:
                built[id(src)] = (src, src.to(self.device).contiguous())
            scale = frame0.get("voxel_scale")
            return built[id(src)][1], scale0 if scale is None else float(scale)
        from . import mesh_sdf
        scale = float(frame0.get("voxel_scale", scale0))
        vol = mesh_sdf.frame_volume(frame0, size, scale, self.device)
        if vol is not None:
            return vol, scale
        if opt is not None and opt.sdf_volume is not None:  # (as forward: the volume loaded last stays)
            return opt.sdf_volume, opt.voxel_scale
        return None, None

    def _interaction_enqueue(self, inputs, ret_dict_lsts):
        """The hand-object interaction columns of S tracked sequences, enqueued on the device: [(members, keys, seq (len(members), 8))]
        per group of sequences whose volumes share resolution, dtype and voxel_scale (a tracker's sequences usually all do: one
        eval_metrics.hand_interaction_metrics call, two launches).  Nothing is read back here.  [] with the reason printed once
        when the hand model has no skinning tables, a result lacks MANO_theta / global_pose, or a volume cannot be resolved.  The
        object pose of a frame is the one the optimiser used (pred_obj_pose with use_pred_obj_pose, else gt_obj_pose), the shape
        the frame's pred_beta (else the hand model's registered shape)."""
        from . import eval_metrics

        def skip(why):
            if why not in HandTrackModel._said_interaction:
                HandTrackModel._said_interaction.add(why)
                print("[Hand Tracking] hand_interaction_eval: the hand_pen_* / hand_contact_* columns are left out (%s)" % why)
            return []
        hm = self.__dict__.get("_interaction_hand")
        tables = hm.skinning_tables() if hm is not None and hasattr(hm, "skinning_tables") else None
        if tables is None:
            return skip("no hand model" if hm is None else "the hand model has no skinning tables (HandModel.skinning_tables() is None)")
        obj_pose = lambda d: d["pred_obj_pose"] if (self.use_pred_obj_pose and "pred_obj_pose" in d) else d.get("gt_obj_pose")
        for seq, rets in zip(inputs, ret_dict_lsts):
            if len(seq) != len(rets):
                return skip("a sequence and its results differ in length")
            if any("MANO_theta" not in r or "global_pose" not in r for r in rets):
                return skip("the results carry no MANO_theta / global_pose (neither IKNet nor the pose optimiser ran)")
            if any(obj_pose(d) is None for d in seq):
                return skip("a frame carries no object pose")
        built, groups = {}, {}
        for k, seq in enumerate(inputs):
            if not len(seq):
                continue
            vol, scale = self._interaction_volume(seq[0], built)
            if vol is None:
                return skip("a sequence's SDF volume cannot be resolved: no 'sdf_volume' and no mesh in its first frame")
            groups.setdefault((tuple(vol.shape), vol.dtype, scale), []).append((k, vol))
        dev, D = self.device, int(getattr(hm, "num_betas", 0)) if "shape_joints" in tables else 0
        f = lambda x, *shape: torch.as_tensor(x).to(dev).float().reshape(1, *shape)
        out = []
        for (_, _, scale), members in groups.items():
            data = [d for k, _ in members for d in inputs[k]]
            rets = [r for k, _ in members for r in ret_dict_lsts[k]]
            offsets = [0]
            for k, _ in members:
                offsets.append(offsets[-1] + len(inputs[k]))
            poses = [obj_pose(d) for d in data]
            frames = {"MANO_theta": torch.cat([f(r["MANO_theta"], 45) for r in rets]),
                      "global_rotation": torch.cat([f(r["global_pose"]["rotation"], 3, 3) for r in rets]),
                      "global_translation": torch.cat([f(r["global_pose"]["translation"], 3) for r in rets]),
                      "obj_rotation": torch.cat([f(p["rotation"], 3, 3) for p in poses]),
                      "obj_translation": torch.cat([f(p["translation"], 3) for p in poses])}
            if all("pred_kp" in r and tuple(r["pred_kp"].shape[-2:]) == (21, 3) and r["pred_kp"].numel() == 63 for r in rets):
                frames["pred_kp"] = torch.cat([f(r["pred_kp"], 21, 3) for r in rets])
            if D > 0:  # the shape tables: one per distinct shape code (a re-estimated shape: several per sequence)
                codes, index, rest_of = [], {}, []
                for r in rets:
                    b = r.get("pred_beta")
                    b = getattr(hm, "registered_beta", None) if b is None else b
                    key = id(b)
                    if key not in index:
                        index[key] = len(codes)
                        codes.append(torch.zeros((1, D), device=dev) if b is None else f(b, D))
                    rest_of.append(index[key])
                frames["beta"], frames["rest_of"] = torch.cat(codes), torch.tensor(rest_of, dtype=torch.long, device=dev)
            _, seq, keys = eval_metrics.hand_interaction_metrics(frames, offsets, tables, [v for _, v in members], scale,
                                                                 contact_threshold=self.contact_threshold)
            out.append(([k for k, _ in members], keys, seq.float()))
        return out

    def hand_interaction_losses(self, inputs, ret_dict_lsts):
        """[{the eight hand-object interaction keys}] per sequence (empty where they are left out): one call for all sequences,
        one read-back."""
        from . import eval_metrics
        outs = [dict() for _ in inputs]
        parts = self._interaction_enqueue(inputs, ret_dict_lsts) if self.hand_interaction_eval else []
        host = torch.cat([seq.reshape(-1) for _, _, seq in parts]).cpu() if parts else torch.zeros(0)
        at = 0
        for members, keys, seq in parts:
            table = host[at:at + seq.numel()].reshape(len(members), -1).tolist()
            at += seq.numel()
            cols = [eval_metrics.HAND_INTERACTION_KEYS.index(k) for k in keys]
            for j, k in enumerate(members):
                outs[k].update((key, table[j][c]) for key, c in zip(keys, cols))
        return outs

    def compute_loss(self, input, ret_dict_lst, flag_dict, interaction=True):
        """HandTrackNet's loss / metric dictionary averaged over the frames.  With `use_pred_obj_pose` and frames that carry
        `pred_obj_pose`, also the reference's object-pose block (track_network.py:244-251): `obj_pred_tdiff_0`,
        `obj_pred_rdiff_0`, `obj_pred_5deg5cm_0`, `obj_pred_10deg10cm_0` of the supplied object poses against gt_obj_pose
        (eval_metrics.eval_part_full: one launch for the whole sequence, enqueued ahead of the single read-back).
        With cfg['fused_hand_eval'] (`--fused_hand_eval`) it is compute_loss_batch of this one sequence instead.
        With cfg['hand_interaction_eval'] (`--hand_interaction_eval`) the eight eval_metrics.HAND_INTERACTION_KEYS are added (see
        _interaction_enqueue for when they are left out); interaction=False leaves them to the caller (Trainer.test_batch asks
        for all its sequences at once)."""
        if self.fused_hand_eval:
            return self.compute_loss_batch([input], [ret_dict_lst], flag_dict, interaction=interaction)[0]
        return self._compute_loss_frames(input, ret_dict_lst, flag_dict, interaction=interaction)

    def _compute_loss_frames(self, input, ret_dict_lst, flag_dict, interaction=True):
        total = {}
        for data, ret in zip(input, ret_dict_lst):
            loss, _ = self.handnet.compute_loss(data, ret, flag_dict)
            for k, v in loss.items():
                total[k] = total[k] + v if k in total else v  # stays on the device: one host sync per sequence
        obj = None
        if self.use_pred_obj_pose and len(input) and all("pred_obj_pose" in d and "gt_obj_pose" in d for d in input):
            from . import eval_metrics
            err = eval_metrics.eval_part_full(_stack_poses([d["gt_obj_pose"] for d in input], self.device),
                                              _stack_poses([d["pred_obj_pose"] for d in input], self.device), axis=int(self.sym),
                                              up_and_down_sym=_up_and_down_sym(input[0]["gt_obj_pose"]))
            obj = torch.stack([err[k] for k in eval_metrics.METRIC_KEYS])
        inter = self.hand_interaction_eval and interaction and len(input)
        extra = self.hand_interaction_losses([input], [ret_dict_lst])[0] if inter else {}
        out = {k: float(v) / len(input) for k, v in total.items()}
        if obj is not None:
            out.update({"obj_pred_" + k: v for k, v in zip(eval_metrics.METRIC_KEYS, obj.tolist())})
        out.update(extra)
        return out, ret_dict_lst

    _said_eval = set()

    def _fused_eval_unsupported(self, inputs, ret_dict_lsts):
        """Why compute_loss_batch cannot take the two-launch route for these sequences (None: it can)."""
        if getattr(self.handnet, "handframe", None) == "OBB":
            return "the OBB hand frame has no pose terms"
        for seq, rets in zip(inputs, ret_dict_lsts):
            if len(seq) != len(rets):
                return "a sequence and its results differ in length"
            for r in rets:
                if tuple(r["pred_kp"].shape) != (1, 21, 3):
                    return "it needs one hand of 21 keypoints per frame, got pred_kp %s" % (tuple(r["pred_kp"].shape),)
        return None

    def compute_loss_batch(self, inputs, ret_dict_lsts, flag_dict, interaction=True):
        """`compute_loss` for S tracked sequences at once, on the reference's rule (track_network.py:228-307): every frame of every
        sequence is stacked, ONE eval_metrics.hand_sequence_metrics call (two launches on the GPU) gives the per-frame and the
        per-sequence values, the `obj_pred_*` block is enqueued as in compute_loss, and one read-back brings everything to the
        host.  Returns [(loss_dict, ret_dict_lst)] per sequence, the dictionary in the reference's key order with
        `MANO_theta_diff` (needs `MANO_theta` in the results and `mano_pose` in gt_hand_pose) after `hand_canon_t_diff`.
        Unlike compute_loss, the three `init` keys are the sequence's FIRST frame (the reference's rule), not the mean.  With
        flag_dict['save_flag'], ret_dict_lst[0]['frame_errors'] is the (T,3) CPU table of the per-frame kp_error, r_error and
        t_error (hand_pred_kp_diff, hand_pred_r_diff, hand_pred_t_diff), and every frame's 'gt_kp_handframe' is filled.  The palm
        template of a sequence is its first frame's.  Sequences the route does not cover (OBB hand frame, other keypoint counts)
        go through compute_loss's loop; the reason is printed once."""
        from . import eval_metrics
        from .hand_utils import canonicalize
        why = self._fused_eval_unsupported(inputs, ret_dict_lsts)
        if why is not None:
            if why not in HandTrackModel._said_eval:
                HandTrackModel._said_eval.add(why)
                print("[Hand Tracking] fused_hand_eval: the per-frame evaluation runs (%s)" % why)
            return [self._compute_loss_frames(seq, rets, flag_dict, interaction=interaction) for seq, rets in zip(inputs, ret_dict_lsts)]
        dev, save = self.device, bool(flag_dict.get("save_flag"))
        f = lambda x: x.to(dev).float()
        S = len(inputs)
        # sequences that determine the same columns share a call (a tracker's sequences all do: one call)
        sig = lambda seq, rets: (all("global_pose" in r for r in rets), all("rotation" in d.get("gt_hand_pose", {}) for d in seq),
                                 all("MANO_theta" in r for r in rets) and all("mano_pose" in d.get("gt_hand_pose", {}) for d in seq))
        groups = {}
        for k in range(S):
            if len(inputs[k]):
                groups.setdefault(sig(inputs[k], ret_dict_lsts[k]), []).append(k)
        pieces, layout = [], []  # the device tensors of the one read-back; (what, whose, count)
        for (pose_mode, has_gt, has_theta), members in groups.items():
            data = [d for k in members for d in inputs[k]]
            rets = [r for k in members for r in ret_dict_lsts[k]]
            offsets = [0]
            for k in members:
                offsets.append(offsets[-1] + len(inputs[k]))
            F = offsets[-1]
            def cat(ts, *shape):  # (F, *shape) on the device: tensors that share a device travel as one copy
                ts = [torch.as_tensor(t) for t in ts]
                if len({t.device for t in ts}) == 1:
                    return f(torch.cat([t.reshape(1, *shape) for t in ts], dim=0))
                return torch.cat([f(t).reshape(1, *shape) for t in ts], dim=0)
            frames = {"pred_kp": cat([r["pred_kp"] for r in rets], 21, 3),
                      "pred_kp_handframe": cat([r["pred_kp_handframe"] for r in rets], 3, 21),
                      "init_kp_handframe": cat([r["init_kp_handframe"] for r in rets], 3, 21),
                      "gt_hand_kp": cat([d["gt_hand_kp"] for d in data], 21, 3),
                      "canon_rotation": cat([r["canon_pose"]["rotation"] for r in rets], 3, 3),
                      "canon_translation": cat([r["canon_pose"]["translation"] for r in rets], 3),
                      "canon_scale": cat([r["canon_pose"]["scale"] for r in rets]).reshape(F)}
            if pose_mode:
                frames["global_rotation"] = cat([r["global_pose"]["rotation"] for r in rets], 3, 3)
                frames["global_translation"] = cat([r["global_pose"]["translation"] for r in rets], 3)
            if has_gt or pose_mode:
                frames["gt_rotation"] = cat([d["gt_hand_pose"]["rotation"] for d in data], 3, 3)
                frames["gt_translation"] = cat([d["gt_hand_pose"]["translation"] for d in data], 3)
            if has_theta:
                frames["MANO_theta"] = cat([r["MANO_theta"] for r in rets], 45)
                frames["gt_MANO_theta"] = cat([d["gt_hand_pose"]["mano_pose"].reshape(1, -1)[:, 3:] for d in data], 45)
            palm = None if pose_mode else cat([inputs[k][0]["gt_hand_pose"]["palm_template"] for k in members], 6, 3)
            rows, seq, keys = eval_metrics.hand_sequence_metrics(frames, offsets, palm=palm)
            gt_hf = None
            if save:
                gt_hf = canonicalize(frames["gt_hand_kp"].transpose(-1, -2),
                                     {"rotation": frames["canon_rotation"], "translation": frames["canon_translation"][:, :, None],
                                      "scale": frames["canon_scale"]})
            for i, r in enumerate(rets):
                r["gt_kp_handframe"] = gt_hf[i:i + 1] if save else None
            cols = [eval_metrics.HAND_METRIC_KEYS.index(k) for k in keys]
            pieces.append(seq.reshape(-1))
            layout.append(("seq", (members, keys, cols), seq.numel()))
            if save:
                pieces.append(torch.stack([rows[:, 1], rows[:, 7], rows[:, 8]], dim=-1).reshape(-1))
                layout.append(("frames", (members, offsets), 3 * F))
        for k in range(S):
            seq_in = inputs[k]
            if self.use_pred_obj_pose and len(seq_in) and all("pred_obj_pose" in d and "gt_obj_pose" in d for d in seq_in):
                err = eval_metrics.eval_part_full(_stack_poses([d["gt_obj_pose"] for d in seq_in], self.device),
                                                  _stack_poses([d["pred_obj_pose"] for d in seq_in], self.device), axis=int(self.sym),
                                                  up_and_down_sym=_up_and_down_sym(seq_in[0]["gt_obj_pose"]))
                pieces.append(torch.stack([err[key] for key in eval_metrics.METRIC_KEYS]).float())
                layout.append(("obj", k, len(eval_metrics.METRIC_KEYS)))
        # the hand-object interaction columns (cfg['hand_interaction_eval']): enqueued here, read back with everything else
        for members, keys, seq in (self._interaction_enqueue(inputs, ret_dict_lsts) if self.hand_interaction_eval and interaction else ()):
            pieces.append(seq.reshape(-1))
            layout.append(("interaction", (members, keys, [eval_metrics.HAND_INTERACTION_KEYS.index(k) for k in keys]), seq.numel()))
        host = torch.cat(pieces).cpu() if pieces else torch.zeros(0)  # the one read-back
        outs, at = [dict() for _ in range(S)], 0
        for what, info, n in layout:
            part = host[at:at + n]
            at += n
            if what in ("seq", "interaction"):
                members, keys, cols = info
                table = part.reshape(len(members), -1).tolist()
                for j, k in enumerate(members):
                    outs[k].update((key, table[j][c]) for key, c in zip(keys, cols))
            elif what == "frames":
                members, offsets = info
                for j, k in enumerate(members):
                    ret_dict_lsts[k][0]["frame_errors"] = part.reshape(-1, 3)[offsets[j]:offsets[j + 1]].clone()
            else:
                outs[info].update({"obj_pred_" + key: v for key, v in zip(eval_metrics.METRIC_KEYS, part.tolist())})
        return [(outs[k], ret_dict_lsts[k]) for k in range(S)]


class _ObjSequence:
    """One object sequence being tracked: the pose dict carried from frame to frame (`last`), the results (`rets`), the observed
    surface (or None) and the refinement's stats.  `forward` drives one, `forward_batch` one per sequence of its group: per frame
    `begin`, the caller's optimiser call (`optimize`, or one `optimize_batch` for the group), `accept`; `finish` at the end.  The
    volume is the caller's: `forward` reads the optimiser's, a group keeps one per sequence."""

    def __init__(self, model, frames):
        self.model, self.frames = model, frames
        self.last, self.surf = None, None
        self.rets, self.refined = [], []

    def begin(self, data):
        """Completes a frame for the optimiser: frame 0 starts from its jittered pose, frame t from frame t-1's result, which is
        also the pose dict's `prev_*` entries (:353-370)."""
        m = self.model
        if m.fuse_depth or m.render_model:  # one upload serves the front end, the fusion and the rendering's comparison
            for key in ("depth", "seg"):
                if isinstance(data[key], torch.Tensor):
                    data[key] = data[key].to(m.device, non_blocking=True)
        first = self.last is None
        if first:
            jp = data["jittered_obj_pose"]
            jp["translation"] = jp["translation"].float().reshape(1, 3, 1).to(m.device)
            jp["rotation"] = jp["rotation"].float().reshape(1, 3, 3).to(m.device)
            jp["prev_translation"], jp["prev_rotation"] = jp["translation"], jp["rotation"]
            self.last = {"translation": jp["translation"], "rotation": jp["rotation"]}
        else:
            data["jittered_obj_pose"] = self.last
        m._front_end.complete(data, "obj_points")
        if first and m.accumulate_surface:  # the pose the tracking starts from (load_obj, :153-158)
            cloud0 = data["obj_points"].float().to(m.device)
            self.surf = m._new_surface(cloud0).start(cloud0, data["jittered_obj_pose"])

    def accept(self, data, ret, corner_volume, voxel_scale):
        """Takes the frame's tracked (and, with opt.refine_pose, refined) pose; the volume is the one it was tracked against."""
        m = self.model
        if m.refine_pose:
            self.refined.append(ret.pop("refine_stats"))
        if self.surf is not None:
            self.surf.add(data["obj_points"].float().to(m.device), ret, corner_volume, voxel_scale)
        last = self.last
        last["prev_translation"], last["prev_rotation"] = last["translation"], last["rotation"]  # last frame's pose
        last["translation"], last["rotation"] = ret["translation"], ret["rotation"]            # current frame's pose
        self.rets.append(ret)

    def finish(self, volume, corner_volume, voxel_scale, fused_state, flag_dict, shared_meshes=None):
        """What the switches attach to rets[0] at the end of a sequence (one that has frames), read off its final volume."""
        m, rets = self.model, self.rets
        if self.refined:
            rets[0]["obj_refine"] = torch.stack(self.refined)  # (frames, 8): hotrack_amd.sdf.obj_refine's stats, on the device
        if fused_state is not None:
            rets[0]["obj_fused"] = fused_state
        if m.render_model:  # every frame with its tracked pose; one launch per sequence (no batched raycast: DESIGN.md 8m)
            m._attach_render(self.frames, rets, volume, voxel_scale, fused_state is not None, flag_dict)
        if self.surf is not None:
            rets[0]["obj_surface"] = m._surface_entry(self.surf, corner_volume, voxel_scale)
        if m.extract_mesh:
            m._attach_mesh(self.frames, rets, volume, voxel_scale, flag_dict, shared_meshes)


def _require_frame_keys(feature, frames, where):
    """`feature` (a switch's name) reads every frame's depth image: raises for the first of `frames` that lacks a key it needs.
    `where` goes in front of the frame's index ('' or 'sequence k, ')."""
    for t, data in enumerate(frames):
        missing = [key for key in ("depth", "seg", "intrinsics") if key not in data]
        if missing:
            raise KeyError(f"{feature} reads the observed depth frames: the sequence's frames must carry 'depth', 'seg' and "
                           f"'intrinsics' (as the --from_depth frames do); {where}frame {t} ({data['file_name'][0]}) lacks {missing}")


def _sequence_stem(input, save_folder):
    """<save_folder>/<sequence>, the stem of every file saved for a sequence; makes the folder."""
    name = os.path.dirname(input[0]["file_name"][0]) or input[0]["file_name"][0]
    os.makedirs(save_folder, exist_ok=True)
    return os.path.join(save_folder, name.replace("/", "_"))


class ObjTrackModel_Optimization(nn.Module):
    """Per-sequence object-pose tracking by gradient-free particle optimisation against the object's SDF volume
    (counterpart of the reference's ObjTrackModel_Optimization, track_network.py:322-383; BASELINE configs[3], stage 1).

    Frame 0 starts from the jittered pose; frame t starts from frame t-1's result, which also becomes the `prev_*` entries
    of the pose dict (:353-370).  Each frame is one `gf_optimize_obj.optimize` call = 10 iterations x 2048 candidate
    poses evaluated by the fused SDF-lookup kernels with the pose update on the device (hotrack_amd/csrc/sdf.hip): the loop
    never synchronises with the host.  The reference decodes the volume from a DeepSDF latent per sequence
    (`load_obj_for_opt` + `optimizer.load_obj`, :342-346 -- needs the checkpoints); here the sequence hands the volume
    over (`input[0]['sdf_volume']`, `['voxel_scale']`) or hands over the object's triangle mesh (`input[0]['obj_mesh']` =
    {'vertices', 'faces'} or `['obj_mesh_path']`), from which the volume is built once (models/mesh_sdf.py, the reference's
    load_obj_oracle)."""

    # The switches' defaults, for a tracker built without __init__ or with an attribute deleted.  __init__ sets them from cfg['opt']
    # and cfg['save_dir'] and says there what each one does; a *_route has no config key: None (the kernel for GPU tensors),
    # 'kernel' or 'torch'
    extract_mesh, extract_mesh_route = False, None
    fuse_depth, lockstep_fuse, fuse_route = False, False, None
    render_model, render_occl_margin, render_route = False, 0.01, None
    refine_pose, refine_route = False, None
    save_folder = None

    def __init__(self, cfg):
        super().__init__()
        from .optimization_obj import gf_optimize_obj
        self.device = cfg["device"]
        self.dataset_name = cfg["data_cfg"]["dataset_name"]
        self.sdf_code_source = cfg.get("sdf_code_source", "pred")
        self.num_parts = cfg.get("num_parts", 1)
        self.sym = cfg.get("obj_sym", -1)
        self.optimizer = gf_optimize_obj(cfg)
        self._front_end = _FrontEndSlot(cfg)  # frames that carry a depth image instead of obj_points (models/frame_frontend.py)
        # opt.accumulate_surface: keep each sequence's observed surface (models/obs_surface.py); the poses do not depend on it
        self.accumulate_surface = bool((cfg.get("opt") or {}).get("accumulate_surface", False))
        # opt.extract_mesh: at the end of a sequence extract the mesh of its SDF volume (models/mesh_sdf.volume_to_mesh); the poses
        # do not depend on it
        self.extract_mesh = bool((cfg.get("opt") or {}).get("extract_mesh", False))
        self.extract_mesh_route = None
        # opt.fuse_depth: fuse every tracked depth frame into the sequence's own copy of the volume (models/shape_fusion.py,
        # hotrack_amd/csrc/tsdf_fuse.hip) and track the later frames against it.  fuse_every: frames between flushes (the reference
        # refits its shape every tenth frame);  fuse_trunc: the truncation distance in VOXELS (5: wide enough for the trilinear
        # lookup's cell and the tracker's centimetre pose errors, narrow enough not to reach through the 8 cm capsule);
        # fuse_prior_weight: the weight of the handed-over model, in frames (8: a model is trusted like eight observations, so
        # one flush of ten frames already outweighs it where the object was seen)
        opt_cfg = cfg.get("opt") or {}
        self.fuse_depth = bool(opt_cfg.get("fuse_depth", False))
        self.fuse_every = int(opt_cfg.get("fuse_every", 10))
        self.fuse_trunc = float(opt_cfg.get("fuse_trunc", 5.0))
        self.fuse_prior_weight = float(opt_cfg.get("fuse_prior_weight", 8.0))
        self.fuse_route = None
        # opt.lockstep_fuse: allow opt.fuse_depth in forward_batch.  Opt-in, for memory: every sequence of a group then owns a copy
        # of the volume and its weights, and from its first flush on a corner layout (201^3 fp16: 49 MB + 130 MB per sequence)
        self.lockstep_fuse = bool(opt_cfg.get("lockstep_fuse", False))
        self._fuse_frontend = dict(cfg.get("depth_frontend") or {})
        # opt.render_model: at the end of a sequence render its volume (with opt.fuse_depth the fused one) at every tracked pose in
        # one launch and compare the maps with the observed frames in a second (models/volume_render.py,
        # hotrack_amd/csrc/sdf_raycast.hip); the poses do not depend on it.  render_occl_margin (metres) is a choice, like
        # contact_threshold: how far in front of the model a non-object pixel must lie to count as an occluder
        # (hotrack_amd.sdf.OCCL_MARGIN says why 1 cm)
        self.render_model = bool(opt_cfg.get("render_model", False))
        self.render_occl_margin = float(opt_cfg.get("render_occl_margin", 0.01))
        self.render_route = None
        # opt.refine_pose: after every frame's particle search, refine_iters damped Gauss-Newton steps on the volume inside a band of
        # refine_band metres (gf_optimize_obj.refine, hotrack_amd/csrc/sdf_refine.hip): one more launch per frame or group step.  The
        # refined pose is the frame's pose: the next frame starts from it and every later stage reads it.  Off: no new code runs
        self.refine_pose = bool(opt_cfg.get("refine_pose", False))
        self.refine_route = None
        self.surface_seed = 0  # every sequence draws from a generator of its own with this seed: alone or in a group, the same surface
        self.save_folder = cfg.get("save_dir")

    def _new_surface(self, cloud):
        """An ObservedSurface for a sequence whose first cloud is `cloud`: as many slots as that cloud has points (the
        reference's merged cloud is its first cloud), at most the normal kernel's 2048."""
        from hotrack_amd import ext
        from .obs_surface import ObservedSurface
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(self.surface_seed))
        return ObservedSurface(min(cloud.reshape(-1, 3).shape[0], ext.CLOUD_NORMALS_MAX_N), generator=gen)

    @staticmethod
    def _surface_entry(surf, corner_volume, voxel_scale):
        from .obs_surface import surface_fit
        return dict(surf.state(), fit=surface_fit(surf.points, surf.normals, corner_volume, voxel_scale))

    def _attach_mesh(self, input, rets, volume, voxel_scale, flag_dict, shared=None):
        """opt.extract_mesh, at the end of a sequence (the reference: optimizer.sdf2mesh, track_network.py:380-381): the mesh of
        the sequence's SDF volume goes into rets[0]['obj_info'] = {'recon_path', 'recon_mesh': {'vertices', 'faces'}}.  With
        --save and a save directory the mesh is written as <sequence>_recon.ply and 'recon_path' names the file (else None).
        `shared` maps id(volume) to a mesh already extracted: sequences of a group that share a volume share one extraction."""
        from . import mesh_sdf
        hit = None if shared is None else shared.get(id(volume))
        if hit is None:
            verts, faces = mesh_sdf.volume_to_mesh(volume, voxel_scale, 0.0, route=self.extract_mesh_route)
            hit = (volume, {"vertices": verts, "faces": faces})  # (the volume is kept with the mesh: the key's id stays its)
            if shared is not None:
                shared[id(volume)] = hit
        path = None
        if flag_dict.get("save_flag") and self.save_folder:
            path = _sequence_stem(input, self.save_folder) + "_recon.ply"
            mesh_sdf.save_mesh(path, hit[1]["vertices"], hit[1]["faces"])
        rets[0]["obj_info"] = {"recon_path": path, "recon_mesh": hit[1]}

    def _attach_render(self, input, rets, volume, voxel_scale, fused, flag_dict):
        """opt.render_model, at the end of a sequence: `input` holds every frame, `rets` its tracked pose (device references).  All
        frames are rendered in one launch and compared in a second (volume_render.model_frame_fit); a fused volume is marched with
        step_scale 0.8, because a projective TSDF overestimates the distance at grazing angles.
        rets[0]['obj_render'] = {'depth' (F,H,W), 'normal' (F,H,W,3), 'stats' (F,4), 'columns' (3,), 'skipped' ()}; with --save and
        a save directory the last frame's maps are written as <sequence>_model_depth.png / _model_normal.png."""
        from . import volume_render
        fe = self._fuse_frontend
        out = volume_render.model_frame_fit(volume, voxel_scale, list(input), list(rets),
                                            obj_class=tuple(fe.get("obj_class", (1, 255))), flip_yz=bool(fe.get("flip_yz", False)),
                                            step_scale=0.8 if fused else 1.0, occl_margin=self.render_occl_margin,
                                            route=self.render_route)
        rets[0]["obj_render"] = out
        if flag_dict.get("save_flag") and self.save_folder:
            stem = _sequence_stem(input, self.save_folder)
            out["paths"] = (volume_render.save_depth_png(stem + "_model_depth.png", out["depth"][-1]),
                            volume_render.save_normal_png(stem + "_model_normal.png", out["normal"][-1]))

    def _begin_tracking(self, sequences, flag_dict):
        """Before any work: every frame of `sequences` ({where: frames}) must carry what the switches that read the observed depth
        frames need."""
        flag_dict["track_flag"] = True
        assert flag_dict["test_flag"]
        for feature, on in (("opt.render_model", self.render_model), ("opt.fuse_depth", self.fuse_depth)):
            if on:
                for where, frames in sequences.items():
                    _require_frame_keys(feature, frames, where)

    def forward(self, input, flag_dict):
        self._begin_tracking({"": input}, flag_dict)
        opt = self.optimizer
        self._sequence_volume(input[0], {})
        seq = _ObjSequence(self, input)
        fusion = self._new_fusion() if self.fuse_depth else None
        for data in input:
            seq.begin(data)
            ret = opt.optimize(data["obj_points"], data["jittered_obj_pose"], data["category"][0], data["file_name"][0],
                               data.get("projection"))
            if self.refine_pose:
                ret = opt.refine(data["obj_points"], ret, route=self.refine_route)
            seq.accept(data, ret, opt._corners, opt.voxel_scale)
            if fusion is not None:
                fusion.push(data, ret)
                if fusion.due():  # the later frames are tracked against the fused volume (load_volume rebuilds the corner layout)
                    opt.load_volume(fusion.flush(), fusion.voxel_scale)
        if fusion is not None and fusion.pending:
            opt.load_volume(fusion.flush(), fusion.voxel_scale)
        # (after the last flush: the fused volume, else the loaded one)
        seq.finish(opt.sdf_volume, opt._corners, opt.voxel_scale, None if fusion is None else fusion.state(), flag_dict)
        return seq.rets

    def _new_fusion(self):
        """opt.fuse_depth: the VolumeFusion of a sequence whose volume has just been loaded (a clone: the handed-over tensor,
        which a dataset may share between sequences, and a cached mesh volume are never written)."""
        from .shape_fusion import VolumeFusion
        fe = self._fuse_frontend
        scale = float(self.optimizer.voxel_scale)
        return VolumeFusion(self.optimizer.sdf_volume, scale, self.fuse_prior_weight, self.fuse_trunc * scale, self.fuse_every,
                            obj_class=tuple(fe.get("obj_class", (1, 255))), flip_yz=bool(fe.get("flip_yz", False)),
                            route=self.fuse_route, device=self.device)

    def _new_fusion_group(self, corner_volumes, voxel_scale):
        """opt.fuse_depth with opt.lockstep_fuse: the VolumeFusionGroup of a lockstep group whose volumes have just been loaded --
        every sequence gets a clone of its volume, as `_new_fusion` gives a single one (sequences that share a volume stop sharing)."""
        from .shape_fusion import VolumeFusionGroup
        fe = self._fuse_frontend
        scale = float(voxel_scale)
        return VolumeFusionGroup([None if c is None else c.source for c in corner_volumes], scale, self.fuse_prior_weight,
                                 self.fuse_trunc * scale, self.fuse_every, obj_class=tuple(fe.get("obj_class", (1, 255))),
                                 flip_yz=bool(fe.get("flip_yz", False)), route=self.fuse_route, device=self.device)

    def _sequence_volume(self, frame0, built):
        """The volume `forward` would load for a sequence whose first frame is `frame0`, in its lookup layout ->
        (hotrack_amd.sdf.CornerVolume, voxel_scale).  `built` maps id(volume tensor) to what was built from it, so sequences
        that hand over the same tensor (or the same mesh: mesh_sdf caches its volume) share one copy.  Leaves the optimiser
        in the state `forward` leaves it in (volume_size, voxel_scale, sdf_volume), which the next mesh build reads."""
        opt = self.optimizer
        if "sdf_volume" in frame0:
            src, scale = frame0["sdf_volume"], frame0.get("voxel_scale")
        else:
            from . import mesh_sdf
            scale = float(frame0.get("voxel_scale", opt.voxel_scale))
            src = mesh_sdf.frame_volume(frame0, opt.volume_size, scale, self.device)
            if src is None:
                if opt.sdf_volume is None:
                    raise RuntimeError("no SDF volume: decoding it from a DeepSDF latent needs the checkpoints (out of scope); "
                                       "put 'sdf_volume' / 'voxel_scale', or the object's mesh as 'obj_mesh' ({'vertices', 'faces'}) or "
                                       "'obj_mesh_path', into the sequence's first frame")
                return opt._corners, opt.voxel_scale  # (the volume loaded last stays)
        hit = built.get(id(src))
        if hit is None:
            opt.load_volume(src, scale)
            built[id(src)] = (src, opt.sdf_volume, opt._corners)
        else:
            opt.volume_size, opt.sdf_volume, opt._corners = hit[0].shape[0], hit[1], hit[2]
            if scale is not None:
                opt.voxel_scale = float(scale)
        return opt._corners, opt.voxel_scale

    def forward_batch(self, inputs, flag_dict):
        """`forward` for S sequences in lockstep: frame index t of every sequence that still has one is ONE
        `gf_optimize_obj.optimize_batch` call (the same 11 launches over a (particle, sequence) grid), so the device works on S
        sequences' particles while each one's serial tail runs, and the per-frame host work is paid once per step instead of
        once per sequence.  inputs: a list of S sequences, each what `forward` takes; sequences shorter than the longest sit
        out once they have ended.  All volumes must share one resolution, dtype and voxel_scale (one launch reads them all).
        Returns a list of S `ret_dict_lst`, bit-equal to S `forward` calls."""
        if self.fuse_depth and not self.lockstep_fuse:
            raise ValueError("opt.fuse_depth for sequences tracked in lockstep needs opt.lockstep_fuse (--lockstep_fuse) as well: a group's "
                             "sequences share volumes, a fused volume belongs to one sequence, so every sequence of the group then owns "
                             "a copy of the volume, its weights and, from its first flush on, the corner layout; or track with "
                             "--seq_batch 1")
        self._begin_tracking({f"sequence {k}, ": seq for k, seq in enumerate(inputs)}, flag_dict)
        opt, built, vols, scales = self.optimizer, {}, [], []
        for seq in inputs:
            v, s = self._sequence_volume(seq[0], built) if len(seq) else (None, None)
            vols.append(v)
            scales.append(s)
        known = [(k, s) for k, s in enumerate(scales) if s is not None]
        for k, s in known:
            if s != known[0][1]:
                raise ValueError(f"sequences {known[0][0]} and {k} differ in voxel_scale ({known[0][1]}, {s}): a group tracked in "
                                 "lockstep shares one; track them in separate groups")
        scale = known[0][1] if known else None
        S = len(inputs)
        seqs = [_ObjSequence(self, seq) for seq in inputs]
        group = self._new_fusion_group(vols, scale) if self.fuse_depth and known else None
        for t in range(max((len(seq) for seq in inputs), default=0)):
            live = [k for k in range(S) if t < len(inputs[k])]
            for k in live:
                seqs[k].begin(inputs[k][t])
            # (a sequence that has ended keeps its slot, with no cloud and no volume: the launch skips it; an EMPTY sequence
            # has no pose either and borrows a live one's, which comes back unchanged and is dropped)
            clouds = [inputs[k][t]["obj_points"] if t < len(inputs[k]) else None for k in range(S)]
            step_vols = [vols[k] if t < len(inputs[k]) else None for k in range(S)]
            poses = [inputs[k][t]["jittered_obj_pose"] if t < len(inputs[k]) else seqs[k].last for k in range(S)]
            out = opt.optimize_batch(clouds, [p if p is not None else poses[live[0]] for p in poses], step_vols, scale)
            if self.refine_pose:  # one more launch for the group; a sequence that has ended sits it out too
                out = opt.refine_batch(clouds, out, step_vols, scale)
            for k in live:
                seqs[k].accept(inputs[k][t], out[k], vols[k], scale)
            if group is not None:
                # as `forward`: the frame is pushed with the pose just found; a sequence whose pending frames reach fuse_every, or
                # whose last frame this was, is flushed -- all of them in ONE launch -- and tracked against its own fused volume
                # from the next frame on (until its first flush it reads the group's shared corner layout: the same bits)
                for k in live:
                    group.push(k, inputs[k][t], out[k])
                flush = [k for k in live if group.due(k) or t == len(inputs[k]) - 1]
                if flush:
                    from hotrack_amd import sdf as _sdf
                    for k, fused in zip(flush, group.flush(flush)):
                        vols[k] = _sdf.CornerVolume(fused)
                    opt.forget_volume_tables()  # (they hold the corner layouts just replaced)
        meshes = {}
        for k, st in enumerate(seqs):
            if st.rets:  # vols[k].source is the sequence's volume, fused if it was
                st.finish(vols[k].source, vols[k], scale, None if group is None else group.state(k), flag_dict, meshes)
        return [st.rets for st in seqs]

    def compute_loss(self, input, ret_dict_lst, flag_dict):
        """The reference's evaluation of a tracked sequence (track_network.py:385-434) next to this project's three figures,
        every frame at once on the device (eval_metrics; hotrack_amd/csrc/seq_eval.hip) with one read-back per sequence:

          obj_pred_r_diff / obj_pred_axis_diff / obj_pred_t_diff   mean geodesic rotation / object-z-axis (degrees) and
                                                  translation (metres) error against gt_obj_pose;
          tdiff_0, rdiff_0, 5deg5cm_0, 10deg10cm_0                 eval_part_full with axis = int(cfg['obj_sym']) (default -1) and
                                                  up_and_down_sym from gt_obj_pose (default False).  An optional
                                                  input[0]['eval_frame'] = {'rotation' (3,3), 'translation' (3,)} is the
                                                  reference's HO3D / DexYCB change of evaluation frame (:417-425), applied to both
                                                  poses; its per-instance table of such frames is not part of this project;
          raw_obj_chamfer(mm), pred_obj_chamfer(mm)                when input[0] carries 'obj_model_points' ((N,3) samples of the
                                                  ground-truth surface, object frame): chamfer distance to the predicted
                                                  cloud (input[0]['obj_recon_points'], else the same points) un-posed, and under
                                                  the ground-truth / predicted pose of each frame, averaged.  The reference
                                                  samples a mesh file and the decoded reconstruction instead (mesh assets).  A
                                                  cloud of more than 2048 points is cut to 2048 by this project's FPS operator
                                                  (the reference: its Python FPS).  Without model points but with a mesh
                                                  ('obj_mesh' / 'obj_mesh_path') 2048 points are sampled from it
                                                  (mesh_sdf.sample_surface, seed 0); with neither, and opt.extract_mesh on, from
                                                  the mesh extracted from the sequence's volume
                                                  (ret_dict_lst[0]['obj_info']['recon_mesh']); else the two keys are absent
                                                  and the log says so once;
          model_depth_residual(mm), model_silhouette_iou, model_occluded_ratio   with opt.render_model: the sequence's volume
                                                  rendered at the tracked poses against the observed depth frames, means over
                                                  frames (volume_render.fit_columns); they need no ground truth;
          refine_cost_drop, refine_accepted_steps  with opt.refine_pose: the mean over frames of 1 - final / initial cost of the
                                                  Gauss-Newton refinement (its own weighted mean squared distance inside the
                                                  band) and of the steps it accepted (ret_dict_lst[0]['obj_refine'], (frames, 8))."""
        from . import eval_metrics
        r_err = t_err = a_err = 0.0
        gRs, gts, Rs, ts = [], [], [], []
        for data, ret in zip(input, ret_dict_lst):
            gR = data["gt_obj_pose"]["rotation"].float().reshape(3, 3).to(self.device)
            gt = data["gt_obj_pose"]["translation"].float().reshape(3).to(self.device)
            R, t = ret["rotation"].reshape(3, 3), ret["translation"].reshape(3)
            cos = ((R.t() @ gR).diagonal().sum() - 1) / 2
            r_err = r_err + torch.rad2deg(torch.arccos(cos.clamp(-1, 1)))
            a_err = a_err + torch.rad2deg(torch.arccos((R[:, 2] * gR[:, 2]).sum().clamp(-1, 1)))  # object z axis (revolution axis)
            t_err = t_err + (t - gt).norm()
            gRs.append(gR)
            gts.append(gt)
            Rs.append(R.float())
            ts.append(t.float())
        n = max(len(input), 1)
        if not len(input):
            return {"obj_pred_r_diff": 0.0, "obj_pred_axis_diff": 0.0, "obj_pred_t_diff": 0.0}, ret_dict_lst
        gt_pose = {"rotation": torch.stack(gRs), "translation": torch.stack(gts)}
        pred_pose = {"rotation": torch.stack(Rs), "translation": torch.stack(ts)}
        ev_gt, ev_pred = gt_pose, pred_pose
        if "eval_frame" in input[0]:
            ev_gt, ev_pred = eval_metrics.to_eval_frame(gt_pose, input[0]["eval_frame"]), eval_metrics.to_eval_frame(pred_pose, input[0]["eval_frame"])
        err = eval_metrics.eval_part_full(ev_gt, ev_pred, axis=int(self.sym), up_and_down_sym=_up_and_down_sym(input[0]["gt_obj_pose"]))
        keys = ["obj_pred_r_diff", "obj_pred_axis_diff", "obj_pred_t_diff", *eval_metrics.METRIC_KEYS]
        vals = [r_err, a_err, t_err, *[err[k] for k in eval_metrics.METRIC_KEYS]]
        model_points = input[0].get("obj_model_points")
        if model_points is None:  # the reference's trimesh.sample.sample_surface(mesh, 2048) (:398)
            from . import mesh_sdf
            mesh = mesh_sdf.frame_mesh(input[0], self.device)
            if mesh is not None:
                model_points = mesh_sdf.sample_surface(mesh[1], mesh[2], 2048, seed=0)
            else:  # opt.extract_mesh: the mesh extracted from the sequence's own volume stands in
                recon = (ret_dict_lst[0].get("obj_info") or {}).get("recon_mesh")
                if recon is not None and recon["faces"].shape[0] > 0:
                    model_points = mesh_sdf.sample_surface(recon["vertices"], recon["faces"], 2048, seed=0)
        if model_points is not None:
            gt_cloud = self._eval_cloud(model_points)
            pred_cloud = self._eval_cloud(input[0]["obj_recon_points"]) if "obj_recon_points" in input[0] else gt_cloud
            eye, zero = torch.eye(3, device=self.device).reshape(1, 3, 3), torch.zeros((1, 3), device=self.device)
            raw = eval_metrics.posed_chamfer(gt_cloud, pred_cloud, eye, zero, eye, zero)[0] * 1000
            posed = eval_metrics.posed_chamfer(gt_cloud, pred_cloud, gt_pose["rotation"], gt_pose["translation"], pred_pose["rotation"],
                                               pred_pose["translation"]).mean() * 1000
            keys += ["raw_obj_chamfer(mm)", "pred_obj_chamfer(mm)"]
            vals += [raw, posed]
        elif not ObjTrackModel_Optimization._said_no_points:
            ObjTrackModel_Optimization._said_no_points = True
            print("[Object Tracking] no 'obj_model_points' and no mesh in the sequence's first frame: raw_obj_chamfer(mm) / pred_obj_chamfer(mm) are not reported")
        surface = ret_dict_lst[0].get("obj_surface")
        if surface is not None:  # opt.accumulate_surface: how well the model fits what was seen (obs_surface.surface_fit)
            keys += ["obs_surface_residual(mm)", "obs_surface_normal_agree"]
            vals += [surface["fit"][0], surface["fit"][1]]
        rendered = ret_dict_lst[0].get("obj_render")
        if rendered is not None:  # opt.render_model: the rendered model against the observed frames (volume_render.fit_columns)
            from .volume_render import COLUMNS
            keys += list(COLUMNS)
            vals += list(rendered["columns"].unbind())
        refine = ret_dict_lst[0].get("obj_refine")
        if refine is not None:  # opt.refine_pose: what the Gauss-Newton steps did to their own cost, means over frames
            c0, c1 = refine[:, 0], refine[:, 1]
            keys += ["refine_cost_drop", "refine_accepted_steps"]
            vals += [torch.where(c0 > 0, 1 - c1 / c0.clamp_min(1e-30), torch.zeros_like(c0)).mean(), refine[:, 4].mean()]
        host = torch.stack([torch.as_tensor(v, dtype=torch.float32, device=self.device).reshape(()) for v in vals]).tolist()  # the one read-back
        out = dict(zip(keys, host))
        for k in keys[:3]:
            out[k] = out[k] / n
        if surface is not None and flag_dict.get("save_flag") and self.save_folder:
            self._save_surface(input, ret_dict_lst, surface)
        return out, ret_dict_lst

    def _save_surface(self, input, ret_dict_lst, surface):
        """--save with opt.accumulate_surface: the sequence's pickle (named as the reference names it, track_network.py:446-451)
        with the tracked poses and the observed surface."""
        import pickle
        cpu = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else v
        with open(_sequence_stem(input, self.save_folder) + ".pkl", "wb") as f:
            pickle.dump({"CAD_ID": input[0]["category"][0],
                         "pred_obj_poses": [{k: cpu(r[k]) for k in ("rotation", "translation")} for r in ret_dict_lst],
                         "obj_surface": {k: cpu(v) for k, v in surface.items()}}, f)

    _said_no_points = False

    def _eval_cloud(self, points):
        """(N,3) fp32 cloud on the device, cut to 2048 points by farthest point sampling when larger (:400-402)."""
        pts = torch.as_tensor(points).float().reshape(-1, 3).to(self.device).contiguous()
        if pts.shape[0] > 2048:
            from hotrack_amd import pointnet2_utils
            idx = pointnet2_utils.furthest_point_sample(pts[None], 2048)
            pts = pts[idx[0].long()].contiguous()
        return pts


def _load_mesh_volume(optimizer, frame0, device) -> bool:
    """The reference's load_obj_oracle (optimization_obj.py:163-182): when the first frame carries the object's mesh
    ('obj_mesh' or 'obj_mesh_path'), build its SDF volume at the optimiser's own volume_size and the frame's (else the
    optimiser's) voxel_scale -- once per mesh, cached -- and load it.  False: the frame carries no mesh."""
    from . import mesh_sdf
    voxel_scale = float(frame0.get("voxel_scale", optimizer.voxel_scale))
    vol = mesh_sdf.frame_volume(frame0, optimizer.volume_size, voxel_scale, device)
    if vol is None:
        return False
    optimizer.load_volume(vol, voxel_scale)
    return True


def _stack_poses(poses, device):
    """[{'rotation', 'translation'} per frame] -> {'rotation' (T,3,3), 'translation' (T,3)} fp32 on `device`."""
    return {"rotation": torch.stack([p["rotation"].float().reshape(3, 3).to(device) for p in poses]),
            "translation": torch.stack([p["translation"].float().reshape(3).to(device) for p in poses])}


def _up_and_down_sym(gt_obj_pose) -> bool:
    v = gt_obj_pose.get("up_and_down_sym", False)
    if torch.is_tensor(v):
        return bool(v.reshape(-1)[0]) if v.numel() else False
    if isinstance(v, (list, tuple)):
        return bool(v[0]) if len(v) else False
    return bool(v)
