"""IKNet: tracked hand keypoints -> MANO pose code + global pose (counterpart of the reference's IKNet,
hand_network.py:246-335, with the quaternion helpers of hand_utils.py:13-28 over pose_utils/rotations.py:135-152).

Same parameters as the reference (`linear.0..6`, `bn.0..5`: 126 -> 6 x (1024, BatchNorm, ReLU) -> 60), so its checkpoints
load; their `mano_layer_right.*` buffers are dropped (the hand model is passed in, never registered, never saved).

Two routes, picked per call:
  * kernel -- CUDA input, eval mode, no autograd, <= 16 rows: the palm fit (device Kabsch) and one launch per layer of
    hotrack_amd/csrc/iknet.hip on BatchNorm-folded copies of the weights (folded once per weight version, dropped by train(),
    load_state_dict() and .to()); no host sync, so the step captures into a HIP graph.
  * torch  -- everything else (CPU, training, larger batches): the reference's composition.
`use_kernel = False` forces the torch route (A/B tests).

Deviation: where rounding makes 1 - w^2 negative in the quaternion -> axis-angle conversion, the reference's sqrt yields NaN;
both routes return the limit sin = 0 instead (axis = xyz, angle = 2 acos(clamp(w)))."""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .hand_utils import canonicalize, handkp2palmkp, ransac_rt
from .rotations import matrix_to_unit_quaternion

PARENT = [0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]  # hand_network.py:290
SCALE = 0.2          # hand_network.py:278
EPS_Q = 1e-8         # pose_utils/rotations.py normalize
EPS_AA = 1e-7        # hand_utils.py:9
_CONST = {}


def _const(kind, device):
    """Device-resident constants, created once per device (no host-to-device copy per call: capturable)."""
    key = (kind, str(device))
    if key not in _CONST:
        _CONST[key] = (torch.tensor(PARENT, dtype=torch.long, device=device) if kind == "parent"
                       else SCALE * torch.ones(1, device=device))
    return _CONST[key]


def quat2axisang(quat: torch.Tensor) -> torch.Tensor:
    """(B, 4J) quaternions [w, x, y, z] per joint -> (B, 3J) axis * angle (reference mano_quat2axisang), no sign flip for
    w < 0; sin = sqrt(max(1 - w^2, 0)) (the reference: NaN where rounding makes 1 - w^2 negative)."""
    B = quat.shape[0]
    q = quat.reshape(B, -1, 4)
    q = q / (q.norm(dim=-1, keepdim=True) + EPS_Q)
    cosa = q[..., 0]
    sina = torch.sqrt(torch.clamp(1 - cosa ** 2, min=0)).unsqueeze(-1)
    axis = q[..., 1:] / torch.max(sina, (sina < 1e-8).to(sina.dtype))
    theta = 2 * torch.acos(torch.clamp(cosa, min=-1, max=1))
    return (axis * theta.unsqueeze(-1)).reshape(B, -1)


def axisang2quat(axisang: torch.Tensor) -> torch.Tensor:
    """(B, 3J) axis-angle -> (B, 4J) unit quaternions [w, x, y, z] (reference mano_axisang2quat: axis = aa / (|aa| + 1e-7),
    [cos, axis sin] of the half angle, normalised)."""
    B = axisang.shape[0]
    a = axisang.reshape(B, -1, 3)
    theta = a.norm(dim=-1, keepdim=True)
    axis = a / (theta + EPS_AA)
    half = theta / 2.0
    q = torch.cat([torch.cos(half), axis * torch.sin(half)], dim=-1)
    q = q / (q.norm(dim=-1, keepdim=True) + EPS_Q)
    return q.reshape(B, -1)


def gt_quat(mano_pose: torch.Tensor) -> torch.Tensor:
    """Training target: the 15 joint quaternions of a pose code (B, 45), or of (B, 48) with the global block dropped."""
    q = axisang2quat(mano_pose)
    return q[:, 4:] if mano_pose.shape[1] == 48 else q


def L2_loss(x, y):
    return (x - y).norm(dim=1).mean()


def iknet_checkpoint(cfg):
    """Newest IKNet checkpoint under <data root>/exps/<IKNet_dir>/ckpt, or None."""
    d = cfg.get("IKNet_dir")
    if not d:
        return None
    ckpt = os.path.join(cfg.get("root_dir", os.environ.get("HOTRACK_DATA_ROOT", "data")), "exps", d, "ckpt")
    if not os.path.isdir(ckpt):
        return None
    names = sorted(f for f in os.listdir(ckpt) if f.endswith(".pt"))
    return os.path.join(ckpt, names[-1]) if names else None


def resolve_use_iknet(cfg) -> bool:
    """track: hand_IKNet runs IKNet when a checkpoint exists under IKNet_dir and a hand model is given; the decision is made
    once and kept in cfg['use_iknet'] (so the data loader and the Trainer agree).  Nothing is recorded or logged otherwise."""
    if "use_iknet" in cfg:
        return bool(cfg["use_iknet"])
    if cfg.get("track") != "hand_IKNet" or cfg.get("hand_model") is None:
        return False
    name = iknet_checkpoint(cfg)
    if name is None:
        return False
    cfg["use_iknet"] = True
    print(f"[IKNet] using IKNet from {name}")
    return True


class IKNet(nn.Module):
    LAYERS, WIDTH, IN_DIM, OUT_DIM = 6, 1024, 126, 60

    def __init__(self, cfg, hand_model=None):
        super().__init__()
        self.device = cfg["device"]
        self.linear = nn.ModuleList()
        self.bn = nn.ModuleList()
        last = self.IN_DIM
        for _ in range(self.LAYERS):
            self.linear.append(nn.Linear(last, self.WIDTH))
            self.bn.append(nn.BatchNorm1d(self.WIDTH))
            last = self.WIDTH
        self.linear.append(nn.Linear(self.WIDTH, self.OUT_DIM))
        self.layer_num = self.LAYERS
        self.iknetframe = cfg.get("network", {}).get("iknetframe", "kp")
        if self.iknetframe not in ("kp", "camera"):
            raise NotImplementedError(f"iknetframe {self.iknetframe!r}")
        self.__dict__["hand_model"] = hand_model  # not a submodule: never in the state_dict
        self.use_kernel = True
        self._folded = None

    # ---- folded weights of the kernel route ---------------------------------------------------------------------------
    def train(self, mode: bool = True):
        self._folded = None
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._folded = None
        return super()._apply(fn, *a, **k)

    @staticmethod
    def drop_hand_model_keys(state_dict, prefix=""):
        """A reference checkpoint carries its MANO layer's buffers (`mano_layer_right.*`): dropped, and said so."""
        extra = [k for k in state_dict if k.startswith(prefix + "mano_layer_right.")]
        if extra:
            print(f"[IKNet] ignored {len(extra)} {prefix}mano_layer_right.* entries of the checkpoint (the hand model is passed in)")
            state_dict = type(state_dict)((k, v) for k, v in state_dict.items() if k not in set(extra))
        return state_dict

    def load_state_dict(self, state_dict, *a, **k):
        self._folded = None
        return super().load_state_dict(self.drop_hand_model_keys(state_dict), *a, **k)

    def _weights_key(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def folded_weights(self):
        """(w1 (1024,128), b1, wh (5,1024,1024), bh (5,1024), wo (60,1024), bo): eval-mode BatchNorm folded into the Linear
        layers in float64, stored as float32; rebuilt when any parameter or buffer changed."""
        key = self._weights_key()
        if self._folded is not None and self._folded[0] == key:
            return self._folded[1]
        with torch.no_grad():
            W, B = [], []
            for lin, bn in zip(self.linear[:self.LAYERS], self.bn):
                s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
                W.append(lin.weight.double() * s[:, None])
                B.append((lin.bias.double() - bn.running_mean.double()) * s + bn.bias.double())
            dev = W[0].device
            w1 = torch.zeros((self.WIDTH, 128), dtype=torch.float32, device=dev)
            w1[:, :self.IN_DIM] = W[0]
            out = (w1, B[0].float().contiguous(), torch.stack(W[1:]).float().contiguous(), torch.stack(B[1:]).float().contiguous(),
                   self.linear[-1].weight.detach().float().contiguous(), self.linear[-1].bias.detach().float().contiguous())
        self._folded = (key, out)
        return out

    def kernel_route(self, kp: torch.Tensor) -> bool:
        return (self.use_kernel and kp.is_cuda and not self.training and 1 <= kp.shape[0] <= 16
                and not (torch.is_grad_enabled() and self.linear[0].weight.requires_grad))

    # ---- forward -------------------------------------------------------------------------------------------------------
    def solve(self, init_kp: torch.Tensor, palm_template: torch.Tensor):
        """init_kp (B,21,3) camera frame, palm_template (1|B,6,3) -> raw_quat (B,60), MANO_theta (B,45),
        canon_pose {rotation (B,3,3), translation (B,3,1), scale (1,)}, init_kp_handframe (B,3,21)."""
        R, t, _, _, _ = ransac_rt(palm_template, handkp2palmkp(init_kp))  # y ~= R x + t
        canon = {"scale": _const("scale", init_kp.device), "rotation": R, "translation": t}
        if self.kernel_route(init_kp):
            from hotrack_amd import ext
            raw, theta, kp_hf = ext.iknet_forward(init_kp.float().contiguous(), R.contiguous(), t.contiguous(), *self.folded_weights(),
                                                  camera=self.iknetframe == "camera")
            return raw, theta, canon, kp_hf
        kp_hf = self.to_network_frame(init_kp, canon)
        B = init_kp.shape[0]
        bone = kp_hf - kp_hf.index_select(-1, _const("parent", kp_hf.device))
        x = torch.cat([kp_hf.reshape(B, -1), bone.reshape(B, -1)], -1)  # coordinate-major: x0..x20, y0..y20, z0..z20
        for i in range(self.layer_num):
            x = F.relu(self.bn[i](self.linear[i](x)))
        raw = self.linear[self.layer_num](x)
        return raw, quat2axisang(raw), canon, kp_hf

    def to_network_frame(self, kp, canon):
        kp = kp.transpose(-1, -2)
        return canonicalize(kp, canon) if self.iknetframe == "kp" else kp * 5

    def pose_keypoints(self, raw_quat, canon, beta=None):
        """Keypoints of the hand model driven by IKNet's outputs (hand_network.py:313-318): global rotation quat(R), the 15
        joint quaternions, translation t, shape beta (zeros when None)."""
        hm = self.hand_model.to(raw_quat.device)
        B = raw_quat.shape[0]
        coeffs = quat2axisang(torch.cat([matrix_to_unit_quaternion(canon["rotation"]), raw_quat], dim=1))
        nb = int(getattr(hm, "num_betas", 10))
        betas = None
        if nb > 0:
            betas = (torch.zeros((B, nb), device=raw_quat.device) if beta is None else
                     torch.as_tensor(beta).to(raw_quat.device).float().reshape(B, nb))
        _, kp = hm.forward(th_pose_coeffs=coeffs, th_trans=canon["translation"].reshape(B, 3), th_betas=betas)
        return kp

    def forward(self, input, flag_dict):
        ret = {}
        track = flag_dict["track_flag"]
        if not track:
            palm = input["gt_hand_pose"]["palm_template"].to(self.device).float()
            init_kp = input["jittered_hand_kp"].to(self.device).float()
            beta = input["gt_hand_pose"].get("mano_beta")
        else:  # tracking reads no ground truth (the reference reads gt mano_pose unconditionally, :310)
            palm = input["pred_palm_template"]
            init_kp = input["baseline_pred_kp"].to(self.device).float()
            beta = input.get("pred_beta")
        raw, theta, canon, kp_hf = self.solve(init_kp, palm)
        ret["init_kp_handframe"] = kp_hf
        ret["init_kp"] = init_kp
        if not track:
            ret["gt_kp_handframe"] = self.to_network_frame(input["gt_hand_kp"].to(self.device).float(), canon)
            ret["gt_quat"] = gt_quat(input["gt_hand_pose"]["mano_pose"].float().to(self.device))
        ret["raw_quat"] = raw
        if track and not flag_dict.get("opt_flag", False) and self.hand_model is not None:
            ret["pred_kp"] = self.pose_keypoints(raw, canon, beta)
        ret["MANO_theta"] = theta
        ret["global_pose"] = canon
        return ret

    def compute_loss(self, data, ret_dict, flag_dict):
        gt_kp = data["gt_hand_kp"].to(self.device).float().transpose(-1, -2)
        init_kp = ret_dict["init_kp"].transpose(-1, -2)
        loss = {"quat_loss": (ret_dict["raw_quat"] - ret_dict["gt_quat"]).abs().mean(), "init_gt_kp_diff": L2_loss(init_kp, gt_kp)}
        return loss, ret_dict
