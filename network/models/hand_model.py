"""The hand model behind the hand-pose particle optimiser, as an interface.

The reference evaluates 5120 candidate hands per iteration through a MANO layer (third_party/mano/our_mano.py, called at
optimization_hand.py:216-229, :386-387) -- licensed assets this repository cannot ship.  The optimiser only needs
`vertices, keypoints = f(pose, translation)`, a PCA basis for the pose coefficients and the fingertip contact zones, so that
is the interface (`HandModel`); `SyntheticLBSHand` is a deterministic linear-blend-skinning hand with MANO's sizes (778
vertices, 21 keypoints, 45 pose dimensions, MANO keypoint order) for tests, golden vectors and the synthetic sequences.  A
MANO layer with the reference's call signature plugs in unchanged."""
from __future__ import annotations

import math

import torch
import torch.nn as nn


def rodrigues(aa: torch.Tensor) -> torch.Tensor:
    """(…,3) axis-angle -> (…,3,3)."""
    theta = aa.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    k = aa / theta
    kx, ky, kz = k.unbind(-1)
    z = torch.zeros_like(kx)
    K = torch.stack((z, -kz, ky, kz, z, -kx, -ky, kx, z), dim=-1).view(aa.shape[:-1] + (3, 3))
    s, c = torch.sin(theta)[..., None], torch.cos(theta)[..., None]
    eye = torch.eye(3, dtype=aa.dtype, device=aa.device).expand(aa.shape[:-1] + (3, 3))
    return eye + s * K + (1 - c) * (K @ K)


class HandModel(nn.Module):
    """vertices (P, V, 3), keypoints (P, 21, 3) = forward(th_pose_coeffs (P, 3 + num_pose), th_trans (P, 3)).
    Call signature of the reference's OurManoLayer.forward (keyword arguments th_pose_coeffs / th_trans / th_betas /
    use_registed_beta), `pca_comps2pose(ncomps, coeffs)` (our_mano.py:208-209), `register_beta` (:211-216), and
    `contact_zones` = {1..5: vertex indices of the index / middle / ring / pinky / thumb tip regions} (the obman contact zones
    the reference loads at optimization_hand.py:160-168)."""

    num_verts: int
    num_pose: int
    contact_zones: dict
    num_betas: int = 0  # dimensions of the shape code `th_betas` (MANO: 10); 0 = the model has no shape space

    # A shape basis is accepted when it reproduces forward() to this many metres at shape codes as large as the shape search
    # reaches (initial search size 5 x a few standard deviations of the pre-sampled particles).
    BASIS_TOL = 1e-6
    BASIS_CHECK_RANGE = 20.0

    def pca_comps2pose(self, ncomps: int, pca: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def register_beta(self, th_betas=None):
        return None

    def shape_keypoint_basis(self, pose_coeffs: torch.Tensor):
        """Keypoints at the pose `pose_coeffs` (1, 3 + num_pose) as an affine function of the shape code,
        kp(beta) = K0 + sum_d beta_d K[d]  ->  (K0 (21,3), K (num_betas,21,3)) float32 on the model's device, or None when the
        model has no shape space or is not affine in beta there (the check: forward() at a few random beta in
        [-BASIS_CHECK_RANGE, BASIS_CHECK_RANGE]^num_betas, tolerance BASIS_TOL).  A linear-blend-skinned hand with linear shape
        blend directions (MANO, SyntheticLBSHand) is affine at a fixed pose: the rest joints and vertices are linear in beta
        and the rotations do not depend on it.  Built and checked in float64, once per model and pose."""
        D = int(self.num_betas)
        if D <= 0:
            return None
        pose = pose_coeffs.detach().reshape(1, -1).to(torch.float64).cpu()
        cache = self.__dict__.setdefault("_shape_basis_cache", {})
        key = tuple(pose.flatten().tolist())
        if key not in cache:
            g = torch.Generator().manual_seed(1234)
            betas = torch.cat([torch.zeros(1, D, dtype=torch.float64), torch.eye(D, dtype=torch.float64),
                               (torch.rand(4, D, generator=g, dtype=torch.float64) * 2 - 1) * self.BASIS_CHECK_RANGE])
            dev = next(iter(self.buffers()), pose).device
            with torch.no_grad():
                try:  # float64 where the model computes in the pose's dtype (SyntheticLBSHand), else its own precision
                    _, kp = self.forward(th_pose_coeffs=pose.to(dev).expand(betas.shape[0], -1), th_betas=betas.to(dev))
                except RuntimeError:
                    _, kp = self.forward(th_pose_coeffs=pose.float().to(dev).expand(betas.shape[0], -1), th_betas=betas.float().to(dev))
            kp = kp.cpu().double()
            K0, K = kp[0], kp[1:D + 1] - kp[0]
            pred = K0 + torch.einsum("rd,dkc->rkc", betas[D + 1:], K)
            affine = bool((pred - kp[D + 1:]).abs().max() <= self.BASIS_TOL)
            cache[key] = (K0.float().contiguous(), K.float().contiguous()) if affine else None
        basis = cache[key]
        if basis is None:
            return None
        dev = next(iter(self.buffers()), pose_coeffs).device
        return basis[0].to(dev), basis[1].to(dev)

    # Skinning tables are accepted when lbs_forward_from_tables reproduces forward() to this many metres (float64, a handful of
    # seeded random poses: joint angles up to +-TABLES_CHECK_ANGLE rad, random global rotation, translation and shape code).
    TABLES_TOL = 1e-6
    TABLES_CHECK_ANGLE = 1.5

    def _lbs_tables(self):
        """The model's own claim to be a plain linear-blend-skinning hand: a dict with the entries skinning_tables() documents
        (tensors on any device), or None.  skinning_tables() checks the claim against forward() before it hands it out."""
        return None

    def skinning_tables(self):
        """The model as plain linear-blend-skinning tables (CPU tensors), or None when it is not such a model:
          parents (J,) int64, topologically ordered, joint 0 the root;  pose_block (J,) int64: which 3-vector of the num_pose
          pose dimensions rotates the joint (-1: no rotation of its own; the root takes the global rotation);
          rest_joints (J,3), rest_verts (V,3), skin_idx (V,K) int64, skin_w (V,K), K <= 4;
          shape_joints (D,J,3), shape_verts (D,V,3) when num_betas = D > 0 (else absent);
          comps (num_pose, num_pose): the rows pca_comps2pose uses;
          tips (T,) int64 and finger_offsets (6,) int64: the concatenated contact-zone vertex list of fingers 1..5 in the order
          gf_optimize_hand_pose.set_hand_model builds it (finger i = tips[finger_offsets[i]:finger_offsets[i + 1]]).
        Keypoints are the joint positions.  The tables are accepted only if lbs_forward_from_tables reproduces forward() in
        float64 to TABLES_TOL at seeded random poses (and shape codes); a model with a pose-dependent corrective term (a MANO
        layer with pose blend shapes) fails that check and returns None.  Built and checked once per model."""
        if "_skinning_tables_cache" not in self.__dict__:
            self.__dict__["_skinning_tables_cache"] = self._checked_tables()
        return self.__dict__["_skinning_tables_cache"]

    def _checked_tables(self):
        t = self._lbs_tables()
        if t is None:
            return None
        t = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in t.items()}
        J, K, D = t["parents"].numel(), t["skin_idx"].shape[1], int(self.num_betas)
        if J > 21 or K > 4 or (D > 0) != ("shape_joints" in t) or any(int(t["parents"][j]) >= j for j in range(1, J)):
            return None
        zones = self.contact_zones
        tips, offs = [], [0]
        for i in range(5):
            tips.extend(int(v) for v in zones[i + 1])
            offs.append(len(tips))
        t["tips"], t["finger_offsets"] = torch.tensor(tips, dtype=torch.long), torch.tensor(offs, dtype=torch.long)
        g = torch.Generator().manual_seed(4321)
        n, f64 = 6, torch.float64
        pose = torch.cat([(torch.rand(n, 3, generator=g, dtype=f64) * 2 - 1) * 2.0,
                          (torch.rand(n, self.num_pose, generator=g, dtype=f64) * 2 - 1) * self.TABLES_CHECK_ANGLE], dim=1)
        trans = torch.rand(n, 3, generator=g, dtype=f64) - 0.5
        beta = torch.randn(n, D, generator=g, dtype=f64) * 2 if D > 0 else None
        dev = next(iter(self.buffers()), pose).device
        with torch.no_grad():
            want = None
            for dt in (f64, torch.float32):  # float64 where the model computes in the pose's dtype, else its own precision
                try:
                    want = self.forward(th_pose_coeffs=pose.to(dev, dt), th_trans=trans.to(dev, dt),
                                        th_betas=None if beta is None else beta.to(dev, dt))
                    break
                except RuntimeError:
                    continue
            if want is None:
                return None
            got = lbs_forward_from_tables(t, pose, trans, beta)
        ok = all(tuple(a.shape) == tuple(b.shape) and bool((a.cpu().double() - b).abs().max() <= self.TABLES_TOL)
                 for a, b in zip(want, got))
        return t if ok else None


def lbs_forward_from_tables(tables, pose, trans, beta=None):
    """vertices (P,V,3), keypoints (P,J,3) of HandModel.skinning_tables() at pose (P, 3 + num_pose) = [global axis-angle | joint
    angles], trans (P,3) and, for a model with a shape space, beta (P|1, D) -- in pose's dtype, on pose's device:
        rest = rest_* + beta @ shape_*;  R_0 = rodrigues(pose[:, :3]), t_0 = rest_joints[0];
        t_j = t_parent + R_parent (rest_j - rest_parent),  R_j = R_parent rodrigues(pose block pose_block[j]) (or R_parent);
        v = sum_k w_k (R_k (rest_v - rest_k) + t_k) + trans;  keypoints = t_j + trans."""
    dt, dev, P = pose.dtype, pose.device, pose.shape[0]
    T = lambda k: tables[k].to(dev)
    parents, block = [int(v) for v in tables["parents"]], [int(v) for v in tables["pose_block"]]
    rest, verts = T("rest_joints").to(dt)[None], T("rest_verts").to(dt)[None]
    if beta is not None and "shape_joints" in tables:
        b = beta.to(dev, dt).reshape(-1, tables["shape_joints"].shape[0])
        rest = rest + torch.einsum("pd,djc->pjc", b, T("shape_joints").to(dt))
        verts = verts + torch.einsum("pd,dvc->pvc", b, T("shape_verts").to(dt))
    Rl = rodrigues(pose[:, 3:].reshape(P, -1, 3))
    R_w, t_w = [rodrigues(pose[:, :3])], [rest[:, 0].expand(P, 3)]
    for j in range(1, len(parents)):
        pa = parents[j]
        t_w.append(t_w[pa] + (R_w[pa] @ (rest[:, j] - rest[:, pa])[..., None]).squeeze(-1))
        R_w.append(R_w[pa] @ Rl[:, block[j]] if block[j] >= 0 else R_w[pa])
    R_w, t_w = torch.stack(R_w, dim=1), torch.stack(t_w, dim=1)
    idx, w = T("skin_idx"), T("skin_w").to(dt)
    rel = verts[:, :, None, :] - rest[:, idx]                                   # (P|1, V, K, 3)
    vk = (R_w[:, idx] @ rel[..., None]).squeeze(-1) + t_w[:, idx]
    out = (vk * w[None, :, :, None]).sum(dim=2)
    return out + trans[:, None, :], t_w + trans[:, None, :]


class SyntheticLBSHand(HandModel):
    FINGERS = ((1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12), (13, 14, 15, 16), (17, 18, 19, 20))  # thumb, index, middle, ring, pinky

    def __init__(self, num_verts: int = 778, seed: int = 0, num_betas: int = 0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.num_verts, self.num_pose, self.num_betas = num_verts, 45, int(num_betas)
        # ---- rest skeleton (metres), wrist at the origin, fingers along +y, palm in the xy plane -------------------------
        rest = torch.zeros(21, 3)
        base_x = (-0.035, -0.02, 0.0, 0.018, 0.034)
        base_y = (0.02, 0.085, 0.09, 0.085, 0.075)
        seg = ((0.038, 0.03, 0.026), (0.04, 0.025, 0.02), (0.044, 0.028, 0.022), (0.04, 0.026, 0.02), (0.032, 0.02, 0.018))
        for f, chain in enumerate(self.FINGERS):
            p = torch.tensor([base_x[f], base_y[f], 0.0])
            direction = torch.tensor([-0.6, 0.8, 0.0]) if f == 0 else torch.tensor([0.05 * (f - 2), 1.0, 0.0])
            direction = direction / direction.norm()
            rest[chain[0]] = p
            for j in range(3):
                p = p + direction * seg[f][j]
                rest[chain[j + 1]] = p
        parents = [0] * 21
        for chain in self.FINGERS:
            parents[chain[0]] = 0
            for a, b in zip(chain[:-1], chain[1:]):
                parents[b] = a
        self.parents = parents
        # articulated joints (15): the first three of every finger chain; pose block j drives joint ART[j]
        self.art = [c for chain in self.FINGERS for c in chain[:3]]
        # ---- vertices: cylinders around the 20 bones + a palm slab, skinned to the bone's two end joints -------------------
        bones = [(parents[j], j) for j in range(1, 21)]
        per = num_verts // 22
        verts, w_idx, w_val, bone_of = [], [], [], []
        for b, (pa, ch) in enumerate(bones):
            n = per
            t = torch.rand(n, generator=g)
            ang = torch.rand(n, generator=g) * 2 * math.pi
            axis = rest[ch] - rest[pa]
            ax = axis / axis.norm()
            u = torch.linalg.cross(ax, torch.tensor([0.0, 0.0, 1.0]))
            u = u / u.norm()
            v = torch.linalg.cross(ax, u)
            radius = 0.009 if pa != 0 else 0.012
            pts = rest[pa] + t[:, None] * axis + radius * (torch.cos(ang)[:, None] * u + torch.sin(ang)[:, None] * v)
            verts.append(pts)
            w_idx.append(torch.tensor([[pa, ch]]).expand(n, 2))
            w_val.append(torch.stack((1 - t, t), dim=1))
            bone_of += [b] * n
        n_palm = num_verts - per * 20
        palm = torch.stack((torch.rand(n_palm, generator=g) * 0.08 - 0.04, torch.rand(n_palm, generator=g) * 0.08,
                            (torch.rand(n_palm, generator=g) - 0.5) * 0.02), dim=1)
        verts.append(palm)
        w_idx.append(torch.zeros(n_palm, 2, dtype=torch.long))
        w_val.append(torch.tensor([[1.0, 0.0]]).expand(n_palm, 2))
        bone_of += [-1] * n_palm
        self.register_buffer("rest_joints", rest)
        self.register_buffer("rest_verts", torch.cat(verts))
        self.register_buffer("skin_idx", torch.cat(w_idx).long())
        self.register_buffer("skin_w", torch.cat(w_val).float())
        # PCA basis of the pose space: orthonormal rows, scaled like MANO's components (a few hundredths of a radian per unit)
        q, _ = torch.linalg.qr(torch.randn(45, 45, generator=g))
        self.register_buffer("th_comps", (q * 0.02).contiguous())
        # fingertip contact zones, numbered as the reference uses them (optimization_hand.py:164-168 with the finger order of
        # get_attraction_loss, :240: keypoints 8, 12, 16, 20, 4 = index, middle, ring, pinky, thumb)
        bone_of = torch.tensor(bone_of)
        tip_bone = {kp: bones.index((parents[kp], kp)) for kp in (8, 12, 16, 20, 4)}
        self.contact_zones = {i + 1: torch.nonzero(bone_of == tip_bone[kp]).flatten().tolist() for i, kp in enumerate((8, 12, 16, 20, 4))}
        self.registered_beta = None
        if self.num_betas > 0:
            self._init_shape_space(g)

    def _init_shape_space(self, g: torch.Generator):
        """num_betas shape directions, drawn after (so without changing) everything above.  Direction d moves every bone
        along its own axis by a random fraction of its length (a few per cent per unit of beta) plus a small random
        sideways offset; the wrist stays at the origin.  The rest joints are a linear function of beta, and every vertex
        moves rigidly with the end joint of its bone (palm vertices: with a random palm stretch), so the skinning offsets
        rest[j] - rest[parent] and v_rest - j_k are linear in beta and the posed hand is affine in beta at a fixed pose."""
        D, rest, par = self.num_betas, self.rest_joints, self.parents
        stretch = torch.randn(D, 21, generator=g) * 0.03               # relative bone-length change per unit of beta
        side = torch.randn(D, 21, 3, generator=g) * 0.0005             # metres per unit of beta
        d_off = torch.zeros(D, 21, 3)
        for j in range(1, 21):
            d_off[:, j] = stretch[:, j, None] * (rest[j] - rest[par[j]]) + side[:, j]
        d_joints = torch.zeros(D, 21, 3)
        for chain in self.FINGERS:                                     # accumulate the offsets down each finger
            for j in chain:
                d_joints[:, j] = d_joints[:, par[j]] + d_off[:, j]
        palm = torch.randn(D, 3, generator=g) * torch.tensor([0.02, 0.02, 0.005])
        # a vertex follows its bone's end joint: v_rest - j_k changes only by the difference of the two end joints' motion
        end = self.skin_idx[:, 1].clone()
        is_palm = self.skin_w[:, 1] == 0
        d_verts = d_joints[:, end]                                     # (D, V, 3)
        d_verts[:, is_palm] = self.rest_verts[is_palm][None] * palm[:, None, :]
        self.register_buffer("shape_joints", d_joints.contiguous())
        self.register_buffer("shape_verts", d_verts.contiguous())

    def register_beta(self, th_betas=None):
        """The shape used by forward(..., use_registed_beta=True) (our_mano.py:211-216); ignored by a model without a shape
        space."""
        if self.num_betas == 0 or th_betas is None:
            return None
        self.registered_beta = torch.as_tensor(th_betas).reshape(1, self.num_betas).to(self.rest_joints)
        return None

    def pca_comps2pose(self, ncomps: int, pca: torch.Tensor) -> torch.Tensor:
        return pca.mm(self.th_comps[:ncomps])

    def _lbs_tables(self):
        block = [-1] * 21
        for a, j in enumerate(self.art):
            block[j] = a
        t = {"parents": torch.tensor(self.parents, dtype=torch.long), "pose_block": torch.tensor(block, dtype=torch.long),
             "rest_joints": self.rest_joints, "rest_verts": self.rest_verts, "skin_idx": self.skin_idx, "skin_w": self.skin_w,
             "comps": self.th_comps}
        if self.num_betas > 0:
            t["shape_joints"], t["shape_verts"] = self.shape_joints, self.shape_verts
        return t

    def forward(self, th_pose_coeffs, th_betas=None, th_trans=None, use_registed_beta=False, **_):
        P = th_pose_coeffs.shape[0]
        dev, dt = th_pose_coeffs.device, th_pose_coeffs.dtype
        Rg = rodrigues(th_pose_coeffs[:, :3])                                  # (P,3,3)
        Rl = rodrigues(th_pose_coeffs[:, 3:].reshape(P, 15, 3))                # (P,15,3,3)
        rest = self.rest_joints.to(dt)
        rest_verts = self.rest_verts.to(dt)
        if self.num_betas > 0:
            if th_betas is None and use_registed_beta:
                th_betas = self.registered_beta
            if th_betas is not None:  # per-candidate rest pose: (P,21,3) joints, (P,V,3) vertices, linear in beta
                b = th_betas.to(dt).reshape(-1, self.num_betas).expand(P, -1)
                rest = rest + (b @ self.shape_joints.to(dt).reshape(self.num_betas, -1)).view(P, 21, 3)
                rest_verts = rest_verts + (b @ self.shape_verts.to(dt).reshape(self.num_betas, -1)).view(P, -1, 3)
        shaped = rest.dim() == 3
        R_w = [None] * 21
        t_w = [None] * 21
        R_w[0] = Rg
        t_w[0] = torch.zeros(P, 3, dtype=dt, device=dev)
        art_of = {j: a for a, j in enumerate(self.art)}
        for chain in self.FINGERS:
            for j in chain:
                pa = self.parents[j]
                off = (rest[..., j, :] - rest[..., pa, :]).view(-1, 3, 1)
                t_w[j] = t_w[pa] + (R_w[pa] @ off).squeeze(-1)
                R_w[j] = R_w[pa] @ Rl[:, art_of[j]] if j in art_of else R_w[pa]
        R_w = torch.stack(R_w, dim=1)                                          # (P,21,3,3)
        t_w = torch.stack(t_w, dim=1)                                          # (P,21,3)
        # linear blend skinning: v = sum_k w_k (R_k (v_rest - j_k) + t_k)
        if shaped:
            rel = rest_verts[:, :, None, :] - rest[:, self.skin_idx]           # (P,V,2,3)
        else:
            rel = (rest_verts[:, None, :] - rest[self.skin_idx])[None]         # (1,V,2,3)
        Rk = R_w[:, self.skin_idx]                                             # (P,V,2,3,3)
        vk = (Rk @ rel[..., None]).squeeze(-1) + t_w[:, self.skin_idx]
        verts = (vk * self.skin_w.to(dt)[None, :, :, None]).sum(dim=2)         # (P,V,3)
        joints = t_w
        if th_trans is not None:
            verts = verts + th_trans[:, None, :]
            joints = joints + th_trans[:, None, :]
        return verts, joints
