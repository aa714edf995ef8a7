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
        Keypoints are the joint positions.  Optional entries, for a hand with MANO's structure (a table without them is a plain
        hand, and everything computed from it is what it was before they existed):
          posedirs (V,3,9 B): pose blend shapes over the B pose blocks, v_rest += posedirs . vec(R_b - I) with feature
          9 b + 3 r + c = (R_b - I)[r][c] of pose block b's own rotation (the order of the reference's th_pose_map);
          pose_mean (num_pose,): added to the joint angles before Rodrigues;
          kp_vertex (J,) int64: entry j >= 0 makes table joint j a keypoint read from that SKINNED vertex (a fingertip) -- such
          a joint has no rotation, is nobody's parent and no skin index names it; -1 = a real joint;
          centre_root bool: vertices and keypoints have keypoint 0 subtracted before the translation is added.
        Joints stay in keypoint order (root, then per finger three joints and the tip) either way; rest joints regressed from
        the shaped vertices are linear in beta and fit rest_joints / shape_joints.
        The tables are accepted only if lbs_forward_from_tables reproduces forward() in float64 to TABLES_TOL at seeded random
        poses (and shape codes); a model whose claim leaves a term out (a MANO layer that claims plain tables without its pose
        blend shapes) fails that check and returns None.  Built and checked once per model."""
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
        if not _mano_entries_consistent(t, self.num_pose):
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


def lbs_forward_from_tables(tables, pose, trans, beta=None, root_R=None):
    """vertices (P,V,3), keypoints (P,J,3) of HandModel.skinning_tables() at pose (P, 3 + num_pose) = [global axis-angle | joint
    angles], trans (P,3) and, for a model with a shape space, beta (P|1, D) -- in pose's dtype, on pose's device:
        rest = rest_* + beta @ shape_*;  R_0 = rodrigues(pose[:, :3]), t_0 = rest_joints[0];
        t_j = t_parent + R_parent (rest_j - rest_parent),  R_j = R_parent rodrigues(pose block pose_block[j]) (or R_parent);
        v = sum_k w_k (R_k (rest_v - rest_k) + t_k) + trans;  keypoints = t_j + trans.
    With the optional entries: the joint angles have pose_mean added, rest_v has posedirs . vec(R_b - I) added (after the shape
    term, before the skinning), keypoint j with kp_vertex[j] >= 0 is that skinned vertex, and with centre_root keypoint 0 is
    subtracted from vertices and keypoints before trans is added.
    root_R (P,3,3): the root's rotation as a matrix, used in place of rodrigues(pose[:, :3]) (which is then not read) -- the way
    the pose optimiser carries it."""
    dt, dev, P = pose.dtype, pose.device, pose.shape[0]
    T = lambda k: tables[k].to(dev)
    parents, block = [int(v) for v in tables["parents"]], [int(v) for v in tables["pose_block"]]
    rest, verts = T("rest_joints").to(dt)[None], T("rest_verts").to(dt)[None]
    if beta is not None and "shape_joints" in tables:
        b = beta.to(dev, dt).reshape(-1, tables["shape_joints"].shape[0])
        rest = rest + torch.einsum("pd,djc->pjc", b, T("shape_joints").to(dt))
        verts = verts + torch.einsum("pd,dvc->pvc", b, T("shape_verts").to(dt))
    angles = pose[:, 3:] + T("pose_mean").to(dt)[None] if "pose_mean" in tables else pose[:, 3:]
    Rl = rodrigues(angles.reshape(P, -1, 3))
    if "posedirs" in tables:
        feat = (Rl - torch.eye(3, dtype=dt, device=dev)).reshape(P, -1)
        verts = verts + torch.einsum("vcf,pf->pvc", T("posedirs").to(dt), feat)
    R_w, t_w = [rodrigues(pose[:, :3]) if root_R is None else root_R.to(dev, dt)], [rest[:, 0].expand(P, 3)]
    for j in range(1, len(parents)):
        pa = parents[j]
        t_w.append(t_w[pa] + (R_w[pa] @ (rest[:, j] - rest[:, pa])[..., None]).squeeze(-1))
        R_w.append(R_w[pa] @ Rl[:, block[j]] if block[j] >= 0 else R_w[pa])
    R_w, t_w = torch.stack(R_w, dim=1), torch.stack(t_w, dim=1)
    idx, w = T("skin_idx"), T("skin_w").to(dt)
    rel = verts[:, :, None, :] - rest[:, idx]                                   # (P|1, V, K, 3)
    vk = (R_w[:, idx] @ rel[..., None]).squeeze(-1) + t_w[:, idx]
    out = (vk * w[None, :, :, None]).sum(dim=2)
    if "kp_vertex" in tables:
        kpv = [int(v) for v in tables["kp_vertex"]]
        t_w = torch.stack([t_w[:, j] if v < 0 else out[:, v] for j, v in enumerate(kpv)], dim=1)
    if tables.get("centre_root", False):
        centre = t_w[:, :1]
        out, t_w = out - centre, t_w - centre
    return out + trans[:, None, :], t_w + trans[:, None, :]


def _mano_entries_consistent(t, num_pose):
    """The optional entries of skinning_tables() against the rest of the claim (shapes, and what a kp_vertex joint may not be)."""
    J, V = t["parents"].numel(), t["rest_verts"].shape[0]
    if "posedirs" in t and (t["posedirs"].dim() != 3 or tuple(t["posedirs"].shape[:2]) != (V, 3) or
                            t["posedirs"].shape[2] != 3 * num_pose):
        return False
    if "pose_mean" in t and t["pose_mean"].numel() != num_pose:
        return False
    if "kp_vertex" in t:
        kpv = [int(v) for v in t["kp_vertex"]]
        if len(kpv) != J or kpv[0] >= 0 or any(v >= V for v in kpv):
            return False
        taken = {j for j, v in enumerate(kpv) if v >= 0}
        named = {int(p) for p in t["parents"][1:]} | {int(i) for i in t["skin_idx"].flatten()}
        if taken & named or any(int(t["pose_block"][j]) >= 0 for j in taken):
            return False
    return True


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


NAMED_HAND_MODELS = ("synthetic", "synthetic_shaped", "synthetic_mano")


def named_hand_model(name: str) -> HandModel:
    """The hand models --hand_model selects by name: 'synthetic' (SyntheticLBSHand), 'synthetic_shaped' (the same with 10 shape
    dimensions), 'synthetic_mano' (SyntheticManoHand: MANO's structure with seeded tables)."""
    if name not in NAMED_HAND_MODELS:
        raise ValueError("hand_model: %s or a models.hand_model.HandModel instance" % ", ".join(repr(n) for n in NAMED_HAND_MODELS))
    return SyntheticManoHand() if name == "synthetic_mano" else SyntheticLBSHand(num_betas=10 if name == "synthetic_shaped" else 0)


class SyntheticManoHand(HandModel):
    """A hand with MANO's STRUCTURE (the model the reference tracks, third_party/mano/our_mano.py:218-360) and seeded random
    tables -- the licensed assets stay out of this repository:
      v_shaped = v_template + shapedirs beta;  rest joints = J_regressor v_shaped (16 joints: the wrist, then three per finger in
      MANO's order index, middle, pinky, ring, thumb, a three-level tree under the wrist);
      joint angles = hands_mean + pose;  v_posed = v_shaped + posedirs vec(R_j - I) over the 15 finger joints (135 features);
      linear blend skinning of v_posed with dense weights (V,16), at most `weights_per_vertex` <= 4 non-zeros per vertex;
      keypoints = the 16 joints and five skinned fingertip VERTICES (thumb, index, middle, ring, pinky), reordered to
      [0, 13, 14, 15, 16, 1, 2, 3, 17, ...] = wrist, then thumb, index, middle, ring, pinky with the tip last;
      vertices and keypoints centred on keypoint 0, then translated.
    `tip_vertices` overrides the five fingertip vertex indices (default: the far end of each finger's last bone)."""

    PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
    KP_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)  # over [16 joints | 5 tips]

    def __init__(self, num_verts: int = 778, seed: int = 0, weights_per_vertex: int = 4, tip_vertices=None):
        super().__init__()
        if num_verts < 22 or not 1 <= weights_per_vertex <= 4:
            raise ValueError("SyntheticManoHand: at least 22 vertices (one per bone and a palm) and 1..4 weights per vertex")
        g = torch.Generator().manual_seed(seed)
        V = self.num_verts = int(num_verts)
        self.num_pose, self.num_betas = 45, 10
        # ---- a hand-sized skeleton in keypoint order (wrist at the origin, fingers along +y, palm in the xy plane) ----------
        fingers = SyntheticLBSHand.FINGERS
        skel = torch.zeros(21, 3)
        base = ((-0.035, 0.02), (-0.02, 0.085), (0.0, 0.09), (0.018, 0.085), (0.034, 0.075))
        seg = ((0.038, 0.03, 0.026), (0.04, 0.025, 0.02), (0.044, 0.028, 0.022), (0.04, 0.026, 0.02), (0.032, 0.02, 0.018))
        kp_parent = [0] * 21
        for f, chain in enumerate(fingers):
            p = torch.tensor([base[f][0], base[f][1], 0.0])
            d = torch.tensor([-0.6, 0.8, 0.0]) if f == 0 else torch.tensor([0.05 * (f - 2), 1.0, 0.0])
            d = d / d.norm()
            skel[chain[0]] = p
            for s in range(3):
                p = p + d * seg[f][s]
                skel[chain[s + 1]] = p
            for a, b in zip(chain[:-1], chain[1:]):
                kp_parent[b] = a
        mano_of = {k: m for k, m in enumerate(self.KP_ORDER) if m < 16}   # keypoint -> MANO joint (tips have none)
        # ---- template: a tube of vertices around each of the 20 bones and a palm slab; dense skinning weights ---------------
        per = V // 22
        verts, W, bone_of, along = [], torch.zeros(V, 16), [], []
        for b in range(1, 21):
            pa = kp_parent[b]
            t, ang = torch.rand(per, generator=g), torch.rand(per, generator=g) * 2 * math.pi
            axis = skel[b] - skel[pa]
            ax = axis / axis.norm()
            u = torch.linalg.cross(ax, torch.tensor([0.0, 0.0, 1.0]))
            u = u / u.norm()
            r = 0.009 if pa != 0 else 0.012
            verts.append(skel[pa] + t[:, None] * axis + r * (torch.cos(ang)[:, None] * u + torch.sin(ang)[:, None] * torch.linalg.cross(ax, u)))
            rows = slice((b - 1) * per, b * per)
            if b in mano_of:                                   # between two joints: blended along the bone
                W[rows, mano_of[pa]] += 1 - t
                W[rows, mano_of[b]] += t
            else:                                              # the last bone ends in a fingertip, which is no joint
                W[rows, mano_of[pa]] += 1.0
            bone_of += [b] * per
            along.append(t)
        n_palm = V - 20 * per
        verts.append(torch.stack((torch.rand(n_palm, generator=g) * 0.08 - 0.04, torch.rand(n_palm, generator=g) * 0.08,
                                  (torch.rand(n_palm, generator=g) - 0.5) * 0.02), dim=1))
        W[20 * per:, 0] = 1.0
        bone_of += [0] * n_palm
        W = W + 0.15 * torch.rand(V, 16, generator=g) * (torch.rand(V, 16, generator=g) < 0.25)  # a little of a few other joints
        keep = W.topk(weights_per_vertex, dim=1)
        W = torch.zeros(V, 16).scatter_(1, keep.indices, keep.values)
        W = W / W.sum(dim=1, keepdim=True)
        v_template = torch.cat(verts)
        bone_of = torch.tensor(bone_of)
        # ---- joint regressor: each joint a convex combination of the template vertices nearest to it ------------------------
        Jreg = torch.zeros(16, V)
        for k, m in mano_of.items():
            near = (v_template - skel[k]).norm(dim=1).topk(min(8, V), largest=False).indices
            Jreg[m, near] = torch.rand(len(near), generator=g) + 0.1
        Jreg = Jreg / Jreg.sum(dim=1, keepdim=True)
        q, _ = torch.linalg.qr(torch.randn(45, 45, generator=g))
        self.register_buffer("th_v_template", v_template.contiguous())
        self.register_buffer("th_shapedirs", (torch.randn(V, 3, 10, generator=g) * 0.0008).contiguous())
        # offsets of a few millimetres at joint angles of +-1.5 rad (135 features of size up to ~1)
        self.register_buffer("th_posedirs", (torch.randn(V, 3, 135, generator=g) * 3e-4).contiguous())
        self.register_buffer("th_J_regressor", Jreg.contiguous())
        self.register_buffer("th_weights", W.contiguous())
        self.register_buffer("th_hands_mean", (torch.randn(45, generator=g) * 0.1).contiguous())
        self.register_buffer("th_comps", (q * 0.02).contiguous())
        tip_bone = [chain[3] for chain in fingers]                       # thumb, index, middle, ring, pinky
        if tip_vertices is None:
            tip_vertices = [(b - 1) * per + int(along[b - 1].argmax()) for b in tip_bone]
        if len(tip_vertices) != 5 or any(not 0 <= int(v) < V for v in tip_vertices):
            raise ValueError("SyntheticManoHand: tip_vertices is five vertex indices")
        self.tip_vertices = [int(v) for v in tip_vertices]
        # forward()'s gathers as device-side index tensors (a Python list as an index is a host copy: a graph cannot hold it)
        self.register_buffer("th_tip_idx", torch.tensor(self.tip_vertices, dtype=torch.long))
        self.register_buffer("th_kp_order", torch.tensor(self.KP_ORDER, dtype=torch.long))
        # contact zones in the optimiser's finger order (index, middle, ring, pinky, thumb): the last bone's vertices
        self.contact_zones = {i + 1: torch.nonzero(bone_of == kp).flatten().tolist() for i, kp in enumerate((8, 12, 16, 20, 4))}
        self.registered_beta = None

    def register_beta(self, th_betas=None):
        """The shape forward(..., use_registed_beta=True) uses (our_mano.py:211-216)."""
        if th_betas is None:
            return None
        self.registered_beta = torch.as_tensor(th_betas).reshape(1, self.num_betas).to(self.th_v_template)
        return None

    def pca_comps2pose(self, ncomps: int, pca: torch.Tensor) -> torch.Tensor:
        return pca.mm(self.th_comps[:ncomps])

    def _shaped(self, beta, dt):
        """(v_shaped (B|1,V,3), rest joints (B|1,16,3)) in dtype dt."""
        v = self.th_v_template.to(dt)[None]
        if beta is not None:
            v = v + torch.einsum("vcd,pd->pvc", self.th_shapedirs.to(dt), beta.to(dt).reshape(-1, self.num_betas))
        return v, torch.einsum("jv,pvc->pjc", self.th_J_regressor.to(dt), v)

    def forward(self, th_pose_coeffs, th_betas=None, th_trans=None, use_registed_beta=False, **_):
        P, dt = th_pose_coeffs.shape[0], th_pose_coeffs.dtype
        if th_betas is None and use_registed_beta:
            th_betas = self.registered_beta
        v_shaped, joints = self._shaped(th_betas, dt)
        full = torch.cat([th_pose_coeffs[:, :3], self.th_hands_mean.to(dt)[None] + th_pose_coeffs[:, 3:]], dim=1)
        R = rodrigues(full.reshape(P, 16, 3))
        feat = (R[:, 1:] - torch.eye(3, dtype=dt, device=R.device)).reshape(P, 135)
        v_posed = v_shaped + torch.einsum("vcf,pf->pvc", self.th_posedirs.to(dt), feat)
        # kinematic chain: world rotation and position of every joint
        R_w, t_w = [R[:, 0]], [joints[:, 0].expand(P, 3)]
        for m in range(1, 16):
            pa = self.PARENTS[m]
            t_w.append(t_w[pa] + (R_w[pa] @ (joints[:, m] - joints[:, pa])[..., None]).squeeze(-1))
            R_w.append(R_w[pa] @ R[:, m])
        R_w, t_w = torch.stack(R_w, dim=1), torch.stack(t_w, dim=1)
        # skinning with the blended transforms: A_v = sum_j w_vj [R_j | t_j - R_j j_j]
        shift = t_w - (R_w @ joints[..., None].expand(P, 16, 3, 1)).squeeze(-1)
        weights = self.th_weights.to(dt)
        A_rot, A_tr = torch.einsum("vj,pjab->pvab", weights, R_w), torch.einsum("vj,pja->pva", weights, shift)
        verts = (A_rot @ v_posed[..., None].expand(P, -1, 3, 1)).squeeze(-1) + A_tr
        kp = torch.cat([t_w, verts.index_select(1, self.th_tip_idx)], dim=1).index_select(1, self.th_kp_order)
        centre = kp[:, :1]
        verts, kp = verts - centre, kp - centre
        if th_trans is not None:
            verts, kp = verts + th_trans[:, None, :], kp + th_trans[:, None, :]
        return verts, kp

    def _lbs_tables(self):
        order = self.KP_ORDER
        at = {m: k for k, m in enumerate(order)}                          # MANO joint / tip slot -> table joint
        parents = [0 if m >= 16 or m == 0 else at[self.PARENTS[m]] for m in order]
        block = [m - 1 if 1 <= m < 16 else -1 for m in order]
        kp_vertex = [self.tip_vertices[m - 16] if m >= 16 else -1 for m in order]
        # rest joints: the regressor's rows for the 16 joints, the fingertip vertex's own row for a tip (not read)
        rows = torch.stack([self.th_J_regressor[m] if m < 16 else torch.nn.functional.one_hot(
            torch.tensor(self.tip_vertices[m - 16]), self.num_verts).to(self.th_J_regressor) for m in order])
        keep = self.th_weights.topk(4, dim=1)
        K = max(1, int((keep.values > 0).sum(dim=1).max()))
        idx = torch.tensor([at[int(m)] for m in keep.indices[:, :K].flatten()], dtype=torch.long).view(-1, K)
        shape_verts = self.th_shapedirs.permute(2, 0, 1)
        return {"parents": torch.tensor(parents, dtype=torch.long), "pose_block": torch.tensor(block, dtype=torch.long),
                "rest_joints": rows @ self.th_v_template, "rest_verts": self.th_v_template,
                "shape_joints": torch.einsum("jv,dvc->djc", rows, shape_verts).contiguous(), "shape_verts": shape_verts.contiguous(),
                "skin_idx": idx.to(self.th_weights.device), "skin_w": keep.values[:, :K].contiguous(), "comps": self.th_comps,
                "posedirs": self.th_posedirs, "pose_mean": self.th_hands_mean,
                "kp_vertex": torch.tensor(kp_vertex, dtype=torch.long), "centre_root": True}
