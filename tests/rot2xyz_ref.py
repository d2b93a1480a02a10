"""Torch restatement of the reference's rot2xyz for the skeleton joint types: `Rotation2xyz_x.__call__` / `Rotation2xyz.__call__`
(model/rotation2xyz.py:158-324 / :11-155) around the posed-joint chain of the body layer they call (linear blend skinning's rigid
transforms: 4x4 products down the parent table). Runs in fp64 or fp32, on any device.

tests/test_rot2xyz_cpu.py pins it to the goldens recorded from the reference's own wrappers (tests/golden/rot2xyz_*.npz); the GPU tests use the
fp64 run as the truth and the fp32 run's deviation from it as the yardstick for the kernel; tools/rot2xyz_bench.py times the fp32 run on the device
as "what a user would otherwise write"."""
import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = {"rot6d": 6, "rotvec": 3, "rotquat": 4, "rotmat": 9}


def quaternion_to_matrix(q):                                  # utils/rotation_conversions.py:38-66
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def axis_angle_to_matrix(aa):                                 # :418-479, through the quaternion
    angles = torch.norm(aa, p=2, dim=-1, keepdim=True)
    half = 0.5 * angles
    small = angles.abs() < 1e-6
    s = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / torch.where(small, torch.ones_like(angles), angles))
    return quaternion_to_matrix(torch.cat([torch.cos(half), aa * s], dim=-1))


def rotation_6d_to_matrix(d6):                                # :513-534
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def to_matrix(rows, pose_rep):
    if pose_rep == "rotvec":
        return axis_angle_to_matrix(rows)
    if pose_rep == "rotmat":
        return rows.reshape(rows.shape[:-1] + (3, 3))
    if pose_rep == "rotquat":
        return quaternion_to_matrix(rows)
    if pose_rep == "rot6d":
        return rotation_6d_to_matrix(rows)
    raise NotImplementedError("No geometry for this one.")


def posed_joints(rot, rest, parents):
    """rot [N, J, 3, 3], rest [J, 3] -> [N, J, 3]: the translation parts of G_0 = [R_0 | j_0], G_i = G_parent(i) @ [R_i | j_i - j_parent(i)]."""
    N, J = rot.shape[:2]
    rel = rest.clone()
    if J > 1:
        rel[1:] = rest[1:] - rest[torch.as_tensor(np.asarray(parents[1:]), dtype=torch.long, device=rest.device)]
    tm = torch.zeros(N, J, 4, 4, dtype=rot.dtype, device=rot.device)
    tm[:, :, :3, :3] = rot
    tm[:, :, :3, 3] = rel
    tm[:, :, 3, 3] = 1
    chain = [tm[:, 0]]
    for i in range(1, J):
        chain.append(torch.matmul(chain[int(parents[i])], tm[:, i]))
    return torch.stack(chain, dim=1)[:, :, :3, 3]


def rest_with_betas(skeleton, betas=None, beta=0):
    """fp64 numpy [J, 3]: rest + sum_k betas[k] shape_joints[:, :, k]; betas None -> beta goes into betas[1] (:289-292)."""
    rest = np.asarray(skeleton["rest_joints"], dtype=np.float64)
    sj = skeleton.get("shape_joints", None)
    if betas is None:
        betas = np.zeros(10 if sj is None else sj.shape[2])
        betas[1] = beta
    betas = np.asarray(betas, dtype=np.float64)
    if not betas.any():
        return rest
    return rest + np.asarray(sj, dtype=np.float64)[:, :, :len(betas)] @ betas


def rot2xyz_ref(x, mask, skeleton, pose_rep, translation, glob, vertstrans, betas=None, beta=0, glob_rot=None, num_person=1,
                dtype=torch.float64, return_rotations=False):
    """x [B, R, C * P, T] -> [B, J, 3 * P, T] in `dtype`, on x's device. `skeleton`: dict(rest_joints, parents[, shape_joints])."""
    x = torch.as_tensor(x).to(dtype)
    dev = x.device
    parents = np.asarray(skeleton["parents"]).reshape(-1)
    # the kernel's rest joints are fp32, like the reference layer's buffers: both runs start from those values
    rest = torch.from_numpy(rest_with_betas(skeleton, betas, beta).astype(np.float32)).to(device=dev, dtype=dtype)
    B, _, F_, T = x.shape
    if mask is None:
        mask = torch.ones((B, T), dtype=torch.bool, device=dev)
    mask = torch.as_tensor(mask).to(dev).bool()
    P = int(num_person)
    C = F_ // P
    outs, rots = [], []
    for xp in torch.split(x, C, dim=2):
        xt = xp[:, -1, :3] if translation else None            # [B, 3, T]
        xr = (xp[:, :-1] if translation else xp).permute(0, 3, 1, 2)            # [B, T, rows, C]
        rot = to_matrix(xr.reshape(B * T, xr.shape[2], C), pose_rep)
        if not glob:
            g = axis_angle_to_matrix(torch.tensor(np.asarray(glob_rot, dtype=np.float32))).to(device=dev, dtype=dtype)   # fp32, like torch.tensor(glob_rot)
            rot = torch.cat([g.view(1, 1, 3, 3).expand(B * T, 1, 3, 3), rot], dim=1)
        rots.append(rot.reshape(B, T, -1, 3, 3))
        joints = posed_joints(rot, rest, parents).reshape(B, T, -1, 3)
        xyz = torch.where(mask[:, :, None, None], joints, torch.zeros_like(joints)).permute(0, 2, 3, 1).contiguous()
        xyz = xyz - xyz[:, [0], :, :]
        if translation and vertstrans:
            if P == 1:
                xt = xt - xt[:, :, [0]]
            xyz = xyz + xt[:, None, :, :]
        outs.append(xyz)
    out = torch.cat(outs, 2)
    if return_rotations:
        return out, torch.stack(rots, dim=1)                   # [B, P, T, J, 3, 3]
    return out
