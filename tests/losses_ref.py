"""Torch restatement of the seven terms of the reference's `GaussianDiffusion.training_losses` (diffusion/gaussian_diffusion.py:1239-1403), from
the maths of each term and tests/rot2xyz_ref.py for the joint positions. Runs in fp64 or fp32, on any device.

Every term is a `masked_l2` (:213-225): sum(mask * (a - b)^2) / (sum(mask) * a.shape[1] * a.shape[2]) over everything but the batch axis, with
the shapes the reference hands in - so the [B,1,T] inputs of orient / transl and the [B,J,T] input of body carry the frame count in their
divisor - and an empty mask divides 0 by 0.

tests/test_losses_cpu.py pins it to fixtures recorded from the reference's own code (tests/golden/losses_*.npz); the GPU tests use the fp64 run
as the truth and the fp32 run's deviation from it as the yardstick for the kernel; tools/loss_terms_bench.py times the fp32 run's expressions on
the device as "what a user would otherwise write"."""
import numpy as np
import torch

from tests.rot2xyz_ref import rot2xyz_ref, rotation_6d_to_matrix

TERMS = ("rot_mse", "rcxyz_mse", "vel_mse", "fc", "orient", "body", "transl")
FOOT_JOINTS = (7, 10, 8, 11)          # l_ankle, l_foot, r_ankle, r_foot in the reference's order (:1333-1334)
TRANSL_ROW = 55                       # (:1386-1387)


def masked_l2(a, b, mask):
    """:213-225. mask broadcasts against a; its own element count times a.shape[1] * a.shape[2] is the divisor."""
    loss = ((a - b) ** 2 * mask.to(a.dtype)).flatten(1).sum(1)
    return loss / (mask.flatten(1).sum(1) * (a.shape[1] * a.shape[2]))


def matrix_to_angle(m):
    """|| matrix_to_axis_angle(m) || through matrix_to_quaternion (utils/rotation_conversions.py:98-120: square roots of the positive parts,
    signs copied from the antisymmetric part, real part >= 0) and quaternion_to_axis_angle (:482-510, small-angle branch included)."""
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    sp = lambda v: torch.where(v > 0, torch.sqrt(torch.clamp(v, min=0)), torch.zeros_like(v))      # noqa: E731
    cs = lambda a, b: torch.where((a < 0) != (b < 0), -a, a)                                       # noqa: E731
    o0 = 0.5 * sp(1 + m00 + m11 + m22)
    o1 = cs(0.5 * sp(1 + m00 - m11 - m22), m[..., 2, 1] - m[..., 1, 2])
    o2 = cs(0.5 * sp(1 - m00 + m11 - m22), m[..., 0, 2] - m[..., 2, 0])
    o3 = cs(0.5 * sp(1 - m00 - m11 + m22), m[..., 1, 0] - m[..., 0, 1])
    v = torch.stack((o1, o2, o3), -1)
    norms = torch.linalg.norm(v, dim=-1, keepdim=True)
    half = torch.atan2(norms, o0[..., None])
    angles = 2 * half
    small = angles.abs() < 1e-6
    s = torch.where(small, 0.5 - angles * angles / 48, torch.sin(half) / torch.where(small, torch.ones_like(angles), angles))
    return torch.linalg.norm(v / s, dim=-1)


def joints_of(x, skeleton, dtype):
    """get_xyz (:1254-1258): rot2xyz(sample, mask=None, translation=True, glob=True, vertstrans=False) -> [B, J, 3, T], every frame, joint 0 subtracted."""
    return rot2xyz_ref(x, None, skeleton, "rot6d", True, True, False, dtype=dtype)


def loss_terms_ref(target, output, cmotion, mask, skeleton, vel_threshold, foot_joints=FOOT_JOINTS, transl_row=TRANSL_ROW, dtype=torch.float64,
                   xyz=None):
    """target / output / cmotion [B, R, 6, T], mask bool [B, T] -> dict of [B] tensors in `dtype` (all seven terms). `xyz`: the three
    joint tensors (target, output, cmotion) when the caller already has them."""
    t, o, c = (torch.as_tensor(a).to(dtype) for a in (target, output, cmotion))
    m4 = torch.as_tensor(mask).to(t.device).bool()[:, None, None, :]                # y['mask'] [B,1,1,T]
    m3 = m4.squeeze(1)
    tx, ox, cx = xyz if xyz is not None else (joints_of(a, skeleton, dtype) for a in (t, o, c))
    terms = {"rot_mse": masked_l2(t, o, m4), "rcxyz_mse": masked_l2(tx, ox, m4)}
    # velocities: frame differences of every row but the last, under the mask of the later frame
    tv, ov = t[..., 1:] - t[..., :-1], o[..., 1:] - o[..., :-1]
    terms["vel_mse"] = masked_l2(tv[:, :-1], ov[:, :-1], m4[..., 1:])
    # foot contact: where the ground truth's foot moves at most vel_threshold per frame, the predicted velocity vector is the error
    fj = list(foot_joints)
    gt_speed = torch.linalg.norm(tx[:, fj, :, 1:] - tx[:, fj, :, :-1], dim=2)       # [B,4,T-1]
    pv = ox[:, fj, :, 1:] - ox[:, fj, :, :-1]
    pv = torch.where((gt_speed <= vel_threshold)[:, :, None, :], pv, torch.zeros_like(pv))
    terms["fc"] = masked_l2(pv, torch.zeros_like(pv), m4[..., 1:])
    # the three distances to the actor, target's against output's
    rc, rt, ro = (rotation_6d_to_matrix(a[:, 0:1].permute(0, 1, 3, 2)) for a in (c, t, o))     # [B,1,T,3,3]
    terms["orient"] = masked_l2(matrix_to_angle(rc.transpose(-1, -2) @ rt), matrix_to_angle(rc.transpose(-1, -2) @ ro), m3)
    terms["body"] = masked_l2(torch.linalg.norm(cx - tx, dim=2), torch.linalg.norm(cx - ox, dim=2), m3)
    r = int(transl_row)
    ct, tt, ot = c[:, r:r + 1, 0:3], t[:, r:r + 1, 0:3], o[:, r:r + 1, 0:3]
    terms["transl"] = masked_l2(torch.linalg.norm(ct - tt, dim=2), torch.linalg.norm(ct - ot, dim=2), m3)
    return terms


def stack_terms(terms):
    """dict of [B] -> numpy [B, 7] in TERMS order."""
    return np.stack([np.asarray(terms[k].detach().cpu().double() if torch.is_tensor(terms[k]) else terms[k], dtype=np.float64) for k in TERMS], 1)
