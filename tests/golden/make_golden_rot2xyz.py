"""Golden vectors of the reference's rot2xyz wrappers, recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_rot2xyz.py

`Rotation2xyz_x.__call__` and `Rotation2xyz.__call__` (model/rotation2xyz.py:158-324 / :11-155) are run as they stand: the row split per person,
the rotation conversions of utils/rotation_conversions.py, masking, root subtraction and the translation term are the reference's own code.
What is absent here is the body layer they call (`smplx`, with licensed model files). It is replaced by a stand-in whose `forward` returns, as
`joints`, the posed skeleton joints of linear blend skinning's rigid-transform chain over a SYNTHETIC skeleton (regennet_amd.synth.make_skeleton)
- the quantity the real layer returns in joints 0..54 (0..23 for SMPL), model/smpl.py:108-116 - computed in fp64 from rest joints rounded to
fp32 like the real layer's buffers. The wrappers are fed x in fp64, so `expected` is fp64 throughout.

Only DATA is written: tests/golden/rot2xyz_<case>.npz with the input, mask, skeleton, settings and expected output."""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from regennet_amd import synth  # noqa: E402

B, T = 3, 7


class _SkeletonLayer(nn.Module):
    """Stand-in for smplx.SMPLXLayer / SMPLLayer: posed skeleton joints only."""
    skeleton = None          # set by the recorder before a wrapper is built
    pad_to = 127             # joints the real layer returns (SMPL-X: 127, SMPL: 45); the tail is never selected by 'smplx' / 'smpl'

    def __init__(self, *a, **k):
        super().__init__()
        self.num_betas = 10

    def posed(self, rot, betas):
        sk = type(self).skeleton
        b = betas.double()
        assert bool((b == b[:1]).all())
        rest = sk["rest_joints"].astype(np.float64) + sk["shape_joints"].astype(np.float64) @ b[0].numpy()
        rest = torch.from_numpy(rest.astype(np.float32).astype(np.float64))
        parents = sk["parents"]
        rot = rot.double()
        N, J = rot.shape[:2]
        assert J == len(parents)
        grot, pos = [rot[:, 0]], [rest[0].expand(N, 3)]
        for i in range(1, J):
            p = int(parents[i])
            grot.append(grot[p] @ rot[:, i])
            pos.append((grot[p] @ (rest[i] - rest[p])[:, None]).squeeze(-1) + pos[p])
        joints = torch.stack(pos, dim=1)
        joints = torch.cat([joints, torch.zeros(N, type(self).pad_to - J, 3, dtype=joints.dtype)], dim=1)
        return types.SimpleNamespace(joints=joints, vertices=torch.zeros(N, 1, 3, dtype=joints.dtype))


class _SMPLXLayer(_SkeletonLayer):
    def forward(self, betas=None, body_pose=None, left_hand_pose=None, right_hand_pose=None, global_orient=None, return_verts=True):
        N = body_pose.shape[0]
        eye = torch.eye(3, dtype=body_pose.dtype).expand(N, 3, 3, 3)     # jaw and eyes are not handed over (:294-301): identity, as in the real layer
        rot = torch.cat([global_orient.reshape(N, 1, 3, 3), body_pose, eye, left_hand_pose, right_hand_pose], dim=1)
        return self.posed(rot, betas)


class _SMPLLayer(_SkeletonLayer):
    pad_to = 45

    def forward(self, body_pose=None, global_orient=None, betas=None):
        N = body_pose.shape[0]
        return self.posed(torch.cat([global_orient.reshape(N, 1, 3, 3), body_pose], dim=1), betas)


def reference_wrappers():
    _ref_import.install()
    sys.modules["smplx"].SMPLXLayer = _SMPLXLayer
    sys.modules["smplx"].SMPLLayer = _SMPLLayer
    import model.smpl as ref_smpl
    from model.rotation2xyz import Rotation2xyz, Rotation2xyz_x
    # SMPL.forward appends 9 extra joints regressed from vertices (model/smpl.py:91-92); 'smpl' selects none of them
    ref_smpl.vertices2joints = lambda reg, v: torch.zeros(v.shape[0], 9, 3, dtype=v.dtype)
    return Rotation2xyz, Rotation2xyz_x


def random_rotmat(rng, shape):
    q = rng.standard_normal(shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., i] for i in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)


def make_x(rng, J, pose_rep, translation, glob, P):
    """fp32 [B, R, C * P, T]: un-normalised rot6d / quaternions (the conversions normalise), axis-angle vectors of up to a few radians, proper
    rotation matrices; the translation row is [tx, ty, tz, 0, ...] per person."""
    C = {"rot6d": 6, "rotvec": 3, "rotquat": 4, "rotmat": 9}[pose_rep]
    nrot = J if glob else J - 1
    shape = (B, T, nrot, P)
    if pose_rep == "rotmat":
        rot = random_rotmat(rng, shape)
    else:
        rot = rng.standard_normal(shape + (C,)) * (1.5 if pose_rep == "rotvec" else 1.0)
    rows = rot                                                        # [B, T, nrot, P, C]
    if translation:
        tr = np.zeros((B, T, 1, P, C))
        tr[..., :3] = rng.uniform(-1, 1, (B, T, 1, P, 3))
        rows = np.concatenate([rows, tr], axis=2)
    return np.ascontiguousarray(rows.reshape(B, T, rows.shape[2], P * C).transpose(0, 2, 3, 1)).astype(np.float32)


RAGGED = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0], [0, 1, 1, 0, 1, 0, 0]], dtype=bool)   # (frame 0 of motion 2 is masked: its translation still anchors the row)

CASES = {
    # name: (joints, pose_rep, translation, glob, vertstrans, persons, mask, beta, glob_rot)
    "p1": (55, "rot6d", True, True, True, 1, None, 0, None),
    "p2": (55, "rot6d", True, True, True, 2, None, 0, None),
    "ragged": (55, "rot6d", True, True, True, 1, RAGGED, 0, None),
    "p2_ragged": (55, "rot6d", True, True, True, 2, RAGGED, 0, None),
    "notrans": (55, "rot6d", False, True, True, 1, RAGGED, 0, None),
    "novertstrans": (55, "rot6d", True, True, False, 1, RAGGED, 0, None),
    "noglob": (55, "rot6d", True, False, True, 1, RAGGED, 0, [2.5, 0.5, -0.25]),
    "rotvec": (55, "rotvec", True, True, True, 1, RAGGED, 0, None),
    "rotquat": (55, "rotquat", True, True, True, 2, RAGGED, 0, None),
    "rotmat": (55, "rotmat", True, True, True, 1, RAGGED, 0, None),
    "beta": (55, "rot6d", True, True, True, 1, RAGGED, 1.5, None),
    "smpl24": (24, "rot6d", True, True, True, 1, RAGGED, 0, None),
}


def main():
    Rotation2xyz, Rotation2xyz_x = reference_wrappers()
    for n, (name, (J, pose_rep, translation, glob, vertstrans, P, mask, beta, glob_rot)) in enumerate(CASES.items()):
        sk = synth.make_skeleton(J, seed=J)
        _SkeletonLayer.skeleton = sk
        rng = np.random.Generator(np.random.PCG64(100 + n))
        x = make_x(rng, J, pose_rep, translation, glob, P)
        with mock.patch("numpy.load", lambda *a, **k: np.zeros((9, 1), np.float32)):       # J_regressor_extra (model/smpl.py:76), unused by 'smpl'
            wrapper = (Rotation2xyz_x if J == 55 else Rotation2xyz)("cpu")
        out = wrapper(torch.from_numpy(x).double(), None if mask is None else torch.from_numpy(mask), pose_rep=pose_rep, translation=translation,
                      glob=glob, jointstype="smplx" if J == 55 else "smpl", vertstrans=vertstrans, betas=None, beta=beta, glob_rot=glob_rot,
                      num_person=P)
        assert out.dtype == torch.float64 and tuple(out.shape) == (B, J, 3 * P, T), (out.dtype, out.shape)
        path = os.path.join(HERE, f"rot2xyz_{name}.npz")
        np.savez_compressed(path, x=x, mask=np.ones((B, T), bool) if mask is None else mask, mask_none=np.array(mask is None),
                            rest_joints=sk["rest_joints"], parents=sk["parents"], shape_joints=sk["shape_joints"], pose_rep=np.array(pose_rep),
                            translation=np.array(translation), glob=np.array(glob), vertstrans=np.array(vertstrans), num_person=np.array(P),
                            beta=np.array(float(beta)), glob_rot=np.zeros(3, np.float32) if glob_rot is None else np.array(glob_rot, np.float32),
                            jointstype=np.array("smplx" if J == 55 else "smpl"), expected=out.numpy())
        print(f"{name:14s} x {x.shape} -> {tuple(out.shape)}  max|xyz| {float(out.abs().max()):.3f}  {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
