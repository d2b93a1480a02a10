"""Golden vectors of the reference's rot2xyz wrappers given a `betas` tensor with ONE ROW PER UNMASKED FRAME (model/rotation2xyz.py hands it
straight to the body layer), recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_rot2xyz_shaped.py

The harness is make_golden_rot2xyz.py's / make_golden_rot2verts.py's: `Rotation2xyz_x.__call__` and `Rotation2xyz.__call__` run as they stand
in fp64 - the row split per person (every person gets the same rows), conversions, masking, root subtraction, translation - over a stand-in body
layer. Those two scripts' stand-ins assert equal rows; the `posed` assigned here forms the rest joints and v_shaped PER ROW, as smplx.lbs.lbs
does (blend_shapes, then J_regressor @ v_shaped = rest_joints + shape_joints . betas for a body file), from arrays rounded to fp32.

Only DATA is written: tests/golden/shaped_rot2xyz_<case>.npz (jointstype 'smplx' / 'smpl') and shaped_rot2verts_<case>.npz ('vertices') with
the input, mask, betas rows, settings, make_body's arguments with a sha256 of its arrays, the expected output and `fp32_dev`: how far the fp32
run of tests/rot2xyz_shaped_ref.py is from `expected`. (The names do not start with rot2xyz_ / rot2verts_: the one-shape tests collect those.)"""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_golden_rot2xyz as harness  # noqa: E402
from regennet_amd import synth  # noqa: E402

B, T = harness.B, harness.T


def lbs64_rows(rot, betas, body):
    """rot [N, J, 3, 3] fp64, betas [N, nb] (nb <= the body's) -> (joints [N, J, 3], vertices [N, V, 3]), after smplx.lbs.lbs, a shape per row."""
    mesh = body["mesh"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).astype(np.float64))      # noqa: E731
    b = d(betas.detach().numpy())
    N, J = rot.shape[:2]
    nb = b.shape[1]
    parents = body["parents"]
    v_shaped = d(mesh["v_template"])[None] + torch.einsum("bl,mkl->bmk", b, d(mesh["shapedirs"][:, :, :nb]))
    rest = d(body["rest_joints"])[None] + torch.einsum("bl,jkl->bjk", b, d(body["shape_joints"][:, :, :nb]))
    pose_feature = (rot[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(N, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, d(mesh["posedirs"])).view(N, -1, 3)
    rel = rest.clone()
    rel[:, 1:] = rest[:, 1:] - rest[:, parents[1:].astype(np.int64)]
    tm = torch.cat([F.pad(rot, [0, 0, 0, 1]), F.pad(rel.reshape(N, J, 3, 1), [0, 0, 0, 1], value=1.0)], dim=3)      # [N, J, 4, 4]
    chain = [tm[:, 0]]
    for i in range(1, J):
        chain.append(torch.matmul(chain[int(parents[i])], tm[:, i]))
    transforms = torch.stack(chain, dim=1)
    joints = transforms[:, :, :3, 3]
    rest_h = F.pad(rest.reshape(N, J, 3, 1), [0, 0, 0, 1])
    A = transforms - F.pad(torch.matmul(transforms, rest_h), [3, 0, 0, 0, 0, 0, 0, 0])
    Tm = torch.matmul(d(mesh["lbs_weights"])[None].expand(N, -1, -1), A.view(N, J, 16)).view(N, -1, 4, 4)
    v_h = torch.cat([v_posed, torch.ones(N, v_posed.shape[1], 1, dtype=torch.float64)], dim=2)
    return joints, torch.matmul(Tm, v_h[..., None])[:, :, :3, 0]


def posed(self, rot, betas):
    assert betas.shape[0] == rot.shape[0], (betas.shape, rot.shape)         # one row per unmasked frame
    joints, vertices = lbs64_rows(rot.double(), betas, type(self).skeleton)
    joints = torch.cat([joints, torch.zeros(joints.shape[0], type(self).pad_to - joints.shape[1], 3, dtype=joints.dtype)], dim=1)
    return types.SimpleNamespace(joints=joints, vertices=vertices)


CASES = {
    # name: (joints, vertices, pose_rep, glob, persons, mask, betas per row, glob_rot)
    "p1_ragged": (55, 130, "rot6d", True, 1, harness.RAGGED, 10, None),
    "p2_ragged": (55, 130, "rot6d", True, 2, harness.RAGGED, 10, None),             # both persons take the same rows
    "smpl24": (24, 70, "rot6d", True, 1, None, 10, None),
    "noglob_rotvec": (55, 130, "rotvec", False, 1, harness.RAGGED, 10, [2.5, 0.5, -0.25]),
    "nb3": (55, 130, "rot6d", True, 1, harness.RAGGED, 3, None),                    # 3 betas against a 10-direction file
}


def main():
    from tests.rot2verts_ref import body_sha256
    from tests.rot2xyz_shaped_ref import rows_to_frames, shaped_ref
    harness._SkeletonLayer.posed = posed
    Rotation2xyz, Rotation2xyz_x = harness.reference_wrappers()
    for n, (name, (J, V, pose_rep, glob, P, mask, nb, glob_rot)) in enumerate(CASES.items()):
        args = dict(njoints=J, nverts=V, nbetas=10, seed=J)
        body = synth.make_body(**args)
        harness._SkeletonLayer.skeleton = body
        rng = np.random.Generator(np.random.PCG64(300 + n))
        x = harness.make_x(rng, J, pose_rep, True, glob, P)
        n_live = B * T if mask is None else int(mask.sum())
        rows = rng.standard_normal((n_live, nb)).astype(np.float32)
        with mock.patch("numpy.load", lambda *a, **k: np.zeros((9, 1), np.float32)):       # J_regressor_extra (model/smpl.py:76), unused here
            wrapper = (Rotation2xyz_x if J == 55 else Rotation2xyz)("cpu")
        m = None if mask is None else torch.from_numpy(mask)
        kw = dict(pose_rep=pose_rep, translation=True, glob=glob, vertstrans=True, glob_rot=glob_rot, num_person=P)
        for kind, jointstype, rows_out in (("rot2xyz", "smplx" if J == 55 else "smpl", J), ("rot2verts", "vertices", V)):
            out = wrapper(torch.from_numpy(x).double(), m, jointstype=jointstype, betas=torch.from_numpy(rows).double(), beta=0, **kw)
            assert out.dtype == torch.float64 and tuple(out.shape) == (B, rows_out, 3 * P, T), (out.dtype, out.shape)
            bt = rows_to_frames(rows, mask, B, T, P)
            rkw = dict(kw, vertices=kind == "rot2verts")
            d64 = float((shaped_ref(x, m, body, bt, dtype=torch.float64, **rkw) - out).abs().max())
            d32 = float((shaped_ref(x, m, body, bt, dtype=torch.float32, **rkw).double() - out).abs().max())
            path = os.path.join(HERE, f"shaped_{kind}_{name}.npz")
            np.savez_compressed(path, x=x, mask=np.ones((B, T), bool) if mask is None else mask, mask_none=np.array(mask is None), betas=rows,
                                body_args=np.array([args[k] for k in ("njoints", "nverts", "nbetas", "seed")]), body_sha256=np.array(body_sha256(body)),
                                pose_rep=np.array(pose_rep), translation=np.array(True), glob=np.array(glob), vertstrans=np.array(True),
                                num_person=np.array(P), glob_rot=np.zeros(3, np.float32) if glob_rot is None else np.array(glob_rot, np.float32),
                                jointstype=np.array(jointstype), fp32_dev=np.array(d32), expected=out.numpy())
            print(f"{kind:9s} {name:14s} x {x.shape} betas {rows.shape} -> {tuple(out.shape)}  max|xyz| {float(out.abs().max()):.3f}  "
                  f"restatement fp64 {d64:.2e}  fp32_dev {d32:.3e}  {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
