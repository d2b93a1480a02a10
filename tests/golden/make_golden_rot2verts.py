"""Golden vectors of the reference's rot2xyz wrappers with jointstype='vertices', recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_rot2verts.py

`Rotation2xyz_x.__call__` and `Rotation2xyz.__call__` (model/rotation2xyz.py:158-324 / :11-155) are run as they stand, through the harness of
make_golden_rot2xyz.py: the row split per person, the rotation conversions, which rotations are handed to the layer (not the jaw's and the eyes',
:294-301), masking, the absent root subtraction and the translation term are the reference's own code. The body layer they call (`smplx`, with
licensed model files) is absent; the stand-in's `forward` here also returns `vertices`: linear blend skinning in fp64 over a SYNTHETIC body
(regennet_amd.synth.make_body), written the way smplx.lbs.lbs is - homogeneous 4x4 transforms, one matmul per sum - from arrays rounded to fp32
like the real layer's buffers. The wrappers are fed x in fp64, so `expected` is fp64 throughout.

Only DATA is written: tests/golden/rot2verts_<case>.npz with the input, mask, settings, make_body's arguments with a sha256 of its arrays, the
expected output, and `fp32_dev`: how far the fp32 run of tests/rot2verts_ref.py is from `expected` (printed; tests/test_rot2verts_cpu.py holds
the restatement to it)."""
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


def lbs64(rot, betas, body):
    """rot [N, J, 3, 3] fp64, betas [N, nb] -> (joints [N, J, 3], vertices [N, V, 3]), after smplx.lbs.lbs."""
    mesh = body["mesh"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).astype(np.float64))      # noqa: E731
    b = betas.double()
    assert bool((b == b[:1]).all())
    N, J = rot.shape[:2]
    parents = body["parents"]
    v_shaped = d(mesh["v_template"])[None] + torch.einsum("bl,mkl->bmk", d(b.numpy()), d(mesh["shapedirs"]))
    rest = body["rest_joints"].astype(np.float64) + body["shape_joints"].astype(np.float64) @ b[0].numpy()       # (= J_regressor @ v_shaped for a body file)
    rest = d(rest)[None].expand(N, J, 3)
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
    joints, vertices = lbs64(rot.double(), betas, type(self).skeleton)
    joints = torch.cat([joints, torch.zeros(joints.shape[0], type(self).pad_to - joints.shape[1], 3, dtype=joints.dtype)], dim=1)
    return types.SimpleNamespace(joints=joints, vertices=vertices)


CASES = {
    # name: (joints, vertices, pose_rep, translation, glob, vertstrans, persons, mask, beta, glob_rot)
    "p1": (55, 130, "rot6d", True, True, True, 1, None, 0, None),                       # (rows 22 - 24 of x are random like every other row)
    "p2_ragged": (55, 130, "rot6d", True, True, True, 2, harness.RAGGED, 0, None),
    "smpl24": (24, 70, "rot6d", True, True, True, 1, harness.RAGGED, 0, None),
    "beta": (55, 130, "rot6d", True, True, True, 1, harness.RAGGED, 1.5, None),
    "noglob_rotvec": (55, 130, "rotvec", True, False, True, 1, harness.RAGGED, 0, [2.5, 0.5, -0.25]),
    "novertstrans": (55, 130, "rot6d", True, True, False, 1, harness.RAGGED, 0, None),
}


def main():
    from tests.rot2verts_ref import body_sha256, rot2verts_ref
    harness._SkeletonLayer.posed = posed
    Rotation2xyz, Rotation2xyz_x = harness.reference_wrappers()
    for n, (name, (J, V, pose_rep, translation, glob, vertstrans, P, mask, beta, glob_rot)) in enumerate(CASES.items()):
        args = dict(njoints=J, nverts=V, nbetas=10, seed=J)
        body = synth.make_body(**args)
        assert list(body["mesh"]["identity_joints"]) == ([22, 23, 24] if J == 55 else [])
        harness._SkeletonLayer.skeleton = body
        rng = np.random.Generator(np.random.PCG64(200 + n))
        x = harness.make_x(rng, J, pose_rep, translation, glob, P)
        with mock.patch("numpy.load", lambda *a, **k: np.zeros((9, 1), np.float32)):       # J_regressor_extra (model/smpl.py:76), unused by 'vertices'
            wrapper = (Rotation2xyz_x if J == 55 else Rotation2xyz)("cpu")
        out = wrapper(torch.from_numpy(x).double(), None if mask is None else torch.from_numpy(mask), pose_rep=pose_rep, translation=translation,
                      glob=glob, jointstype="vertices", vertstrans=vertstrans, betas=None, beta=beta, glob_rot=glob_rot, num_person=P)
        assert out.dtype == torch.float64 and tuple(out.shape) == (B, V, 3 * P, T), (out.dtype, out.shape)
        kw = dict(pose_rep=pose_rep, translation=translation, glob=glob, vertstrans=vertstrans, beta=beta, glob_rot=glob_rot, num_person=P)
        m = None if mask is None else torch.from_numpy(mask)
        d64 = float((rot2verts_ref(x, m, body, dtype=torch.float64, **kw) - out).abs().max())
        d32 = float((rot2verts_ref(x, m, body, dtype=torch.float32, **kw).double() - out).abs().max())
        path = os.path.join(HERE, f"rot2verts_{name}.npz")
        np.savez_compressed(path, x=x, mask=np.ones((B, T), bool) if mask is None else mask, mask_none=np.array(mask is None),
                            body_args=np.array([args[k] for k in ("njoints", "nverts", "nbetas", "seed")]), body_sha256=np.array(body_sha256(body)),
                            pose_rep=np.array(pose_rep), translation=np.array(translation), glob=np.array(glob), vertstrans=np.array(vertstrans),
                            num_person=np.array(P), beta=np.array(float(beta)),
                            glob_rot=np.zeros(3, np.float32) if glob_rot is None else np.array(glob_rot, np.float32), fp32_dev=np.array(d32), expected=out.numpy())
        print(f"{name:14s} x {x.shape} -> {tuple(out.shape)}  max|xyz| {float(out.abs().max()):.3f}  restatement fp64 {d64:.2e}  fp32_dev {d32:.3e}  {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
