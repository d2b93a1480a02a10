"""Golden vectors of the reference's rot2xyz wrapper with the joint types its SMPL layer regresses from the mesh - 'vibe', 'a2m', 'a2mpl' -
recorded by RUNNING THE REFERENCE (CPU) in the build container.

    python tests/golden/make_golden_rot2joints.py

`Rotation2xyz.__call__` (model/rotation2xyz.py:17-155) and its `SMPL` class (model/smpl.py:66-98: the index maps, the extra-joint regression, the
selection) are run as they stand in fp64, through the harness of make_golden_rot2xyz.py / make_golden_rot2verts.py. Stand-ins cover only the
missing smplx package: the layer returns `vertices` from lbs64 (a shape per row: lbs64_rows of make_golden_rot2xyz_shaped.py) and
`joints = [chain joints | vertices[:, vertex_joints]]` as the smplx layer's vertex-joint selector appends them, `vertices2joints` is
einsum('bik,ji->bjk', vertices, J_regressor), and np.load of the regressor's path returns a SYNTHETIC J_regressor_extra
(regennet_amd.synth.make_joint_regressors). The body is SMPL-shaped - J = 24, V = 70, 21 vertex joints, 9 regressed - so that the reference's own
maps are valid indices.

Only DATA is written: tests/golden/rot2joints_<case>.npz with the input, mask, settings, make_body's and make_joint_regressors' arguments with a
sha256 / the arrays, THE THREE MAPS AND ROOT ROWS AS THE REFERENCE COMPUTED THEM (wrapper.smpl_model.maps, JOINTSTYPE_ROOT), the expected output
and `fp32_dev`: how far the fp32 run of tests/rot2joints_ref.py is from `expected`."""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_golden_rot2xyz as harness  # noqa: E402
from make_golden_rot2verts import lbs64  # noqa: E402
from make_golden_rot2xyz_shaped import lbs64_rows  # noqa: E402
from regennet_amd import synth  # noqa: E402

B, T = harness.B, harness.T
TYPES = ("vibe", "a2m", "a2mpl")


def posed(self, rot, betas):
    cls = type(self)
    joints, vertices = (lbs64_rows if cls.per_row else lbs64)(rot.double(), betas, cls.skeleton)
    picked = vertices[:, torch.as_tensor(cls.vertex_joints, dtype=torch.long)]
    return types.SimpleNamespace(joints=torch.cat([joints, picked], dim=1), vertices=vertices)


CASES = {
    # name: (jointstype, pose_rep, translation, glob, vertstrans, persons, mask, beta, glob_rot, betas per row)
    "vibe_p1": ("vibe", "rot6d", True, True, True, 1, None, 0, None, 0),
    "a2m_ragged": ("a2m", "rot6d", True, True, True, 1, harness.RAGGED, 0, None, 0),
    "a2mpl_p2_ragged": ("a2mpl", "rot6d", True, True, True, 2, harness.RAGGED, 0, None, 0),
    "vibe_beta": ("vibe", "rot6d", True, True, True, 1, harness.RAGGED, 1.5, None, 0),
    "a2m_noglob_rotvec": ("a2m", "rotvec", True, False, True, 1, harness.RAGGED, 0, [2.5, 0.5, -0.25], 0),
    "vibe_novertstrans": ("vibe", "rot6d", True, True, False, 1, harness.RAGGED, 0, None, 0),
    "vibe_frame_betas": ("vibe", "rot6d", True, True, True, 1, harness.RAGGED, 0, None, 10),         # betas: one row per unmasked frame
}


def main():
    from tests.rot2joints_ref import rot2joints_ref
    from tests.rot2verts_ref import body_sha256
    from tests.rot2xyz_shaped_ref import rows_to_frames
    harness._SkeletonLayer.posed = posed
    Rotation2xyz, _ = harness.reference_wrappers()
    import model.smpl as ref_smpl
    ref_smpl.vertices2joints = lambda reg, v: torch.einsum("bik,ji->bjk", v, reg.to(v.dtype))
    J, V = 24, 70
    args = dict(njoints=J, nverts=V, nbetas=10, seed=J)
    rargs = dict(npicks=21, nreg=9, support=6, seed=J)
    body = synth.make_body(**args)
    regs = synth.make_joint_regressors(body, **rargs)
    harness._SkeletonLayer.skeleton = body
    harness._SkeletonLayer.vertex_joints = regs["vertex_joints"]
    for n, (name, (jointstype, pose_rep, translation, glob, vertstrans, P, mask, beta, glob_rot, nrow)) in enumerate(CASES.items()):
        rng = np.random.Generator(np.random.PCG64(400 + n))
        x = harness.make_x(rng, J, pose_rep, translation, glob, P)
        n_live = B * T if mask is None else int(mask.sum())
        rows = rng.standard_normal((n_live, nrow)).astype(np.float32) if nrow else None
        harness._SkeletonLayer.per_row = rows is not None
        with mock.patch("numpy.load", lambda *a, **k: regs["J_regressor_extra"]):                 # J_regressor_extra (model/smpl.py:76)
            wrapper = Rotation2xyz("cpu")
        maps = {t: np.asarray(wrapper.smpl_model.maps[t], dtype=np.int32) for t in TYPES}
        roots = np.array([ref_smpl.JOINTSTYPE_ROOT[t] for t in TYPES], np.int32)
        assert all(0 <= m.min() and m.max() < J + 21 + 9 for m in maps.values())
        m = None if mask is None else torch.from_numpy(mask)
        x_ref = x
        if not glob:        # Rotation2xyz (:117-123) takes global_orient from glob_rot and STILL drops the first rotation row: the reference is handed
            x_ref = np.concatenate([rng.standard_normal(x[:, :1].shape).astype(np.float32), x], axis=1)     # one more row, which it discards unread
        out = wrapper(torch.from_numpy(x_ref).double(), m, pose_rep=pose_rep, translation=translation, glob=glob, jointstype=jointstype, vertstrans=vertstrans,
                      betas=None if rows is None else torch.from_numpy(rows).double(), beta=beta, glob_rot=glob_rot, num_person=P)
        assert out.dtype == torch.float64 and tuple(out.shape) == (B, len(maps[jointstype]), 3 * P, T), (out.dtype, out.shape)
        kw = dict(pose_rep=pose_rep, translation=translation, glob=glob, vertstrans=vertstrans, beta=beta, glob_rot=glob_rot, num_person=P,
                  frame_betas=None if rows is None else rows_to_frames(rows, mask, B, T, P))
        root = int(roots[TYPES.index(jointstype)])
        d64 = float((rot2joints_ref(x, m, body, regs, maps[jointstype], root, dtype=torch.float64, **kw) - out).abs().max())
        d32 = float((rot2joints_ref(x, m, body, regs, maps[jointstype], root, dtype=torch.float32, **kw).double() - out).abs().max())
        path = os.path.join(HERE, f"rot2joints_{name}.npz")
        np.savez_compressed(path, x=x, mask=np.ones((B, T), bool) if mask is None else mask, mask_none=np.array(mask is None),
                            betas=np.zeros((0, 0), np.float32) if rows is None else rows,
                            body_args=np.array([args[k] for k in ("njoints", "nverts", "nbetas", "seed")]), body_sha256=np.array(body_sha256(body)),
                            regs_args=np.array([rargs[k] for k in ("npicks", "nreg", "support", "seed")]), vertex_joints=regs["vertex_joints"],
                            J_regressor_extra=regs["J_regressor_extra"], map_vibe=maps["vibe"], map_a2m=maps["a2m"], map_a2mpl=maps["a2mpl"],
                            map_roots=roots, jointstype=np.array(jointstype), pose_rep=np.array(pose_rep), translation=np.array(translation),
                            glob=np.array(glob), vertstrans=np.array(vertstrans), num_person=np.array(P), beta=np.array(float(beta)),
                            glob_rot=np.zeros(3, np.float32) if glob_rot is None else np.array(glob_rot, np.float32), fp32_dev=np.array(d32),
                            expected=out.numpy())
        print(f"{name:18s} x {x.shape} -> {tuple(out.shape)}  max|xyz| {float(out.abs().max()):.3f}  restatement fp64 {d64:.2e}  fp32_dev {d32:.3e}  "
              f"{os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
