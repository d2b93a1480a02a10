"""Torch restatement of the reference's rot2xyz for the joint types its SMPL layer regresses from the mesh - 'vibe', 'a2m', 'a2mpl':
`Rotation2xyz.__call__` (model/rotation2xyz.py:17-155) around `SMPL.forward` (model/smpl.py:88-98),

    all_joints = [ J chain joints | vertices[:, vertex_joints] | einsum('bik,ji->bjk', vertices, J_regressor_extra) ],   out = all_joints[:, map]

with frames of mask == 0 set to 0, output row `root` subtracted and the translation row added. Built on tests/rot2verts_ref.py (the one-shape call:
rest joints formed in fp64 on the host and rounded, v_shaped first) and tests/rot2xyz_shaped_ref.py (betas [B, P, T, nb]: rest joints and shape
terms per frame, summed in fp32 on the device); the arithmetic of a vertex is theirs. Runs in fp64 or fp32.

tests/test_rot2joints_cpu.py pins the fp64 run to goldens recorded from the reference's own classes (tests/golden/rot2joints_*.npz); the GPU tests
take the fp64 run as the truth and the fp32 run's deviation from it as the yardstick. In fp32 the long sums run term by term in index order - the
order class of the fp32-input MFMA - and so does the regression, over the vertices that carry a weight, ascending. Only the vertices the joints
touch are skinned here too: a vertex does not depend on the others."""
import hashlib

import numpy as np
import torch

from tests.rot2verts_ref import betas_vector, ordered_sum
from tests.rot2xyz_ref import axis_angle_to_matrix, rest_with_betas, to_matrix
from tests.rot2xyz_shaped_ref import chain


def touched(regs, V):
    """The vertices the joints touch, ascending: the picks united with the regressor's non-zero columns (the kernel's S)."""
    used = np.zeros(V, bool)
    used[np.asarray(regs["vertex_joints"], dtype=np.int64)] = True
    reg = np.asarray(regs["J_regressor_extra"], dtype=np.float32).reshape(-1, V)
    used |= (reg != 0).any(0)
    return np.flatnonzero(used)


def rot2joints_ref(x, mask, body, regs, jmap, root, pose_rep, translation, glob, vertstrans, betas=None, beta=0, glob_rot=None, num_person=1,
                   dtype=torch.float64, frame_betas=None, ordered=None, return_all=False):
    """x [B, R, C * P, T] -> [B, len(jmap), 3 * P, T] in `dtype`. body: as check_body / synth.make_body give it; regs: dict(vertex_joints [Np],
    J_regressor_extra [Jr, V]); jmap: indices into all_joints; root: the output row that is subtracted. betas / beta: the one shape of the call;
    frame_betas [B, P, T, nb]: a shape per frame instead. return_all: all_joints [B, J + Np + Jr, 3 * P, T] masked, nothing subtracted or added."""
    ordered = dtype != torch.float64 if ordered is None else ordered
    x = torch.as_tensor(x).to(dtype)
    mesh = body["mesh"]
    parents = np.asarray(body["parents"]).reshape(-1)
    J, V = len(parents), mesh["v_template"].shape[0]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)       # noqa: E731  (both runs start from the fp32 values)
    S = touched(regs, V)
    nS = len(S)
    at = {int(v): i for i, v in enumerate(S)}
    picks = [at[int(v)] for v in np.asarray(regs["vertex_joints"]).reshape(-1)]
    reg = f32(np.asarray(regs["J_regressor_extra"], dtype=np.float32).reshape(-1, V)[:, S])      # [Jr, nS]
    vt, weights = f32(mesh["v_template"][S]), f32(mesh["lbs_weights"][S])
    posedirs = None if mesh.get("posedirs", None) is None or J == 1 else f32(np.asarray(mesh["posedirs"]).reshape(-1, V, 3)[:, S].reshape(-1, 3 * nS))
    idj = mesh.get("identity_joints", ())
    B, _, F_, T = x.shape
    P = int(num_person)
    C = F_ // P
    N = B * T
    mask = torch.ones((B, T), dtype=torch.bool) if mask is None else torch.as_tensor(mask).bool()
    keep = mask.reshape(N)
    if frame_betas is None:
        b = betas_vector(mesh, betas, beta)
        rest1 = f32(rest_with_betas(body, b))
        v1 = vt
        if b.any():
            sd, bt1 = f32(mesh["shapedirs"][S]), f32(b)
            v1 = ordered_sum([vt] + [bt1[k] * sd[:, :, k] for k in range(len(b))])
    else:
        frame_betas = np.asarray(frame_betas, dtype=np.float32)
        assert frame_betas.shape[:3] == (B, P, T), frame_betas.shape
        nb = frame_betas.shape[-1]
        rest0, sj, sd = f32(body["rest_joints"]), f32(np.asarray(body["shape_joints"])[:, :, :nb]), f32(mesh["shapedirs"][S][:, :, :nb])
    outs = []
    for p, xp in enumerate(torch.split(x, C, dim=2)):
        xt = xp[:, -1, :3] if translation else None
        xr = (xp[:, :-1] if translation else xp).permute(0, 3, 1, 2)
        rot = to_matrix(xr.reshape(N, xr.shape[2], C), pose_rep)
        if not glob:
            g = axis_angle_to_matrix(torch.tensor(np.asarray(glob_rot, dtype=np.float32))).to(dtype)
            rot = torch.cat([g.view(1, 1, 3, 3).expand(N, 1, 3, 3), rot], dim=1)
        if len(idj):
            rot = rot.clone()
            rot[:, [int(j) for j in idj]] = torch.eye(3, dtype=dtype)
        rot = torch.where(keep[:, None, None, None], rot, torch.eye(3, dtype=dtype).expand_as(rot))      # masked frames: any finite value, zeroed below
        if frame_betas is None:
            rest, terms = rest1[None].expand(N, J, 3), [v1.reshape(1, 3 * nS).expand(N, 3 * nS)]
        else:
            bt = torch.from_numpy(np.array(frame_betas[:, p])).reshape(N, nb)
            bt = torch.where(keep[:, None], bt, torch.zeros_like(bt)).to(dtype)                          # a masked frame's betas are never looked at
            rest = ordered_sum([rest0[None].expand(N, J, 3)] + [bt[:, k, None, None] * sj[None, :, :, k] for k in range(nb)])
            terms = [vt.reshape(1, 3 * nS).expand(N, 3 * nS)] + [bt[:, k:k + 1] * sd[:, :, k].reshape(1, 3 * nS) for k in range(nb)]
        grot, gpos = chain(rot, rest, parents)
        if posedirs is not None:
            pf = (rot[:, 1:] - torch.eye(3, dtype=dtype)).reshape(N, 9 * (J - 1))
            if ordered:
                terms = terms + [pf[:, k:k + 1] * posedirs[k:k + 1] for k in range(pf.shape[1])]
            else:
                terms = terms + [pf @ posedirs]
        v_posed = ordered_sum(terms).reshape(N, nS, 3)
        A = [torch.cat([grot[i], (gpos[i] - (grot[i] @ rest[:, i][:, :, None]).squeeze(-1))[:, :, None]], dim=2) for i in range(J)]
        Tm = ordered_sum([weights[None, :, j, None, None] * A[j][:, None] for j in range(J)])
        verts = (Tm[..., :3] @ v_posed[..., None]).squeeze(-1) + Tm[..., 3]                               # [N, nS, 3]
        if ordered:
            extra = torch.zeros(N, reg.shape[0], 3, dtype=dtype) if nS == 0 else ordered_sum([reg[None, :, s, None] * verts[:, None, s] for s in range(nS)])
        else:
            extra = torch.einsum("bik,ji->bjk", verts, reg)
        joints = torch.cat([torch.stack(gpos, dim=1), verts[:, picks], extra], dim=1)                     # all_joints [N, J + Np + Jr, 3]
        joints = torch.where(keep[:, None, None], joints, torch.zeros_like(joints)).reshape(B, T, -1, 3).permute(0, 2, 3, 1).contiguous()
        if not return_all:
            joints = joints[:, torch.as_tensor(np.asarray(jmap), dtype=torch.long)]
            joints = joints - joints[:, [int(root)]]
            if translation and vertstrans:
                if P == 1:
                    xt = xt - xt[:, :, [0]]
                joints = joints + xt[:, None, :, :]
        outs.append(joints)
    return torch.cat(outs, 2)


def regs_sha256(regs):
    """Digest of the regressor arrays and maps: the goldens name theirs by synth.make_joint_regressors' arguments and this."""
    h = hashlib.sha256()
    for a in (regs["vertex_joints"], regs["J_regressor_extra"], *(regs["joint_maps"][t] for t in ("vibe", "a2m", "a2mpl"))):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def golden_regs(g, body):
    """The synthetic regressors a golden was recorded over, rebuilt and checked against the recorded arrays; the maps are THE RECORDED ones (the
    reference's own, `SMPL().maps`), not the synthetic ones."""
    from regennet_amd import synth
    npicks, nreg, support, seed = (int(v) for v in g["regs_args"])
    regs = synth.make_joint_regressors(body, npicks=npicks, nreg=nreg, support=support, seed=seed)
    assert np.array_equal(regs["vertex_joints"], g["vertex_joints"]) and np.array_equal(regs["J_regressor_extra"], g["J_regressor_extra"]), \
        "synth.make_joint_regressors no longer gives the arrays this golden was recorded over"
    return dict(regs, joint_maps={t: np.asarray(g["map_" + t], dtype=np.int32) for t in ("vibe", "a2m", "a2mpl")},
                map_roots={t: int(r) for t, r in zip(("vibe", "a2m", "a2mpl"), g["map_roots"])})
