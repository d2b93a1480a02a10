"""Torch restatement of the reference's rot2xyz with a body shape PER FRAME: `Rotation2xyz_x.__call__` / `Rotation2xyz.__call__`
(model/rotation2xyz.py:158-324 / :11-155) handing a `betas` tensor with one row per frame to the body layer, whose shape blend then gives every
frame its own rest joints and its own v_shaped (smplx.lbs.lbs). tests/rot2xyz_ref.py and tests/rot2verts_ref.py restate the one-shape call; this
is the same arithmetic with the shape inside the batch, and it also takes what the reference's interface cannot express: a shape per PERSON.

    betas [B, P, T, nb]   fp32 values (nb <= the file's shape directions; the rest count as 0); rows of masked frames are never used

tests/test_rot2xyz_shaped_cpu.py pins the fp64 run to the goldens recorded from the reference's own wrappers (tests/golden/shaped_*.npz); the GPU
tests use the fp64 run as the truth and the fp32 run's deviation from it as the yardstick for the kernels. In fp32 the long sums run term by
term in index order, like tests/rot2verts_ref.py: shape terms, then pose terms, from v_template."""
import numpy as np
import torch

from tests.rot2verts_ref import ordered_sum
from tests.rot2xyz_ref import axis_angle_to_matrix, to_matrix


def expand_betas(betas, B, P, T):
    """[B, nb] | [B, P, nb] | [B, P, T, nb] -> numpy fp32 [B, P, T, nb]."""
    b = np.asarray(betas, dtype=np.float32)
    if b.ndim == 2:
        b = b[:, None, None, :]
    elif b.ndim == 3:
        b = b[:, :, None, :]
    return np.ascontiguousarray(np.broadcast_to(b, (B, P, T, b.shape[-1])))


def rows_to_frames(rows, mask, B, T, P):
    """The reference's betas [N_live, nb] (row n: the n-th unmasked frame in (b, t) order, the same for every person) -> [B, P, T, nb]."""
    rows = np.asarray(rows, dtype=np.float32)
    bt = np.zeros((B, T, rows.shape[1]), np.float32)
    bt[np.ones((B, T), bool) if mask is None else np.asarray(mask, bool)] = rows
    return np.ascontiguousarray(np.broadcast_to(bt[:, None], (B, P, T, rows.shape[1])))


def chain(rot, rest, parents):
    """rot [N, J, 3, 3], rest [N, J, 3] -> global rotations and positions, lists of J tensors [N, 3, 3] / [N, 3]."""
    grot, gpos = [rot[:, 0]], [rest[:, 0]]
    for i in range(1, rot.shape[1]):
        p = int(parents[i])
        gpos.append((grot[p] @ (rest[:, i] - rest[:, p])[:, :, None]).squeeze(-1) + gpos[p])
        grot.append(grot[p] @ rot[:, i])
    return grot, gpos


def shaped_ref(x, mask, body, betas, pose_rep, translation, glob, vertstrans, glob_rot=None, num_person=1, dtype=torch.float64, vertices=False,
               identity_joints=None):
    """x [B, R, C * P, T], betas [B, P, T, nb] -> joints [B, J, 3 * P, T] (joint 0 of the frame subtracted) or, with vertices, [B, V, 3 * P, T],
    in `dtype`. `body`: a skeleton dict (rest_joints, parents, shape_joints), with 'mesh' for vertices."""
    x = torch.as_tensor(x).to(dtype)
    parents = np.asarray(body["parents"]).reshape(-1)
    J = len(parents)
    B, _, F_, T = x.shape
    P = int(num_person)
    C = F_ // P
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)      # noqa: E731  (both runs start from the fp32 values)
    betas = np.asarray(betas, dtype=np.float32)
    assert betas.shape[:3] == (B, P, T), betas.shape
    nb = betas.shape[-1]
    rest0, sj = f32(body["rest_joints"]), f32(np.asarray(body["shape_joints"])[:, :, :nb])
    mask = torch.ones((B, T), dtype=torch.bool) if mask is None else torch.as_tensor(mask).bool()
    keep = mask.reshape(B * T)
    if vertices:
        mesh = body["mesh"]
        vt, sd, weights = f32(mesh["v_template"]), f32(mesh["shapedirs"][:, :, :nb]), f32(mesh["lbs_weights"])
        posedirs = None if mesh.get("posedirs", None) is None else f32(mesh["posedirs"])
        idj = mesh.get("identity_joints", ()) if identity_joints is None else identity_joints
        V = vt.shape[0]
    outs = []
    for p, xp in enumerate(torch.split(x, C, dim=2)):
        xt = xp[:, -1, :3] if translation else None
        xr = (xp[:, :-1] if translation else xp).permute(0, 3, 1, 2)
        rot = to_matrix(xr.reshape(B * T, xr.shape[2], C), pose_rep)
        if not glob:
            g = axis_angle_to_matrix(torch.tensor(np.asarray(glob_rot, dtype=np.float32))).to(dtype)
            rot = torch.cat([g.view(1, 1, 3, 3).expand(B * T, 1, 3, 3), rot], dim=1)
        if vertices and len(idj):
            rot = rot.clone()
            rot[:, [int(j) for j in idj]] = torch.eye(3, dtype=dtype)
        bt = torch.from_numpy(np.array(betas[:, p])).reshape(B * T, nb)
        bt = torch.where(keep[:, None], bt, torch.zeros_like(bt)).to(dtype)                  # a masked frame's betas are never looked at
        rest = ordered_sum([rest0[None].expand(B * T, J, 3)] + [bt[:, k, None, None] * sj[None, :, :, k] for k in range(nb)])
        grot, gpos = chain(rot, rest, parents)
        if not vertices:
            joints = torch.stack(gpos, dim=1).reshape(B, T, J, 3)
            xyz = torch.where(mask[:, :, None, None], joints, torch.zeros_like(joints)).permute(0, 2, 3, 1).contiguous()
            xyz = xyz - xyz[:, [0], :, :]
        else:
            N = B * T
            terms = [vt.reshape(1, 3 * V).expand(N, 3 * V)] + [bt[:, k:k + 1] * sd[:, :, k].reshape(1, 3 * V) for k in range(nb)]
            if posedirs is not None and J > 1:
                pf = (rot[:, 1:] - torch.eye(3, dtype=dtype)).reshape(N, 9 * (J - 1))
                terms += [pf[:, k:k + 1] * posedirs[k:k + 1] for k in range(pf.shape[1])]
            v_posed = ordered_sum(terms).reshape(N, V, 3)
            A = [torch.cat([grot[i], (gpos[i] - (grot[i] @ rest[:, i][:, :, None]).squeeze(-1))[:, :, None]], dim=2) for i in range(J)]
            Tm = ordered_sum([weights[None, :, j, None, None] * A[j][:, None] for j in range(J)])
            verts = (Tm[..., :3] @ v_posed[..., None]).squeeze(-1) + Tm[..., 3]
            verts = torch.where(keep[:, None, None], verts, torch.zeros_like(verts))
            xyz = verts.reshape(B, T, V, 3).permute(0, 2, 3, 1).contiguous()
        if translation and vertstrans:
            if P == 1:
                xt = xt - xt[:, :, [0]]
            xyz = xyz + xt[:, None, :, :]
        outs.append(xyz)
    return torch.cat(outs, 2)
