"""Torch restatement of the reference's rot2xyz with jointstype='vertices': `Rotation2xyz_x.__call__` / `Rotation2xyz.__call__`
(model/rotation2xyz.py:303-321 / :236-249) around linear blend skinning as the body layer they call computes it (smplx.lbs.lbs: shape blend,
pose blend shapes, the rigid-transform chain, the blend of the joints' transforms). Runs in fp64 or fp32, on any device.

tests/test_rot2verts_cpu.py pins it to the goldens recorded from the reference's own wrappers (tests/golden/rot2verts_*.npz); the GPU tests use the
fp64 run as the truth and the fp32 run's deviation from it as the yardstick for the kernel. In fp32 the two long sums (pose blend over 9 (J - 1)
terms, blend of transforms over J) are accumulated one term after the other in index order - the order class of the fp32-input MFMA the kernel
runs them on - so that the yardstick is the arithmetic's own error and not a property of a blocked matmul."""
import hashlib

import numpy as np
import torch

from tests.rot2xyz_ref import axis_angle_to_matrix, rest_with_betas, to_matrix


def betas_vector(mesh, betas=None, beta=0):
    sd = mesh.get("shapedirs", None)
    if betas is None:
        betas = np.zeros(10 if sd is None else sd.shape[2])
        if beta != 0:
            betas[1] = beta
    return np.asarray(betas, dtype=np.float64)


def ordered_sum(terms):
    """sum_k terms(k), left to right."""
    acc = None
    for t in terms:
        acc = t if acc is None else acc + t
    return acc


def lbs_vertices(rot, rest, parents, v_shaped, posedirs, weights, ordered):
    """rot [N, J, 3, 3] (identity joints already replaced), rest [J, 3], v_shaped [V, 3], posedirs [9 (J - 1), 3 V] | None, weights [V, J] -> [N, V, 3]."""
    N, J = rot.shape[:2]
    V = v_shaped.shape[0]
    dt = rot.dtype
    v_posed = v_shaped.reshape(1, 3 * V).expand(N, 3 * V)
    if posedirs is not None and J > 1:
        pf = (rot[:, 1:] - torch.eye(3, dtype=dt, device=rot.device)).reshape(N, 9 * (J - 1))
        if not ordered:
            v_posed = v_posed + pf @ posedirs
        else:
            v_posed = ordered_sum([v_posed] + [pf[:, k:k + 1] * posedirs[k:k + 1] for k in range(pf.shape[1])])
    v_posed = v_posed.reshape(N, V, 3)
    grot, gpos = [rot[:, 0]], [rest[0].expand(N, 3)]                # the chain: G_0 = [R_0 | j_0], G_i = G_parent(i) . [R_i | j_i - j_parent(i)]
    for i in range(1, J):
        p = int(parents[i])
        gpos.append((grot[p] @ (rest[i] - rest[p])[:, None]).squeeze(-1) + gpos[p])
        grot.append(grot[p] @ rot[:, i])
    A = [torch.cat([grot[i], (gpos[i] - (grot[i] @ rest[i][:, None]).squeeze(-1))[:, :, None]], dim=2) for i in range(J)]       # [N, 3, 4] each
    if not ordered:
        Tm = torch.einsum("vj,njrc->nvrc", weights, torch.stack(A, dim=1))
    else:
        Tm = ordered_sum([weights[None, :, j, None, None] * A[j][:, None] for j in range(J)])
    return (Tm[..., :3] @ v_posed[..., None]).squeeze(-1) + Tm[..., 3]


def rot2verts_ref(x, mask, body, pose_rep, translation, glob, vertstrans, betas=None, beta=0, glob_rot=None, num_person=1, dtype=torch.float64,
                  identity_joints=None, ordered=None):
    """x [B, R, C * P, T] -> [B, V, 3 * P, T] in `dtype`, on x's device. `body`: dict(rest_joints, parents, shape_joints, mesh=dict(...)) as
    check_body / synth.make_body give it; identity_joints overrides the body's; ordered (default: in fp32) runs the two long sums term by term."""
    ordered = dtype != torch.float64 if ordered is None else ordered
    x = torch.as_tensor(x).to(dtype)
    dev = x.device
    mesh = body["mesh"]
    parents = np.asarray(body["parents"]).reshape(-1)
    J = len(parents)

    def f32(a):                                                  # the kernel's inputs are fp32, like the reference layer's buffers: both runs start from those values
        if isinstance(a, torch.Tensor):                          # (mesh arrays already on the device, for timing)
            return a.to(device=dev, dtype=torch.float32).to(dtype)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device=dev, dtype=dtype)

    b = betas_vector(mesh, betas, beta)
    rest = f32(rest_with_betas(body, b))
    v_shaped = f32(mesh["v_template"])
    if b.any():
        sd, bt = f32(mesh["shapedirs"]), f32(b)
        v_shaped = ordered_sum([v_shaped] + [bt[k] * sd[:, :, k] for k in range(len(b))])
    posedirs = None if mesh.get("posedirs", None) is None else f32(mesh["posedirs"])
    weights = f32(mesh["lbs_weights"])
    idj = mesh.get("identity_joints", ()) if identity_joints is None else identity_joints
    B, _, F_, T = x.shape
    if mask is None:
        mask = torch.ones((B, T), dtype=torch.bool, device=dev)
    mask = torch.as_tensor(mask).to(dev).bool()
    P = int(num_person)
    C = F_ // P
    outs = []
    for xp in torch.split(x, C, dim=2):
        xt = xp[:, -1, :3] if translation else None              # [B, 3, T]
        xr = (xp[:, :-1] if translation else xp).permute(0, 3, 1, 2)
        rot = to_matrix(xr.reshape(B * T, xr.shape[2], C), pose_rep)
        if not glob:
            g = axis_angle_to_matrix(torch.tensor(np.asarray(glob_rot, dtype=np.float32))).to(device=dev, dtype=dtype)
            rot = torch.cat([g.view(1, 1, 3, 3).expand(B * T, 1, 3, 3), rot], dim=1)
        if len(idj):
            rot = rot.clone()
            rot[:, [int(j) for j in idj]] = torch.eye(3, dtype=dtype, device=dev)
        keep = mask.reshape(B * T)
        verts = torch.zeros(B * T, weights.shape[0], 3, dtype=dtype, device=dev)       # frames with mask == 0 are 0 (and cost nothing)
        if bool(keep.any()):
            verts[keep] = lbs_vertices(rot[keep], rest, parents, v_shaped, posedirs, weights, ordered)
        xyz = verts.reshape(B, T, -1, 3).permute(0, 2, 3, 1).contiguous()               # no root subtraction for vertices
        if translation and vertstrans:
            if P == 1:
                xt = xt - xt[:, :, [0]]
            xyz = xyz + xt[:, None, :, :]
        outs.append(xyz)
    return torch.cat(outs, 2)


def body_sha256(body):
    """Digest of a body's arrays: the goldens name their synthetic body by synth.make_body's arguments and this."""
    h = hashlib.sha256()
    for a in (body["rest_joints"], body["parents"], body["shape_joints"],
              *(body["mesh"][k] for k in ("v_template", "posedirs", "lbs_weights", "shapedirs", "faces", "identity_joints"))):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def golden_body(g):
    """The synthetic body a golden was recorded over, rebuilt and checked against the recorded digest."""
    from regennet_amd import synth
    J, V, nb, seed = (int(v) for v in g["body_args"])
    body = synth.make_body(njoints=J, nverts=V, nbetas=nb, seed=seed)
    assert body_sha256(body) == str(g["body_sha256"]), "synth.make_body no longer gives the body this golden was recorded over"
    return body


def golden_settings(g):
    return dict(pose_rep=str(g["pose_rep"]), translation=bool(g["translation"]), glob=bool(g["glob"]), vertstrans=bool(g["vertstrans"]),
                beta=float(g["beta"]), glob_rot=None if bool(g["glob"]) else g["glob_rot"], num_person=int(g["num_person"]))
