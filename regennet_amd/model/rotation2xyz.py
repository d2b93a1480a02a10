"""Joint positions from rotations — counterpart of the reference's `model/rotation2xyz.py` (`Rotation2xyz`, `Rotation2xyz_x`) for the joint
types that are the body model's own skeleton joints ('smplx': 55, 'smpl': 24).

Those joints are the translation parts of linear blend skinning's rigid-transform chain: they depend on the rest joint positions, the parent
table and the rotations, not on vertices, pose blend shapes or skinning weights. So the body model is replaced by a SKELETON FILE, an npz with

    rest_joints   [J, 3]      J_regressor @ v_template
    parents       [J]         kintree_table[0], root = -1, parents[i] < i
    shape_joints  [J, 3, nb]  optional: J_regressor @ shapedirs[:, :, k], for betas / beta
    body_model    str         optional label

which tools/make_skeleton.py writes from a model file the user has licensed (`synth.make_skeleton` gives a synthetic one). The chain itself runs
on the device (rgn_rot2xyz, csrc/rgn_fk.hip) straight from the sampler's [B, rows, feats, T] layout; there is no CPU path."""
import numpy as np
import torch

from .. import _lib
from ..utils import dist_util

JOINTSTYPES = ["a2m", "a2mpl", "smpl", "vibe", "smplx", "vertices"]     # rotation2xyz.py:8
SKELETON_JOINTSTYPES = ("smpl", "smplx")                                  # ... of which these are the skeleton's own joints (model/smpl.py:80,108)


def check_skeleton(sk):
    """Normalise dtypes and validate a skeleton dict (the checks rgn_rot2xyz makes, made where the file is read)."""
    rest = np.ascontiguousarray(sk["rest_joints"], dtype=np.float64)
    parents = np.ascontiguousarray(sk["parents"], dtype=np.int64).reshape(-1)
    J = len(parents)
    if rest.shape != (J, 3) or not 1 <= J <= 64:
        raise ValueError(f"skeleton: rest_joints {rest.shape} / parents {parents.shape}: need [J, 3] and [J] with 1 <= J <= 64")
    if parents[0] != -1 or any(not 0 <= parents[i] < i for i in range(1, J)):
        raise ValueError("skeleton: parents[0] must be -1 and 0 <= parents[i] < i for every other joint")
    out = {"rest_joints": rest, "parents": parents.astype(np.int32), "shape_joints": None, "body_model": str(sk.get("body_model", ""))}
    if sk.get("shape_joints", None) is not None:
        sj = np.ascontiguousarray(sk["shape_joints"], dtype=np.float64)
        if sj.ndim != 3 or sj.shape[:2] != (J, 3):
            raise ValueError(f"skeleton: shape_joints {sj.shape} is not [J, 3, nb]")
        out["shape_joints"] = sj
    return out


def load_skeleton(path):
    """Read a skeleton npz (module docstring) -> dict(rest_joints fp64 [J,3], parents int32 [J], shape_joints fp64 [J,3,nb] | None, body_model)."""
    with np.load(path, allow_pickle=False) as z:
        sk = {k: z[k] for k in ("rest_joints", "parents")}
        sk["shape_joints"] = z["shape_joints"] if "shape_joints" in z.files else None
        sk["body_model"] = str(z["body_model"]) if "body_model" in z.files else ""
    return check_skeleton(sk)


class Rotation2xyz:
    """`Rotation2xyz(skeleton, model)(x, mask, pose_rep, translation, glob, jointstype, vertstrans, ...)` with the keyword arguments of both
    reference classes; unknown extras are accepted and ignored as on `Rotation2xyz_x`. `model` is the CMDM whose engine runs the kernel."""

    def __init__(self, skeleton, model=None):
        self.skeleton = check_skeleton(skeleton)
        self.model = model
        self.smpl_model = None          # (the reference keeps its body layer here; there is none)
        sj = self.skeleton["shape_joints"]
        self.num_betas = 10 if sj is None else int(sj.shape[2])

    def rest_joints(self, betas=None, beta=0):
        """rest + sum_k betas[k] * shape_joints[:, :, k], formed per call on the host; betas None -> zeros with betas[1] = beta (:289-292)."""
        sk = self.skeleton
        if betas is None:
            b = np.zeros(self.num_betas)
            if beta != 0:
                b[1] = float(beta)
        else:
            b = (betas.detach().cpu().numpy() if isinstance(betas, torch.Tensor) else np.asarray(betas)).astype(np.float64)
            if b.ndim == 2:
                if (b != b[:1]).any():
                    raise NotImplementedError("per-row betas: every row of `betas` must be the same shape (one rest skeleton per call)")
                b = b[0]
            if b.ndim != 1:
                raise ValueError(f"betas {b.shape}: expected [nb] or [N, nb]")
        if not b.any():
            return sk["rest_joints"]
        if sk["shape_joints"] is None:
            raise ValueError("non-zero betas / beta need `shape_joints` in the skeleton file")
        if len(b) > sk["shape_joints"].shape[2]:
            raise ValueError(f"{len(b)} betas but the skeleton file holds {sk['shape_joints'].shape[2]} shape directions")
        return sk["rest_joints"] + sk["shape_joints"][:, :, :len(b)] @ b

    def __call__(self, x, mask, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0, glob_rot=None, num_person=1,
                 get_rotations_back=False, **kwargs):
        if pose_rep == "xyz":
            return x
        if not glob and glob_rot is None:
            raise TypeError("You must specify global rotation if glob is False")
        if jointstype not in JOINTSTYPES:
            raise NotImplementedError("This jointstype is not implemented.")
        if jointstype not in SKELETON_JOINTSTYPES:
            raise NotImplementedError(
                f"jointstype={jointstype!r} is computed from the body model's vertices, which a skeleton file does not hold: "
                f"only {SKELETON_JOINTSTYPES} (the skeleton's own joints) are served")
        if pose_rep not in _lib.POSE_REP:
            raise NotImplementedError("No geometry for this one.")
        if self.model is None:
            raise RuntimeError("Rotation2xyz runs on a model's HIP engine: build it as Rotation2xyz(skeleton, model) or use model.set_skeleton()")
        P, C = int(num_person), _lib.POSE_REP_CHANNELS[pose_rep]
        J = len(self.skeleton["parents"])
        B, R, F, T = x.shape
        want = (J if glob else J - 1) + (1 if translation else 0)
        if (R, F) != (want, C * P):
            raise ValueError(f"x {tuple(x.shape)}: a {J}-joint skeleton with pose_rep={pose_rep!r}, glob={bool(glob)}, translation={bool(translation)}, "
                             f"num_person={P} takes [B, {want}, {C * P}, T]")
        model = self.model
        eng = model._engine if (model._engine is not None and not model._engine_stale) else model._get_engine(B, T)[0]
        dev = next(model.parameters()).device
        xc = x.to(device=dev, dtype=torch.float32).contiguous()
        mc = None if mask is None else mask.to(device=dev).reshape(B, T).bool().contiguous()
        out = torch.empty((B, J, 3 * P, T), device=dev, dtype=torch.float32)
        rot = torch.empty((B, P, T, J, 3, 3), device=dev, dtype=torch.float32) if get_rotations_back else None
        flags = (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)
        gr = None if glob else np.asarray(glob_rot, dtype=np.float32).reshape(3)
        eng.rot2xyz(xc, mc, self.rest_joints(betas, beta), self.skeleton["parents"], _lib.POSE_REP[pose_rep], P, flags, gr, out, rot,
                    dist_util.stream_handle(dev))
        out = out.to(x.device)
        if get_rotations_back:      # Rotation2xyz (:152-153): the last person's matrices of the unmasked frames, without and with joint 0
            r = rot[:, -1] if mc is None else rot[:, -1][mc]
            r = r.reshape(-1, J, 3, 3)
            return out, r[:, 1:], r[:, 0]
        return out
