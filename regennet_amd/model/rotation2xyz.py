"""Joint positions from rotations — counterpart of the reference's `model/rotation2xyz.py` (`Rotation2xyz`, `Rotation2xyz_x`) for the joint
types that are the body model's own skeleton joints ('smplx': 55, 'smpl': 24).

Those joints are the translation parts of linear blend skinning's rigid-transform chain: they depend on the rest joint positions, the parent
table and the rotations, not on vertices, pose blend shapes or skinning weights. So the body model is replaced by a SKELETON FILE, an npz with

    rest_joints   [J, 3]      J_regressor @ v_template
    parents       [J]         kintree_table[0], root = -1, parents[i] < i
    shape_joints  [J, 3, nb]  optional: J_regressor @ shapedirs[:, :, k], for betas / beta
    body_model    str         optional label

which tools/make_skeleton.py writes from a model file the user has licensed (`synth.make_skeleton` gives a synthetic one). The chain itself runs
on the device (rgn_rot2xyz, csrc/rgn_fk.hip) straight from the sampler's [B, rows, feats, T] layout; there is no CPU path.

jointstype='vertices' needs the body model's surface: a BODY FILE is a skeleton file with the mesh arrays beside it (`make_skeleton.py --mesh`;
`synth.make_body` gives a synthetic one),

    v_template       [V, 3]
    posedirs         [9 (J - 1), 3 V]   optional: pose blend shapes, the layout smplx.lbs.lbs multiplies with
    lbs_weights      [V, J]
    shapedirs        [V, 3, nb]         optional; shape_joints = J_regressor @ shapedirs keeps joints and surface consistent
    faces            [F, 3] int32       optional, for writing meshes
    identity_joints  [n]                joints whose rotation the reference's wrapper does not hand to the layer (SMPL-X: 22, 23, 24)

and linear blend skinning runs on the device too (rgn_rot2verts, csrc/rgn_lbs.hip).

The joint types the reference's SMPL layer regresses from the mesh - 'vibe', 'a2m', 'a2mpl' (model/smpl.py:76-98) - are index maps into
[J skeleton joints | Np vertex joints | Jr regressed joints]. A body file may hold what they need (`make_skeleton.py --mesh --vertex_joints
--joint_regressor_extra --joint_maps`; `synth.make_joint_regressors` gives synthetic ones),

    vertex_joints      [Np] int32      vertex ids in [0, V): vertices[:, ids] are joints
    J_regressor_extra  [Jr, V]         finite; Np + Jr <= 32, not both 0
    map_vibe, map_a2m, map_a2mpl       int32, 1 - 64 entries in [0, J + Np + Jr); any subset; DATA of the file, not constants of this package
    map_roots          [3]             optional: the output row that is subtracted, default 8, 0, 0

and those joints come from the device as well, skinned over the touched vertices only (rgn_rot2joints)."""
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


MESH_KEYS = ("v_template", "posedirs", "lbs_weights", "shapedirs", "faces", "identity_joints")
REGRESSED_JOINTSTYPES = ("vibe", "a2m", "a2mpl")                         # index maps into [chain joints | vertex joints | regressed joints] (model/smpl.py:76-98)
DEFAULT_MAP_ROOTS = {"vibe": 8, "a2m": 0, "a2mpl": 0}                     # the output row that is subtracted (JOINTSTYPE_ROOT, model/smpl.py)
REGRESSOR_KEYS = ("vertex_joints", "J_regressor_extra", "map_vibe", "map_a2m", "map_a2mpl", "map_roots")


def check_body(d):
    """check_skeleton's dict plus 'mesh': dict(v_template fp32 [V,3], posedirs fp32 [9(J-1),3V] | None, lbs_weights fp32 [V,J], shapedirs fp32
    [V,3,nb] | None, faces int32 [F,3] | None, identity_joints int32 [n]), validated (the checks rgn_body_create makes, and those only a file can fail)."""
    out = check_skeleton(d)
    J = len(out["parents"])
    m = d["mesh"] if isinstance(d.get("mesh", None), dict) else d
    if m.get("v_template", None) is None or m.get("lbs_weights", None) is None:
        raise ValueError("body: v_template and lbs_weights are required (a skeleton file holds no mesh: write one with tools/make_skeleton.py --mesh)")
    vt = np.ascontiguousarray(m["v_template"], dtype=np.float32)
    if vt.ndim != 2 or vt.shape[1] != 3 or not 1 <= vt.shape[0] <= 65536:
        raise ValueError(f"body: v_template {vt.shape}: need [V, 3] with 1 <= V <= 65536")
    V = vt.shape[0]
    w = np.ascontiguousarray(m["lbs_weights"], dtype=np.float32)
    if w.shape != (V, J):
        raise ValueError(f"body: lbs_weights {w.shape} is not [V, J] = [{V}, {J}]")
    if (w < 0).any() or float(np.abs(w.astype(np.float64).sum(1) - 1).max()) > 1e-5:
        raise ValueError("body: every row of lbs_weights must be non-negative and sum to 1 (within 1e-5)")
    pd = m.get("posedirs", None)
    if pd is not None:
        pd = np.ascontiguousarray(pd, dtype=np.float32)
        if pd.shape != (9 * (J - 1), 3 * V):
            raise ValueError(f"body: posedirs {pd.shape} is not [9 (J - 1), 3 V] = [{9 * (J - 1)}, {3 * V}]")
    sd = m.get("shapedirs", None)
    if sd is not None:
        sd = np.ascontiguousarray(sd, dtype=np.float32)
        if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] > 16:
            raise ValueError(f"body: shapedirs {sd.shape} is not [V, 3, nb] with nb <= 16")
        if out["shape_joints"] is None or out["shape_joints"].shape[2] != sd.shape[2]:
            raise ValueError("body: shapedirs need shape_joints with as many shape directions (joints and surface move together)")
        if sd.shape[2] == 0:
            sd = None
    faces = m.get("faces", None)
    if faces is not None:
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        if faces.ndim != 2 or faces.shape[1] != 3 or (faces.size and (faces.min() < 0 or faces.max() >= V)):
            raise ValueError(f"body: faces {faces.shape} is not [F, 3] with vertex indices in [0, V)")
    ij = m.get("identity_joints", None)
    idj = np.zeros(0, np.int32) if ij is None else np.ascontiguousarray(ij, dtype=np.int32).reshape(-1)
    if len(idj) and (idj.min() < 1 or idj.max() >= J):
        raise ValueError(f"body: identity_joints {idj.tolist()} outside [1, J) = [1, {J})")
    out["mesh"] = {"v_template": vt, "posedirs": pd, "lbs_weights": w, "shapedirs": sd, "faces": faces, "identity_joints": idj}
    out["mesh"].update(check_joint_regressors(m, V, J))
    return out


def check_joint_regressors(m, V, J):
    """The regressed joint types' part of a body dict -> dict(vertex_joints int32 [Np] | None, J_regressor_extra fp32 [Jr, V] | None, joint_maps
    {type: int32 [n]}, map_roots {type: int}), validated (the checks rgn_body_set_joint_regressors and rgn_rot2joints make, and those only a file
    can fail). Maps come as `joint_maps` (a dict) or as the file's keys map_vibe / map_a2m / map_a2mpl; all four values are None / empty where the
    body holds no regressors."""
    vj, reg = m.get("vertex_joints", None), m.get("J_regressor_extra", None)
    maps = dict(m["joint_maps"]) if isinstance(m.get("joint_maps", None), dict) else {t: m["map_" + t] for t in REGRESSED_JOINTSTYPES if m.get("map_" + t, None) is not None}
    roots = m.get("map_roots", None)
    if vj is None and reg is None:
        if maps or roots is not None:
            raise ValueError("body: joint_maps / map_roots without vertex_joints or J_regressor_extra")
        return {"vertex_joints": None, "J_regressor_extra": None, "joint_maps": {}, "map_roots": {}}
    vj = np.zeros(0, np.int32) if vj is None else np.asarray(vj)
    if vj.ndim != 1 or (vj.size and (not np.issubdtype(vj.dtype, np.integer) or vj.min() < 0 or vj.max() >= V)):
        raise ValueError(f"body: vertex_joints {vj.shape} is not [Np] integer vertex ids in [0, V) = [0, {V})")
    vj = np.ascontiguousarray(vj, dtype=np.int32)
    reg = np.zeros((0, V), np.float32) if reg is None else np.ascontiguousarray(reg, dtype=np.float32)
    if reg.ndim != 2 or reg.shape[1] != V:
        raise ValueError(f"body: J_regressor_extra {reg.shape} is not [Jr, V] = [Jr, {V}]")
    if not np.isfinite(reg).all():
        raise ValueError("body: J_regressor_extra holds a value that is not finite")
    Np, Jr = len(vj), len(reg)
    if Np + Jr == 0:
        raise ValueError("body: vertex_joints and J_regressor_extra are both empty (Np or Jr may be 0, not both)")
    if Np + Jr > 32:
        raise ValueError(f"body: Np + Jr = {Np} + {Jr} > 32 vertex and regressed joints")
    nall, good = J + Np + Jr, {}
    for t, a in maps.items():
        if t not in REGRESSED_JOINTSTYPES:
            raise ValueError(f"body: joint_maps has {t!r}; the joint types are {REGRESSED_JOINTSTYPES}")
        a = np.asarray(a)
        if a.ndim != 1 or not 1 <= a.size <= 64 or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() >= nall:
            raise ValueError(f"body: map_{t} {a.shape} is not 1 to 64 integer entries in [0, J + Np + Jr) = [0, {nall})")
        good[t] = np.ascontiguousarray(a, dtype=np.int32)
    if roots is None:
        roots = DEFAULT_MAP_ROOTS
    elif not isinstance(roots, dict):
        r = np.asarray(roots).reshape(-1)
        if r.shape != (3,) or not np.issubdtype(r.dtype, np.integer):
            raise ValueError(f"body: map_roots {r.shape} is not [3] integers (the root rows of {REGRESSED_JOINTSTYPES})")
        roots = dict(zip(REGRESSED_JOINTSTYPES, (int(v) for v in r)))
    for t, a in good.items():
        if not 0 <= int(roots.get(t, 0)) < len(a):
            raise ValueError(f"body: map_roots[{t!r}] = {roots.get(t, 0)} is no row of map_{t} ({len(a)} rows)")
    return {"vertex_joints": vj, "J_regressor_extra": reg, "joint_maps": good, "map_roots": {t: int(roots.get(t, 0)) for t in REGRESSED_JOINTSTYPES}}


def body_file_arrays(body):
    """check_body's dict -> the flat {key: array} a body npz holds (np.savez(path, **body_file_arrays(body)); load_body reads it back)."""
    d = {"rest_joints": body["rest_joints"], "parents": body["parents"], "body_model": np.array(body.get("body_model", ""))}
    if body.get("shape_joints", None) is not None:
        d["shape_joints"] = body["shape_joints"]
    m = body["mesh"]
    for k in MESH_KEYS + ("vertex_joints", "J_regressor_extra"):
        if m.get(k, None) is not None:
            d[k] = m[k]
    for t, a in (m.get("joint_maps", None) or {}).items():
        d["map_" + t] = a
    if m.get("joint_maps", None):
        d["map_roots"] = np.array([m["map_roots"][t] for t in REGRESSED_JOINTSTYPES], np.int32)
    return d


def load_body(path):
    """Read a body npz (module docstring) -> check_body's dict."""
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in ("rest_joints", "parents")}
        d["shape_joints"] = z["shape_joints"] if "shape_joints" in z.files else None
        d["body_model"] = str(z["body_model"]) if "body_model" in z.files else ""
        for k in MESH_KEYS + REGRESSOR_KEYS:
            d[k] = z[k] if k in z.files else None
    return check_body(d)


def load_skeleton_or_body(path):
    """A body file gives check_body's dict, a skeleton file check_skeleton's."""
    with np.load(path, allow_pickle=False) as z:
        mesh = "v_template" in z.files
    return load_body(path) if mesh else load_skeleton(path)


class Rotation2xyz:
    """`Rotation2xyz(skeleton, model)(x, mask, pose_rep, translation, glob, jointstype, vertstrans, ...)` with the keyword arguments of both
    reference classes; unknown extras are accepted and ignored as on `Rotation2xyz_x`. `model` is the CMDM whose engine runs the kernel."""

    def __init__(self, skeleton, model=None):
        with_mesh = isinstance(skeleton.get("mesh", None), dict) or skeleton.get("v_template", None) is not None
        self.skeleton = check_body(skeleton) if with_mesh else check_skeleton(skeleton)
        self.mesh = self.skeleton.get("mesh", None)     # None: a skeleton file, joints only
        self._body, self._work = None, None             # (BodyEngine, its device), workspace tensor: made at the first 'vertices' call
        self._sj_dev = {}                               # (device, nb) -> shape_joints on that device, for per-frame betas
        self.model = model
        self.smpl_model = None          # (the reference keeps its body layer here; there is none)
        sj = self.skeleton["shape_joints"]
        self.num_betas = 10 if sj is None else int(sj.shape[2])

    def rest_joints(self, betas=None, beta=0):
        """rest + sum_k betas[k] * shape_joints[:, :, k], formed per call on the host; betas None -> zeros with betas[1] = beta (:289-292)."""
        sk = self.skeleton
        b = self.betas_vector(betas, beta)
        if not b.any():
            return sk["rest_joints"]
        if sk["shape_joints"] is None:
            raise ValueError("non-zero betas / beta need `shape_joints` in the skeleton file")
        if len(b) > sk["shape_joints"].shape[2]:
            raise ValueError(f"{len(b)} betas but the skeleton file holds {sk['shape_joints'].shape[2]} shape directions")
        return sk["rest_joints"] + sk["shape_joints"][:, :, :len(b)] @ b

    def betas_vector(self, betas=None, beta=0):
        """The one shape vector of a call, fp64 [n]."""
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
        return b

    def shape_plan(self, betas, beta, betas_per_motion, mask, B, T, P, vertices=False):
        """Which route a call's shape arguments take, decided and checked on the host: None where the call has ONE shape and rest_joints() serves
        it (betas None, 1-D, or 2-D with equal rows: today's path, today's bits), else ('frames' | 'motions', rows) for the per-frame kernels.
          betas [N_live, nb] with differing rows  the reference's meaning: row n is the n-th unmasked frame in (b, t) order, for every person
          betas_per_motion [B, nb] | [B, P, nb]   one shape per motion, or per motion and person
        Fewer betas than the file's shape directions count the rest as 0; more, or a file without them, is a ValueError."""
        if betas_per_motion is not None:
            if betas is not None or beta != 0:
                raise ValueError("betas_per_motion and betas / beta are mutually exclusive: give the shapes one way")
            rows = torch.as_tensor(betas_per_motion).detach()
            if rows.ndim not in (2, 3) or tuple(rows.shape[:-1]) not in ((B,), (B, P)):
                raise ValueError(f"betas_per_motion {tuple(rows.shape)}: expected [B, nb] = [{B}, nb] or [B, P, nb] = [{B}, {P}, nb]")
            kind = "motions"
        else:
            if betas is None or getattr(betas, "ndim", 0) != 2:
                return None
            rows = torch.as_tensor(betas).detach()
            if rows.shape[0] == 0 or bool((rows == rows[:1]).all()):
                return None
            n_live = B * T if mask is None else int(torch.as_tensor(mask).reshape(B, T).bool().sum())
            if rows.shape[0] != n_live:
                raise ValueError(f"betas has {rows.shape[0]} rows, but the mask leaves {n_live} frames (one row per unmasked frame, in (b, t) order)")
            kind = "frames"
        sj, nb = self.skeleton["shape_joints"], int(rows.shape[-1])
        if sj is None or sj.shape[2] == 0:
            raise ValueError("per-frame betas need `shape_joints` in the skeleton file")
        if vertices and self.mesh["shapedirs"] is None:
            raise ValueError("per-frame betas need `shapedirs` in the body file")
        if not 1 <= nb <= sj.shape[2]:
            raise ValueError(f"{nb} betas but the {'body' if vertices else 'skeleton'} file holds {sj.shape[2]} shape directions")
        return kind, rows

    def device_shape(self, plan, mask, B, T, P, dev):
        """shape_plan's rows on the device -> (betas fp32, (stride_b, stride_p, stride_t) in elements, shape_joints fp32 [J, 3, nb]) as
        rgn_rot2xyz_shaped / rgn_rot2verts_shaped take them. `mask`: bool [B, T] on dev, or None."""
        kind, rows = plan
        nb = int(rows.shape[-1])
        rows = rows.to(device=dev, dtype=torch.float32).contiguous()
        if kind == "motions":
            bt, strides = rows, ((nb, 0, 0) if rows.ndim == 2 else (P * nb, nb, 0))
        else:
            if mask is None:
                bt = rows.reshape(B, T, nb)
            else:                               # scattered to [B, T, nb]; the masked frames' rows are never read
                bt = torch.zeros((B, T, nb), device=dev, dtype=torch.float32)
                bt[mask] = rows
            strides = (T * nb, 0, nb)
        key = (str(dev), nb)
        if key not in self._sj_dev:             # the first nb directions, re-packed [J, 3, nb]: made once per device
            self._sj_dev[key] = torch.from_numpy(np.ascontiguousarray(self.skeleton["shape_joints"][:, :, :nb], dtype=np.float32)).to(dev)
        return bt, strides, self._sj_dev[key]

    def body_engine(self, dev):
        """The device-resident mesh data for `dev`: created at first use, rebuilt when the model has moved."""
        if self._body is None or self._body[1] != dev:
            if self._body is not None:
                self._body[0].close()
            self._body, self._work = (_lib.BodyEngine(self.mesh, len(self.skeleton["parents"]), dev.index or 0), dev), None
            if self.mesh["vertex_joints"] is not None:      # the regressed joint types: the body cut to their vertices, once
                self._body[0].set_joint_regressors(self.mesh["vertex_joints"], self.mesh["J_regressor_extra"])
        return self._body[0]

    def __call__(self, x, mask, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0, glob_rot=None, num_person=1,
                 get_rotations_back=False, betas_per_motion=None, **kwargs):
        if pose_rep == "xyz":
            return x
        if not glob and glob_rot is None:
            raise TypeError("You must specify global rotation if glob is False")
        if jointstype not in JOINTSTYPES:
            raise NotImplementedError("This jointstype is not implemented.")
        vertices = jointstype == "vertices" and self.mesh is not None
        jmap = None                                     # (map, root row) of a regressed joint type the body file serves
        if jointstype in REGRESSED_JOINTSTYPES and self.mesh is not None and self.mesh["vertex_joints"] is not None:
            if jointstype not in self.mesh["joint_maps"]:
                raise NotImplementedError(f"jointstype={jointstype!r}: the body file holds joint regressors but no `map_{jointstype}` "
                                          f"(tools/make_skeleton.py --mesh --joint_maps)")
            jmap, vertices = (self.mesh["joint_maps"][jointstype], self.mesh["map_roots"][jointstype]), True
        if jointstype not in SKELETON_JOINTSTYPES and not vertices:
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
        plan = self.shape_plan(betas, beta, betas_per_motion, mask, B, T, P, vertices)      # not None: a shape per frame, read on the device
        if vertices:
            return self._vertices(x, mask, pose_rep, translation, glob, vertstrans, betas, beta, glob_rot, P, get_rotations_back, plan, jmap)
        eng = model._engine if (model._engine is not None and not model._engine_stale) else model._get_engine(B, T)[0]
        dev = next(model.parameters()).device
        xc = x.to(device=dev, dtype=torch.float32).contiguous()
        mc = None if mask is None else mask.to(device=dev).reshape(B, T).bool().contiguous()
        out = torch.empty((B, J, 3 * P, T), device=dev, dtype=torch.float32)
        rot = torch.empty((B, P, T, J, 3, 3), device=dev, dtype=torch.float32) if get_rotations_back else None
        flags = (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)
        gr = None if glob else np.asarray(glob_rot, dtype=np.float32).reshape(3)
        if plan is not None:
            shape = self.device_shape(plan, mc, B, T, P, dev)
            eng.rot2xyz_shaped(xc, mc, self.skeleton["rest_joints"], self.skeleton["parents"], shape[2], shape[0], shape[1], _lib.POSE_REP[pose_rep], P,
                               flags, gr, out, rot, dist_util.stream_handle(dev))
        else:
            eng.rot2xyz(xc, mc, self.rest_joints(betas, beta), self.skeleton["parents"], _lib.POSE_REP[pose_rep], P, flags, gr, out, rot,
                        dist_util.stream_handle(dev))
        out = out.to(x.device)
        if get_rotations_back:      # Rotation2xyz (:152-153): the last person's matrices of the unmasked frames, without and with joint 0
            r = rot[:, -1] if mc is None else rot[:, -1][mc]
            r = r.reshape(-1, J, 3, 3)
            return out, r[:, 1:], r[:, 0]
        return out

    def _vertices(self, x, mask, pose_rep, translation, glob, vertstrans, betas, beta, glob_rot, P, get_rotations_back, plan=None, jmap=None):
        """jointstype='vertices' (:236-249 / :303-321): [B, V, 3 P, T] by linear blend skinning on the device (rgn_rot2verts; with a shape per
        frame rgn_rot2verts_shaped). jmap = (map, root row): a regressed joint type (:17-155 over model/smpl.py:76-98) instead, [B, len(map), 3 P, T]
        from the same skinning restricted to the vertices its joints touch (rgn_rot2joints / rgn_rot2joints_shaped); no vertex array exists."""
        J, V = len(self.skeleton["parents"]), self.mesh["v_template"].shape[0]
        B, T = x.shape[0], x.shape[-1]
        dev = next(self.model.parameters()).device
        body = self.body_engine(dev)
        mc = None if mask is None else mask.to(device=dev).reshape(B, T).bool().contiguous()
        shape = None if plan is None else self.device_shape(plan, mc, B, T, P, dev)
        b = np.zeros(1) if shape is not None else self.betas_vector(betas, beta)
        bv = None
        if b.any():
            if body.nb == 0:
                raise ValueError("non-zero betas / beta need `shapedirs` in the body file")
            if len(b) > body.nb:
                raise ValueError(f"{len(b)} betas but the body file holds {body.nb} shape directions")
            bv = np.zeros(body.nb, np.float32)
            bv[:len(b)] = b
        xc = x.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty((B, V if jmap is None else len(jmap[0]), 3 * P, T), device=dev, dtype=torch.float32)
        rot = torch.empty((B, P, T, J, 3, 3), device=dev, dtype=torch.float32) if get_rotations_back else None
        if jmap is None:
            need = body.workspace_bytes(B, T, P) if shape is None else body.workspace_bytes_shaped(B, T, P)
        else:
            need = body.joints_workspace_bytes(B, T, P) if shape is None else body.joints_workspace_bytes_shaped(B, T, P)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, device=dev, dtype=torch.uint8)
        flags = (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)
        gr = None if glob else np.asarray(glob_rot, dtype=np.float32).reshape(3)
        with torch.cuda.device(dev):
            if jmap is not None and shape is not None:
                body.rot2joints_shaped(xc, mc, self.skeleton["rest_joints"], self.skeleton["parents"], shape[2], shape[0], shape[1],
                                       _lib.POSE_REP[pose_rep], P, flags, gr, jmap[0], jmap[1], out, rot, self._work, dist_util.stream_handle(dev))
            elif jmap is not None:
                body.rot2joints(xc, mc, self.rest_joints(betas, beta), self.skeleton["parents"], _lib.POSE_REP[pose_rep], P, flags, gr, bv, jmap[0],
                                jmap[1], out, rot, self._work, dist_util.stream_handle(dev))
            elif shape is not None:
                body.rot2verts_shaped(xc, mc, self.skeleton["rest_joints"], self.skeleton["parents"], shape[2], shape[0], shape[1],
                                      _lib.POSE_REP[pose_rep], P, flags, gr, out, rot, self._work, dist_util.stream_handle(dev))
            else:
                body.rot2verts(xc, mc, self.rest_joints(betas, beta), self.skeleton["parents"], _lib.POSE_REP[pose_rep], P, flags, gr, bv, out, rot,
                               self._work, dist_util.stream_handle(dev))
        out = out.to(x.device)
        if get_rotations_back:
            r = rot[:, -1] if mc is None else rot[:, -1][mc]
            r = r.reshape(-1, J, 3, 3)
            return out, r[:, 1:], r[:, 0]
        return out
