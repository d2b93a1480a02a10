"""CPU: the vertex restatement (tests/rot2verts_ref.py) is pinned to goldens recorded from the reference's own wrappers
(tests/golden/make_golden_rot2verts.py) and to what linear blend skinning must give analytically; the host side of the feature - synthetic body,
body files, the extraction tool's --mesh, the OBJ writer, the CLI flags, the C entry points' argument checks - behaves as specified.
The kernels are tested in tests/test_rot2verts_gpu.py."""
import ctypes
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests.rot2verts_ref import golden_body, golden_settings, rot2verts_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "rot2verts_*.npz")))


def test_the_recorded_cases_are_all_there():
    assert {n[len("rot2verts_"):] for n in GOLDENS} == {"p1", "p2_ragged", "smpl24", "beta", "noglob_rotvec", "novertstrans"}
    assert all(os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) < 200 * 1024 for n in GOLDENS)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_reference(golden, name):
    """fp64 within 1e-12 of the recorded run; fp32 within the deviation the recorder measured and stored (fp32_dev), which itself stays below
    1e-5 at |xyz| < 4 - were it larger, the synthetic body would be at fault."""
    g = golden(name)
    exp, body = g["expected"], golden_body(g)
    mask = None if bool(g["mask_none"]) else torch.from_numpy(g["mask"])
    assert exp.dtype == np.float64 and float(np.abs(exp).max()) < 4.0 and float(g["fp32_dev"]) <= 1e-5
    e64 = float(np.abs(rot2verts_ref(g["x"], mask, body, dtype=torch.float64, **golden_settings(g)).numpy() - exp).max())
    e32 = float(np.abs(rot2verts_ref(g["x"], mask, body, dtype=torch.float32, **golden_settings(g)).double().numpy() - exp).max())
    print(f"{name}: fp64 {e64:.2e}  fp32 {e32:.2e}  recorded fp32_dev {float(g['fp32_dev']):.2e}")
    assert e64 < 1e-12, e64
    assert e32 <= float(g["fp32_dev"]), (e32, float(g["fp32_dev"]))


def test_masked_frames_of_the_goldens_hold_the_translation_term_alone(golden):
    g = golden("rot2verts_p2_ragged")
    x = g["x"].astype(np.float64)
    for b, t in zip(*np.nonzero(~g["mask"])):                       # two persons: masked frames are 0 + the row as stored (:247-249)
        for p in range(2):
            assert np.array_equal(g["expected"][b, :, 3 * p:3 * p + 3, t], np.broadcast_to(x[b, -1, 6 * p:6 * p + 3, t], (130, 3)))
    g = golden("rot2verts_novertstrans")                            # no translation term: masked frames are 0
    assert all(not g["expected"][b, :, :, t].any() for b, t in zip(*np.nonzero(~g["mask"])))


def identity_x(B, T, J, rng=None):
    """rot6d rows of the identity for J joints + a translation row."""
    x = np.zeros((B, J + 1, 6, T), np.float32)
    x[:, :J, 0] = 1
    x[:, :J, 4] = 1
    if rng is not None:
        x[:, J, :3] = rng.uniform(-1, 1, (B, 3, T))
    return x


def rot6d_of(R):
    return np.concatenate([R[0], R[1]]).astype(np.float32)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 1e-6)])
def test_identity_pose_gives_v_shaped(dtype, tol):
    """... times the vertex's weight sum, which is 1 to fp32's precision: the blend of J equal transforms is (sum_j w) times that transform."""
    body = synth.make_body()
    m = body["mesh"]
    ws = m["lbs_weights"].astype(np.float64).sum(1, keepdims=True)
    out = rot2verts_ref(identity_x(1, 2, 55), None, body, "rot6d", True, True, True, dtype=dtype).double().numpy()
    assert np.abs(out[0, :, :, 1] - ws * m["v_template"]).max() < tol
    out = rot2verts_ref(identity_x(1, 2, 55), None, body, "rot6d", True, True, True, beta=1.5, dtype=dtype).double().numpy()
    assert np.abs(out[0, :, :, 0] - ws * (m["v_template"].astype(np.float64) + 1.5 * m["shapedirs"][:, :, 1].astype(np.float64))).max() < tol


def test_a_pure_root_rotation_turns_the_body_about_joint_0():
    body = synth.make_body()
    R = rotation([0.3, -1.0, 0.5], 1.1)
    x = identity_x(1, 1, 55)
    x[0, 0, :, 0] = rot6d_of(R)
    out = rot2verts_ref(x, None, body, "rot6d", True, True, True).numpy()[0, :, :, 0]
    j0 = body["rest_joints"][0].astype(np.float64)
    Rx = rot2verts_ref(x, None, body, "rot6d", True, True, True, dtype=torch.float64)           # (the matrix as the conversion gives it from fp32 rows)
    R32 = np.stack([rot6d_of(R)[:3], rot6d_of(R)[3:]]).astype(np.float64)
    b1 = R32[0] / np.linalg.norm(R32[0])
    b2 = R32[1] - (b1 @ R32[1]) * b1
    b2 /= np.linalg.norm(b2)
    Rm = np.stack([b1, b2, np.cross(b1, b2)])
    ws = body["mesh"]["lbs_weights"].astype(np.float64).sum(1, keepdims=True)                   # (1 to fp32's precision)
    want = ws * ((body["mesh"]["v_template"].astype(np.float64) - j0) @ Rm.T + j0)               # the root's pose feature is not part of pf: no blend shapes move
    assert Rx.shape == (1, 130, 3, 1) and np.abs(out - want).max() < 1e-12


def test_rotating_a_joint_moves_only_vertices_weighted_on_its_subtree():
    body = synth.make_body(identity_joints=[])
    body["mesh"]["posedirs"] = None                                 # (pose blend shapes move every vertex a little; skinning alone is local)
    parents, w = body["parents"], body["mesh"]["lbs_weights"]
    base = rot2verts_ref(identity_x(1, 1, 55), None, body, "rot6d", True, True, True).numpy()[0, :, :, 0]
    for j in (3, 9, 22, 40):
        sub = {j}
        for i in range(j + 1, 55):
            if int(parents[i]) in sub:
                sub.add(i)
        x = identity_x(1, 1, 55)
        x[0, j, :, 0] = rot6d_of(rotation([1.0, 0.2, -0.4], 0.9))
        moved = np.abs(rot2verts_ref(x, None, body, "rot6d", True, True, True).numpy()[0, :, :, 0] - base).max(1) > 1e-9
        on = w[:, sorted(sub)].sum(1) > 0
        assert not (moved & ~on).any() and moved.any() and (moved <= on).all(), j


def test_identity_joints_are_ignored_by_chain_pose_feature_and_skinning():
    body = synth.make_body()
    assert list(body["mesh"]["identity_joints"]) == [22, 23, 24]
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.standard_normal((2, 56, 6, 3)).astype(np.float32)
    y = x.copy()
    y[:, 22:25] = rng.standard_normal((2, 3, 6, 3))
    a = rot2verts_ref(x, None, body, "rot6d", True, True, True).numpy()
    assert np.array_equal(a, rot2verts_ref(y, None, body, "rot6d", True, True, True).numpy())
    assert not np.array_equal(rot2verts_ref(x, None, body, "rot6d", True, True, True, identity_joints=[]).numpy(),
                              rot2verts_ref(y, None, body, "rot6d", True, True, True, identity_joints=[]).numpy())


def test_make_body_is_deterministic_over_make_skeletons_skeleton_and_regressor_consistent():
    from regennet_amd.model.rotation2xyz import Rotation2xyz, check_body
    body, again, sk = synth.make_body(), synth.make_body(), synth.make_skeleton()
    m = body["mesh"]
    assert all(np.array_equal(body[k], sk[k]) for k in ("rest_joints", "parents", "shape_joints"))
    assert all(np.array_equal(m[k], again["mesh"][k]) for k in ("v_template", "posedirs", "lbs_weights", "shapedirs", "faces", "identity_joints"))
    assert m["v_template"].shape == (130, 3) and m["posedirs"].shape == (486, 390) and m["lbs_weights"].shape == (130, 55) and m["shapedirs"].shape == (130, 3, 10)
    assert m["faces"].dtype == np.int32 and m["faces"].min() >= 0 and m["faces"].max() < 130 and list(m["identity_joints"]) == [22, 23, 24]
    assert ((m["lbs_weights"] > 0).sum(1) == 4).all() and float(np.abs(m["posedirs"]).max()) < 0.06
    rest, parents = sk["rest_joints"].astype(np.float64), sk["parents"]
    for v in range(130):                                            # within 10 cm of a bone, and weighted on that bone's joints
        d = []
        for j in range(1, 55):
            a, b = rest[parents[j]], rest[j]
            s = np.clip((m["v_template"][v] - a) @ (b - a) / ((b - a) @ (b - a)), 0, 1)
            d.append(np.linalg.norm(m["v_template"][v] - (a + s * (b - a))))
        assert min(d) < 0.10 + 1e-6, (v, min(d))
    reg = m["J_regressor"]
    assert reg.shape == (55, 130) and (reg >= 0).all() and np.allclose(reg.sum(1), 1)
    betas = np.zeros(10)
    betas[1] = 1.5
    v_shaped = m["v_template"].astype(np.float64) + m["shapedirs"].astype(np.float64) @ betas
    assert float(np.abs(reg @ v_shaped - Rotation2xyz(body).rest_joints(beta=1.5)).max()) < 1e-6
    assert list(synth.make_body(24, 70, seed=24)["mesh"]["identity_joints"]) == [] and check_body(synth.make_body(1, 1))["mesh"]["posedirs"].shape == (0, 3)
    for J, V in ((2, 63), (64, 65), (64, 63)):
        check_body(synth.make_body(J, V, seed=J))


def test_body_file_round_trip_and_validation(tmp_path):
    from regennet_amd.model.rotation2xyz import check_body, check_skeleton, load_body, load_skeleton, load_skeleton_or_body
    body = synth.make_body()
    path = str(tmp_path / "body.npz")
    flat = {k: body[k] for k in ("rest_joints", "parents", "shape_joints", "body_model")}
    flat.update({k: v for k, v in body["mesh"].items() if k != "J_regressor"})
    np.savez(path, **flat)
    got = load_body(path)
    assert all(np.array_equal(got["mesh"][k], body["mesh"][k]) for k in ("v_template", "posedirs", "lbs_weights", "shapedirs", "faces", "identity_joints"))
    assert np.array_equal(got["parents"], body["parents"]) and got["body_model"] == "synthetic55"
    assert "mesh" in load_skeleton_or_body(path) and "mesh" not in load_skeleton(path)         # load_skeleton reads the skeleton of a body file, as before
    skel = str(tmp_path / "skel.npz")
    np.savez(skel, **synth.make_skeleton())
    assert "mesh" not in load_skeleton_or_body(skel)
    with pytest.raises(ValueError, match="v_template and lbs_weights"):
        load_body(skel)
    assert "mesh" not in check_skeleton(body)

    def broken(**kw):
        d = dict(body, mesh=dict(body["mesh"]))
        for k, v in kw.items():
            if k in ("parents", "shape_joints"):
                d[k] = v
            else:
                d["mesh"][k] = v
        return d

    m = body["mesh"]
    w_neg = m["lbs_weights"].copy()
    w_neg[0, np.flatnonzero(w_neg[0])[:2]] += np.array([-2.0, 2.0], np.float32)
    bad_par = body["parents"].copy()
    bad_par[3] = 7
    for kw, text in ((dict(v_template=np.zeros((130, 2))), "v_template"), (dict(v_template=np.zeros((65537, 3), np.float32)), "V <= 65536"),
                     (dict(lbs_weights=m["lbs_weights"][:, :54]), r"lbs_weights .* is not \[V, J\]"), (dict(lbs_weights=m["lbs_weights"] * 1.001), "sum to 1"),
                     (dict(lbs_weights=w_neg), "non-negative"), (dict(posedirs=m["posedirs"][:-1]), "posedirs"), (dict(shapedirs=m["shapedirs"][:, :2]), "shapedirs"),
                     (dict(shapedirs=m["shapedirs"][:, :, :4]), "shape_joints"), (dict(faces=m["faces"] + 5), "faces"), (dict(identity_joints=[0]), "identity_joints"),
                     (dict(identity_joints=[55]), "identity_joints"), (dict(parents=bad_par), "parents")):
        with pytest.raises(ValueError, match=text):
            check_body(broken(**kw))
    ok = check_body(broken(posedirs=None, faces=None, identity_joints=None))
    assert ok["mesh"]["posedirs"] is None and ok["mesh"]["faces"] is None and len(ok["mesh"]["identity_joints"]) == 0


def test_make_skeleton_tool_mesh_flag(tmp_path):
    spec = importlib.util.spec_from_file_location("make_skeleton_tool", os.path.join(ROOT, "tools", "make_skeleton.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.Generator(np.random.PCG64(5))
    J, V = 7, 40
    reg = rng.uniform(0, 1, (J, V))
    reg /= reg.sum(1, keepdims=True)
    vt, sd = rng.standard_normal((V, 3)), rng.standard_normal((V, 3, 12))
    kt = np.array([[2 ** 32 - 1, 0, 0, 1, 2, 2, 5], np.arange(J)], dtype=np.uint32)
    w = rng.uniform(0, 1, (V, J))
    w /= w.sum(1, keepdims=True)
    pdirs = rng.standard_normal((V, 3, 9 * (J - 1)))
    faces = rng.integers(0, V, (9, 3)).astype(np.uint32)
    src = str(tmp_path / "model.npz")
    np.savez(src, J_regressor=reg, v_template=vt, shapedirs=sd, kintree_table=kt, weights=w, posedirs=pdirs, f=faces, unrelated=np.zeros(3))
    plain, again, mesh, smplx = (str(tmp_path / n) for n in ("plain.npz", "again.npz", "mesh.npz", "smplx.npz"))
    tool.main([src, "--out", plain, "--body_model", "toy"])
    with np.load(plain) as z:
        assert sorted(z.files) == ["body_model", "parents", "rest_joints", "shape_joints"]         # without --mesh: what the tool wrote before
    tool.main([src, "--out", again, "--body_model", "toy"])
    assert open(plain, "rb").read() == open(again, "rb").read()
    tool.main([src, "--out", mesh, "--body_model", "toy", "--mesh"])
    from regennet_amd.model.rotation2xyz import load_body, load_skeleton
    body, sk = load_body(mesh), load_skeleton(plain)
    assert all(np.array_equal(body[k], sk[k]) for k in ("rest_joints", "parents", "shape_joints"))
    m = body["mesh"]
    assert np.array_equal(m["v_template"], vt.astype(np.float32)) and np.array_equal(m["lbs_weights"], w.astype(np.float32))
    assert m["posedirs"].shape == (9 * (J - 1), 3 * V) and m["posedirs"][5, 3 * 11 + 2] == np.float32(pdirs[11, 2, 5])
    assert m["shapedirs"].shape == (V, 3, 10) and m["faces"].dtype == np.int32 and np.array_equal(m["faces"], faces) and len(m["identity_joints"]) == 0
    tool.main([src, "--out", smplx, "--body_model", "smplx", "--mesh"])
    with np.load(smplx) as z:
        assert list(z["identity_joints"]) == [22, 23, 24]          # (a toy of 7 joints cannot use them: load_body refuses the file)
    with pytest.raises(ValueError, match="identity_joints"):
        load_body(smplx)


def test_obj_writer_text(tmp_path):
    from regennet_amd.utils.mesh_io import obj_text, write_obj_sequences
    v = np.array([[0, 0, 0], [1, 0.5, -2], [0.25, 1e-3, 3]], np.float32)
    assert obj_text(v, np.array([[0, 1, 2]])) == "v 0.000000 0.000000 0.000000\nv 1.000000 0.500000 -2.000000\nv 0.250000 0.001000 3.000000\nf 1 2 3\n"
    assert obj_text(v) == "v 0.000000 0.000000 0.000000\nv 1.000000 0.500000 -2.000000\nv 0.250000 0.001000 3.000000\n"
    seq = np.stack([v, v + 1], -1)[None].repeat(2, 0)                # [2, 3, 3, 2]
    assert write_obj_sequences(str(tmp_path / "o"), seq, np.array([[0, 1, 2]])) == 4
    assert open(tmp_path / "o" / "sample01" / "frame001.obj").read().splitlines()[0] == "v 1.000000 1.000000 1.000000"


def test_vertices_flags_parse_in_both_clis_and_need_a_mesh():
    from regennet_amd.sample.cgenerate import set_skeleton
    from regennet_amd.utils.parser_util import cgenerate_args, edit_args
    a = cgenerate_args(["--synthetic"])
    assert a.vertices is False and a.obj_dir == ""
    a = cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--vertices", "--obj_dir", "out"])
    assert a.vertices is True and a.obj_dir == "out"
    e = edit_args(["--synthetic", "--skeleton", "body.npz", "--vertices"])
    assert e.vertices is True and e.obj_dir == "" and e.skeleton == "body.npz"
    with pytest.raises(SystemExit, match="--vertices needs --skeleton"):
        set_skeleton(None, cgenerate_args(["--synthetic", "--vertices"]))
    with pytest.raises(SystemExit, match="--obj_dir"):
        set_skeleton(None, cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--obj_dir", "out"]))


def test_vertices_are_served_only_by_a_body_with_a_mesh():
    """Rotation2xyz over a body accepts 'vertices' up to the point where it needs the device; the regressed joint types stay refused."""
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    from tests.test_rot2xyz_cpu import _model
    body = synth.make_body(4, 9)
    r2x = Rotation2xyz(body, model=_model())
    assert r2x.mesh is not None and Rotation2xyz(synth.make_skeleton(4)).mesh is None
    x = torch.zeros(2, 5, 6, 8)
    kw = dict(mask=None, translation=True, glob=True, vertstrans=True)
    for jt in ("vibe", "a2m", "a2mpl"):
        with pytest.raises(NotImplementedError, match="vertices"):
            r2x(x, pose_rep="rot6d", jointstype=jt, **kw)
    with pytest.raises(ValueError, match=r"\[B, 5, 6, T\]"):
        r2x(torch.zeros(2, 6, 6, 8), pose_rep="rot6d", jointstype="vertices", **kw)
    m = _model()
    m.set_skeleton(body)
    assert m.rot2xyz.mesh is not None


def test_body_abi_symbols_and_argument_checks_without_a_device():
    from regennet_amd import _lib
    lib = _lib.load()
    for name in ("rgn_body_create", "rgn_body_destroy", "rgn_body_last_error", "rgn_rot2verts_workspace", "rgn_rot2verts"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    assert all(f" {n}(" in header for n in ("rgn_body_create", "rgn_body_destroy", "rgn_body_last_error", "rgn_rot2verts_workspace", "rgn_rot2verts"))
    vt, w, pd, sd = np.zeros((4, 3), np.float32), np.ones((4, 2), np.float32) / 2, np.zeros((9, 12), np.float32), np.zeros((4, 3, 2), np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def create(V=4, J=2, nb=2, vt_=vt, pd_=pd, w_=w, sd_=sd, idj=None, out=True):
        h = ctypes.c_void_p()
        ij = None if idj is None else np.asarray(idj, np.int32)
        rc = lib.rgn_body_create(0, V, J, nb, p(vt_), p(pd_), p(w_), p(sd_), p(ij), 0 if ij is None else len(ij), ctypes.byref(h) if out else None)
        return rc, (lib.rgn_body_last_error(None) or b"").decode(), h

    for kw, text in ((dict(V=0), "V outside [1, 65536]"), (dict(V=65537), "V outside [1, 65536]"), (dict(J=0), "J outside [1, 64]"), (dict(J=65), "J outside [1, 64]"),
                     (dict(nb=17), "nb outside [0, 16]"), (dict(nb=-1), "nb outside [0, 16]"), (dict(vt_=None), "null v_template"), (dict(w_=None), "lbs_weights"),
                     (dict(sd_=None), "without shapedirs"), (dict(idj=[0]), "identity_joints[0] outside [1, J)"), (dict(idj=[1, 2]), "identity_joints[1] outside [1, J)"),
                     (dict(out=False), "null out")):
        rc, err, h = create(**kw)
        assert rc == -1 and text in err and not h.value, (kw, rc, err)
    rc, err, h = create(pd_=None)                                   # no posedirs is allowed ("no pose blend shapes"): it gets as far as the device
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert lib.rgn_body_destroy(h) == 0
    else:
        assert rc == -6 and "no HIP device" in err, (rc, err)
    assert lib.rgn_body_destroy(None) == -1 and lib.rgn_rot2verts_workspace(None, 1, 1, 1, None) == -1
    assert lib.rgn_rot2verts(None, None, None, 1, 1, None, None, 0, 1, 0, None, None, None, None, None, 0, None) == -1
