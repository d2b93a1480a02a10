"""CPU: the restatement of the regressed joint types (tests/rot2joints_ref.py) is pinned to goldens recorded from the reference's own classes
(tests/golden/make_golden_rot2joints.py); the host side of the feature - body-file keys and their checks, the synthetic regressors, the tool, the
ABI's argument checks that need no device, the CLI options - is checked without a GPU. The kernels are tested in tests/test_rot2joints_gpu.py."""
import ctypes
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests.rot2joints_ref import golden_regs, rot2joints_ref, touched
from tests.rot2verts_ref import body_sha256, golden_body, golden_settings
from tests.rot2xyz_shaped_ref import rows_to_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "rot2joints_*.npz")))
TYPES = ("vibe", "a2m", "a2mpl")


def test_the_golden_cases_are_the_issue_s():
    assert {n[len("rot2joints_"):] for n in GOLDENS} == {"vibe_p1", "a2m_ragged", "a2mpl_p2_ragged", "vibe_beta", "a2m_noglob_rotvec", "vibe_novertstrans",
                                                         "vibe_frame_betas"}


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_the_reference(golden, name):
    g = golden(name)
    body = golden_body(g)
    regs = golden_regs(g, body)
    t, s = str(g["jointstype"]), golden_settings(g)
    mask = None if bool(g["mask_none"]) else torch.from_numpy(g["mask"])
    B, T = g["x"].shape[0], g["x"].shape[-1]
    if g["betas"].size:
        s["frame_betas"] = rows_to_frames(g["betas"], None if mask is None else g["mask"], B, T, s["num_person"])
    jmap, root = regs["joint_maps"][t], regs["map_roots"][t]
    exp = g["expected"]
    assert exp.shape == (B, len(jmap), 3 * s["num_person"], T) and len(regs["joint_maps"]["vibe"]) == 49 and len(regs["joint_maps"]["a2m"]) == 18
    assert regs["map_roots"] == {"vibe": 8, "a2m": 0, "a2mpl": 0} and all(int(regs["joint_maps"][k][regs["map_roots"][k]]) == 0 for k in TYPES)
    e64 = float(np.abs(rot2joints_ref(g["x"], mask, body, regs, jmap, root, dtype=torch.float64, **s).numpy() - exp).max())
    e32 = float(np.abs(rot2joints_ref(g["x"], mask, body, regs, jmap, root, dtype=torch.float32, **s).double().numpy() - exp).max())
    print(f"{name}: fp64 {e64:.2e}  fp32 {e32:.3e} (recorded {float(g['fp32_dev']):.3e})")
    assert e64 < 1e-12 and e32 <= float(g["fp32_dev"]) * (1 + 1e-6) + 1e-12


def test_the_restatement_s_vertex_rows_are_rot2verts_ref_s():
    """all_joints' picked block is the vertex restatement's rows, and its first block the joint restatement's before the root subtraction."""
    from tests.rot2verts_ref import rot2verts_ref
    from tests.rot2xyz_ref import rot2xyz_ref
    body = synth.make_body(24, 70, seed=24)
    regs = synth.make_joint_regressors(body, seed=3)
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.standard_normal((2, 25, 6, 5)).astype(np.float32)
    mask = torch.tensor([[1, 1, 0, 1, 1], [0, 1, 1, 1, 0]], dtype=torch.bool)
    kw = dict(pose_rep="rot6d", translation=True, glob=True, vertstrans=False, beta=1.5)
    allj = rot2joints_ref(x, mask, body, regs, None, 0, return_all=True, **kw).numpy()
    verts = rot2verts_ref(x, mask, body, **kw).numpy()
    assert allj.shape == (2, 24 + 21 + 9, 3, 5)
    assert float(np.abs(allj[:, 24:45] - verts[:, regs["vertex_joints"]]).max()) < 1e-12
    reg = regs["J_regressor_extra"].astype(np.float64)
    assert float(np.abs(allj[:, 45:] - np.einsum("jv,bvct->bjct", reg, verts)).max()) < 1e-12
    joints = rot2xyz_ref(x, mask, body, **kw).numpy()
    assert float(np.abs((allj[:, :24] - allj[:, :1]) - joints).max()) < 1e-12


def test_make_body_is_unchanged_and_the_synthetic_regressors():
    g = np.load(os.path.join(ROOT, "tests", "golden", "rot2verts_smpl24.npz"))
    body = synth.make_body(24, 70, seed=24)
    assert body_sha256(body) == str(g["body_sha256"]) and "vertex_joints" not in body["mesh"]
    regs = synth.make_joint_regressors(body)
    again = synth.make_joint_regressors(synth.make_body(24, 70, seed=24))
    assert all(np.array_equal(regs[k], again[k]) for k in ("vertex_joints", "J_regressor_extra")) and all(np.array_equal(regs["joint_maps"][t], again["joint_maps"][t]) for t in TYPES)
    vj, reg, maps = regs["vertex_joints"], regs["J_regressor_extra"], regs["joint_maps"]
    assert vj.shape == (21,) and len(set(vj.tolist())) == 21 and vj.min() >= 0 and vj.max() < 70
    assert reg.shape == (9, 70) and ((reg != 0).sum(1) == 6).all() and ((reg > 0).any(1) & (reg < 0).any(1)).all()
    nall = 24 + 21 + 9
    assert len(maps["vibe"]) == 49 and len(maps["a2m"]) == 18 and np.array_equal(maps["a2mpl"], np.unique(np.r_[np.arange(24), maps["a2m"]]))
    for t in TYPES:
        m = maps[t]
        assert m.min() >= 0 and m.max() < nall and (m < 24).any() and ((m >= 24) & (m < 45)).any() and (m >= 45).any()
        assert int(m[regs["map_roots"][t]]) == 0
    assert len(set(maps["vibe"].tolist())) < 49 and regs["map_roots"] == {"vibe": 8, "a2m": 0, "a2mpl": 0}
    small = synth.make_joint_regressors(synth.make_body(2, 5, seed=2), npicks=21, nreg=2, support=6)
    assert small["vertex_joints"].shape == (5,) and ((small["J_regressor_extra"] != 0).sum(1) == 5).all()
    assert len(touched(regs, 70)) <= 21 + 54


def test_check_body_accepts_and_refuses_the_regressor_keys():
    from regennet_amd.model.rotation2xyz import check_body
    body = synth.make_body(24, 70, seed=24)
    regs = synth.make_joint_regressors(body)
    assert check_body(body)["mesh"]["vertex_joints"] is None and check_body(body)["mesh"]["joint_maps"] == {}

    def with_(**kw):
        m = dict(body["mesh"], **regs)
        m.update(kw)
        return dict(body, mesh=m)

    ok = check_body(with_())["mesh"]
    assert ok["vertex_joints"].dtype == np.int32 and ok["J_regressor_extra"].dtype == np.float32 and set(ok["joint_maps"]) == set(TYPES)
    assert ok["map_roots"] == {"vibe": 8, "a2m": 0, "a2mpl": 0}
    again = check_body(dict(body, mesh=ok))["mesh"]                  # its own output is accepted
    assert all(np.array_equal(again["joint_maps"][t], ok["joint_maps"][t]) for t in TYPES)
    only = check_body(with_(joint_maps={"a2m": regs["joint_maps"]["a2m"]}))["mesh"]
    assert set(only["joint_maps"]) == {"a2m"}
    assert len(check_body(with_(vertex_joints=None, joint_maps={"a2m": np.array([0, 30])}))["mesh"]["vertex_joints"]) == 0      # Np = 0: 24 + 0 + 9 joints
    assert check_body(with_(J_regressor_extra=None, joint_maps={"a2m": np.array([0, 44])}))["mesh"]["J_regressor_extra"].shape == (0, 70)
    assert check_body(with_(map_roots=np.array([3, 1, 2])))["mesh"]["map_roots"] == {"vibe": 3, "a2m": 1, "a2mpl": 2}
    nan = regs["J_regressor_extra"].copy()
    nan[2, 5] = np.nan
    neg = -np.abs(regs["J_regressor_extra"]) * 7                     # rows need not be non-negative or sum to 1
    check_body(with_(J_regressor_extra=neg))
    for kw, text in ((dict(vertex_joints=np.array([0, 70])), "vertex_joints"), (dict(vertex_joints=np.array([-1])), "vertex_joints"),
                     (dict(vertex_joints=np.array([0.5])), "vertex_joints"), (dict(J_regressor_extra=regs["J_regressor_extra"][:, :69]), r"J_regressor_extra .* is not \[Jr, V\]"),
                     (dict(J_regressor_extra=nan), "not finite"), (dict(vertex_joints=np.zeros(0, np.int32), J_regressor_extra=np.zeros((0, 70)), joint_maps={}), "both empty"),
                     (dict(vertex_joints=np.arange(24)), "> 32"), (dict(joint_maps={"vibe": np.array([0, 54])}), "map_vibe"),
                     (dict(joint_maps={"a2m": np.array([-1])}), "map_a2m"), (dict(joint_maps={"a2m": np.zeros(0, np.int32)}), "map_a2m"),
                     (dict(joint_maps={"a2m": np.zeros(65, np.int32)}), "map_a2m"), (dict(joint_maps={"smpl": np.arange(24)}), "joint types"),
                     (dict(map_roots=np.array([49, 0, 0])), "map_roots"), (dict(map_roots=np.array([0, 0])), "map_roots"),
                     (dict(vertex_joints=None, J_regressor_extra=None), "without vertex_joints")):
        with pytest.raises(ValueError, match=text):
            check_body(with_(**kw))


def test_body_file_and_tool_round_trip(tmp_path):
    from regennet_amd.model.rotation2xyz import body_file_arrays, check_body, load_body, load_skeleton_or_body
    body = synth.make_body(24, 70, seed=24)
    regs = synth.make_joint_regressors(body)
    full = check_body(dict(body, mesh=dict(body["mesh"], **regs)))
    path = str(tmp_path / "body.npz")
    np.savez(path, **body_file_arrays(full))
    with np.load(path) as z:
        assert {"vertex_joints", "J_regressor_extra", "map_vibe", "map_a2m", "map_a2mpl", "map_roots"} <= set(z.files)
    got = load_skeleton_or_body(path)["mesh"]
    assert np.array_equal(got["vertex_joints"], regs["vertex_joints"]) and np.array_equal(got["J_regressor_extra"], regs["J_regressor_extra"])
    assert all(np.array_equal(got["joint_maps"][t], regs["joint_maps"][t]) for t in TYPES) and got["map_roots"] == regs["map_roots"]
    plain = str(tmp_path / "plain.npz")
    np.savez(plain, **body_file_arrays(check_body(body)))
    assert load_body(plain)["mesh"]["vertex_joints"] is None        # a body file without the keys loads as before
    # the tool: three option files beside a toy model file
    spec = importlib.util.spec_from_file_location("make_skeleton_tool", os.path.join(ROOT, "tools", "make_skeleton.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.Generator(np.random.PCG64(5))
    J, V = 7, 40
    jr = rng.uniform(0, 1, (J, V))
    jr /= jr.sum(1, keepdims=True)
    kt = np.array([[2 ** 32 - 1, 0, 0, 1, 2, 2, 5], np.arange(J)], dtype=np.uint32)
    w = rng.uniform(0, 1, (V, J))
    w /= w.sum(1, keepdims=True)
    src = str(tmp_path / "model.npz")
    np.savez(src, J_regressor=jr, v_template=rng.standard_normal((V, 3)), shapedirs=rng.standard_normal((V, 3, 12)), kintree_table=kt, weights=w,
             posedirs=rng.standard_normal((V, 3, 9 * (J - 1))))
    extra = rng.standard_normal((3, V)).astype(np.float32)
    np.save(str(tmp_path / "extra.npy"), extra)
    with open(tmp_path / "ids.txt", "w") as f:
        f.write("5 11, 39\n7\n")
    np.save(str(tmp_path / "ids.npy"), np.array([5, 11, 39, 7]))
    np.savez(str(tmp_path / "maps.npz"), vibe=np.array([0, 7, 13, 13]), a2m=np.array([0, 6]), roots=np.array([2, 1, 0]))
    outs = []
    for ids in ("ids.txt", "ids.npy"):
        out = str(tmp_path / (ids + ".body.npz"))
        tool.main([src, "--out", out, "--body_model", "toy", "--mesh", "--vertex_joints", str(tmp_path / ids), "--joint_regressor_extra",
                   str(tmp_path / "extra.npy"), "--joint_maps", str(tmp_path / "maps.npz")])
        outs.append(load_body(out)["mesh"])
    for m in outs:
        assert list(m["vertex_joints"]) == [5, 11, 39, 7] and np.array_equal(m["J_regressor_extra"], extra) and set(m["joint_maps"]) == {"vibe", "a2m"}
        assert list(m["joint_maps"]["vibe"]) == [0, 7, 13, 13] and m["map_roots"] == {"vibe": 2, "a2m": 1, "a2mpl": 0}
    np.savez(str(tmp_path / "bad.npz"), vibe=np.array([0, 14]))     # 7 + 4 + 3 = 14 joints: 14 is none of them
    with pytest.raises(ValueError, match="map_vibe"):
        tool.main([src, "--out", str(tmp_path / "x.npz"), "--mesh", "--vertex_joints", str(tmp_path / "ids.npy"), "--joint_regressor_extra",
                   str(tmp_path / "extra.npy"), "--joint_maps", str(tmp_path / "bad.npz")])
    with pytest.raises(SystemExit):
        tool.main([src, "--out", str(tmp_path / "x.npz"), "--vertex_joints", str(tmp_path / "ids.npy")])


def test_rotation2xyz_serves_the_types_only_over_a_body_that_holds_them():
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    from tests.test_rot2xyz_cpu import _model
    body = synth.make_body(4, 9)
    regs = synth.make_joint_regressors(body, npicks=3, nreg=2, support=4)
    x = torch.zeros(2, 5, 6, 8)
    kw = dict(mask=None, translation=True, glob=True, vertstrans=True, pose_rep="rot6d")
    plain = Rotation2xyz(body, model=_model())
    for jt in TYPES:                                                # a body without regressors: today's refusal
        with pytest.raises(NotImplementedError, match="vertices"):
            plain(x, jointstype=jt, **kw)
    part = Rotation2xyz(dict(body, mesh=dict(body["mesh"], **dict(regs, joint_maps={"vibe": regs["joint_maps"]["vibe"]}))), model=_model())
    with pytest.raises(NotImplementedError, match="map_a2m"):
        part(x, jointstype="a2m", **kw)
    with pytest.raises(NotImplementedError, match="map_a2mpl"):
        part(x, jointstype="a2mpl", **kw)
    with pytest.raises(ValueError, match=r"\[B, 5, 6, T\]"):       # served: it gets as far as the shape check in front of the device
        part(torch.zeros(2, 6, 6, 8), jointstype="vibe", **kw)
    with pytest.raises(NotImplementedError, match="vertices"):     # a skeleton file
        Rotation2xyz(synth.make_skeleton(4), model=_model())(x, jointstype="vibe", **kw)


def test_abi_symbols_and_argument_checks_without_a_device():
    """Every refusal that needs no body handle, with its text. A body handle cannot exist without a device, so what is judged against the body - a
    body without regressors, a map entry >= J + Np + Jr, a short workspace, a pick outside [0, V), a non-finite weight - is in
    tests/test_rot2joints_gpu.py::test_argument_errors_that_need_a_body (the host code behind the last two also in tools/joints_args_check.cpp)."""
    from regennet_amd import _lib
    lib = _lib.load()
    names = ("rgn_body_set_joint_regressors", "rgn_rot2joints_workspace", "rgn_rot2joints", "rgn_rot2joints_shaped_workspace", "rgn_rot2joints_shaped")
    header = open(os.path.join(ROOT, "include", "regennet_hip.h")).read()
    for name in names:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and f" {name}(" in header
    assert "rgn_*;" in open(os.path.join(ROOT, "regennet_amd", "csrc", "exports.map")).read()
    vp = ctypes.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)      # noqa: E731
    err = lambda: (lib.rgn_body_last_error(None) or b"").decode()   # noqa: E731
    dummy = np.zeros(64, np.float32)                                # stands for device memory: never read
    rest, par, gr = np.zeros((3, 3), np.float32), np.array([-1, 0, 1], np.int32), np.array([0.1, 0.2, 0.3], np.float32)
    good = dict(x=dummy, out=dummy, rest=rest, par=par, B=1, T=2, rep=0, P=1, flags=3, gr=None, jmap=np.array([0, 1, 1], np.int32), n=None, root=1,
                sj=dummy, nb=10, be=dummy, strides=(10, 0, 0))

    def call(shaped, **kw):
        a = dict(good, **kw)
        n = (0 if a["jmap"] is None else len(a["jmap"])) if a["n"] is None else a["n"]
        if shaped:
            rc = lib.rgn_rot2joints_shaped(None, p(a["x"]), None, a["B"], a["T"], p(a["rest"]), p(a["par"]), p(a["sj"]), a["nb"], p(a["be"]), *a["strides"], a["rep"],
                                           a["P"], a["flags"], p(a["gr"]), n, p(a["jmap"]), a["root"], p(a["out"]), None, None, 0, None)
        else:
            rc = lib.rgn_rot2joints(None, p(a["x"]), None, a["B"], a["T"], p(a["rest"]), p(a["par"]), a["rep"], a["P"], a["flags"], p(a["gr"]), None, n, p(a["jmap"]),
                                    a["root"], p(a["out"]), None, None, 0, None)
        return rc, err()

    common = [(dict(), "null handle"), (dict(x=None), "null x"), (dict(out=None), "null x"), (dict(rest=None), "null x"), (dict(par=None), "null x"),
              (dict(B=0), "B < 1"), (dict(T=0), "T < 1"), (dict(P=0), "num_person < 1"), (dict(rep=4), "unknown pose_rep"), (dict(flags=8), "unknown flag"),
              (dict(flags=1), "glob_rot is required"), (dict(flags=1, gr=gr), "null handle"), (dict(jmap=None, n=3), "null map"), (dict(n=0), "n_map outside [1, 64]"),
              (dict(jmap=np.zeros(65, np.int32)), "n_map outside [1, 64]"), (dict(jmap=np.zeros(64, np.int32)), "null handle"), (dict(root=3), "root outside [0, n_map)"),
              (dict(root=-1), "root outside [0, n_map)"), (dict(jmap=np.array([0, -2, 1], np.int32)), "map[1] < 0")]
    shaped_only = [(dict(sj=None), "null shape_joints_dev or betas_dev"), (dict(be=None), "null shape_joints_dev or betas_dev"), (dict(nb=0), "nb outside [1, 16]"),
                   (dict(nb=17), "nb outside [1, 16]"), (dict(strides=(-1, 0, 0)), "negative beta stride")]
    for shaped, fn in ((False, "rgn_rot2joints"), (True, "rgn_rot2joints_shaped")):
        for kw, text in common + (shaped_only if shaped else []):
            rc, e = call(shaped, **kw)
            assert rc == -1 and e.startswith(fn + ": ") and text in e, (fn, kw, rc, e)
    ids, reg = np.arange(4, dtype=np.int32), np.zeros((2, 8), np.float32)
    for args, text in (((4, p(ids), 2, p(reg)), "null handle"), ((-1, p(ids), 2, p(reg)), "Np or Jr < 0"), ((4, p(ids), -2, p(reg)), "Np or Jr < 0"),
                       ((0, None, 0, None), "both 0"), ((30, p(ids), 3, p(reg)), "Np + Jr = 33 > 32"), ((4, None, 2, p(reg)), "without vertex_joints"),
                       ((4, p(ids), 2, None), "without a regressor"), ((0, None, 2, p(reg)), "null handle"), ((4, p(ids), 0, None), "null handle")):
        rc = lib.rgn_body_set_joint_regressors(None, *args)
        assert rc == -1 and err().startswith("rgn_body_set_joint_regressors: ") and text in err(), (args, rc, err())
    n = ctypes.c_uint64()
    assert lib.rgn_rot2joints_workspace(None, 1, 1, 1, ctypes.byref(n)) == -1 and lib.rgn_rot2joints_shaped_workspace(None, 1, 1, 1, ctypes.byref(n)) == -1


def test_jointstype_option_parses_in_both_clis_and_needs_the_regressors(tmp_path):
    from regennet_amd.model.rotation2xyz import body_file_arrays, check_body
    from regennet_amd.sample.cgenerate import set_skeleton
    from regennet_amd.utils.parser_util import cgenerate_args, edit_args
    assert cgenerate_args(["--synthetic"]).jointstype == "" and edit_args(["--synthetic"]).jointstype == ""
    assert cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--jointstype", "a2m"]).jointstype == "a2m"
    assert edit_args(["--synthetic", "--skeleton", "body.npz", "--jointstype", "vibe"]).jointstype == "vibe"
    with pytest.raises(SystemExit):
        cgenerate_args(["--synthetic", "--jointstype", "smpl"])
    with pytest.raises(SystemExit, match="--jointstype needs --skeleton"):
        set_skeleton(None, cgenerate_args(["--synthetic", "--jointstype", "a2m"]))
    skel, plain, part = (str(tmp_path / n) for n in ("skel.npz", "plain.npz", "part.npz"))
    np.savez(skel, **synth.make_skeleton(24, seed=24))
    body = synth.make_body(24, 70, seed=24)
    np.savez(plain, **body_file_arrays(check_body(body)))
    regs = synth.make_joint_regressors(body)
    np.savez(part, **body_file_arrays(check_body(dict(body, mesh=dict(body["mesh"], **dict(regs, joint_maps={"vibe": regs["joint_maps"]["vibe"]}))))))
    for path, jt in ((skel, "a2m"), (plain, "a2m"), (part, "a2m")):
        with pytest.raises(SystemExit, match="--jointstype a2m: .* holds no joint regressors"):
            set_skeleton(None, cgenerate_args(["--synthetic", "--skeleton", path, "--jointstype", jt]))

    class Taker:
        njoints = 25

        def set_skeleton(self, sk):
            self.sk = sk

    taker = Taker()
    assert set_skeleton(taker, cgenerate_args(["--synthetic", "--skeleton", part, "--jointstype", "vibe"])) and len(taker.sk["mesh"]["joint_maps"]["vibe"]) == 49
    assert set_skeleton(taker, edit_args(["--synthetic", "--skeleton", "synthetic", "--jointstype", "a2mpl"])) and "a2mpl" in taker.sk["mesh"]["joint_maps"]
