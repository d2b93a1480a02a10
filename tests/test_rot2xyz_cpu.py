"""CPU: the rot2xyz restatement (tests/rot2xyz_ref.py) is pinned to goldens recorded from the reference's own wrappers
(tests/golden/make_golden_rot2xyz.py), and the host side of the feature - skeleton files, the extraction tool, the Python class's argument
handling, the CLI flag, the C entry point's NULL handling - behaves as specified. The kernel itself is tested in tests/test_rot2xyz_gpu.py."""
import glob
import importlib.util
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests.rot2xyz_ref import rot2xyz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "rot2xyz_*.npz")))


def golden_call(g, dtype, x=None):
    """The restatement on a golden's input and settings."""
    sk = {"rest_joints": g["rest_joints"], "parents": g["parents"], "shape_joints": g["shape_joints"]}
    return rot2xyz_ref(torch.from_numpy(g["x"]) if x is None else x, None if bool(g["mask_none"]) else torch.from_numpy(g["mask"]), sk,
                       str(g["pose_rep"]), bool(g["translation"]), bool(g["glob"]), bool(g["vertstrans"]), beta=float(g["beta"]),
                       glob_rot=None if bool(g["glob"]) else g["glob_rot"], num_person=int(g["num_person"]), dtype=dtype)


def test_the_recorded_cases_are_all_there():
    want = {"p1", "p2", "ragged", "p2_ragged", "notrans", "novertstrans", "noglob", "rotvec", "rotquat", "rotmat", "beta", "smpl24"}
    assert {n[len("rot2xyz_"):] for n in GOLDENS} == want


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_reference(golden, name):
    """fp64: the same arithmetic as the recorded run up to the association of the chain's products (1e-12 at |xyz| < 4). fp32: a chain of at
    most 10 levels with about 8 roundings each, relative to max|xyz| < 4: 10 * 8 * 2^-24 * 4 = 1.9e-5."""
    g = golden(name)
    exp = g["expected"]
    assert exp.dtype == np.float64 and float(np.abs(exp).max()) < 4.0
    e64 = float(np.abs(golden_call(g, torch.float64).numpy() - exp).max())
    e32 = float(np.abs(golden_call(g, torch.float32).double().numpy() - exp).max())
    print(f"{name}: fp64 {e64:.2e}  fp32 {e32:.2e}")
    assert e64 < 1e-12, e64
    assert e32 < 1.9e-5, e32


def test_masked_frames_hold_the_translation_term_alone(golden):
    g = golden("rot2xyz_ragged")
    exp, x, m = g["expected"], g["x"].astype(np.float64), g["mask"]
    tr = x[:, -1, :3, :] - x[:, -1, :3, :1]                       # one person: relative to frame 0 (rotation2xyz.py:318)
    for b, t in zip(*np.nonzero(~m)):
        assert np.array_equal(exp[b, :, :, t], np.broadcast_to(tr[b, :, t], exp[b, :, :, t].shape))
    g2 = golden("rot2xyz_p2_ragged")
    x2 = g2["x"].astype(np.float64)
    for b, t in zip(*np.nonzero(~g2["mask"])):                      # two persons: the row as stored (:247-249)
        for p in range(2):
            assert np.array_equal(g2["expected"][b, :, 3 * p:3 * p + 3, t], np.broadcast_to(x2[b, -1, 6 * p:6 * p + 3, t], (55, 3)))


def test_synthetic_skeleton_is_a_55_joint_tree_of_depth_10():
    sk = synth.make_skeleton()
    p = sk["parents"]
    assert p.shape == (55,) and p[0] == -1 and all(0 <= p[i] < i for i in range(1, 55))
    depth = np.zeros(55, int)
    for i in range(1, 55):
        depth[i] = depth[p[i]] + 1
    assert depth.max() == 10 and "synthetic" in sk["body_model"]
    assert sk["rest_joints"].shape == (55, 3) and sk["shape_joints"].shape == (55, 3, 10)
    again = synth.make_skeleton()
    assert all(np.array_equal(sk[k], again[k]) for k in ("rest_joints", "parents", "shape_joints"))
    assert len(synth.make_skeleton(24)["parents"]) == 24 and list(synth.make_skeleton(1)["parents"]) == [-1]


def test_skeleton_file_round_trip_and_validation(tmp_path):
    from regennet_amd.model.rotation2xyz import check_skeleton, load_skeleton
    sk = synth.make_skeleton()
    path = str(tmp_path / "skel.npz")
    np.savez(path, **sk)
    got = load_skeleton(path)
    assert np.array_equal(got["rest_joints"], sk["rest_joints"].astype(np.float64)) and np.array_equal(got["parents"], sk["parents"])
    assert got["shape_joints"].shape == (55, 3, 10) and got["body_model"] == "synthetic55"
    np.savez(path, rest_joints=sk["rest_joints"], parents=sk["parents"])
    assert load_skeleton(path)["shape_joints"] is None
    bad = dict(sk, parents=sk["parents"].copy())
    bad["parents"][3] = 7
    with pytest.raises(ValueError, match="parents"):
        check_skeleton(bad)
    with pytest.raises(ValueError, match="J <= 64"):
        check_skeleton({"rest_joints": np.zeros((65, 3)), "parents": np.arange(-1, 64)})


def test_make_skeleton_tool_regresses_the_joints_of_a_model_file(tmp_path):
    spec = importlib.util.spec_from_file_location("make_skeleton_tool", os.path.join(ROOT, "tools", "make_skeleton.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.Generator(np.random.PCG64(5))
    J, V = 7, 40
    reg = rng.uniform(0, 1, (J, V))
    reg /= reg.sum(1, keepdims=True)
    vt, sd = rng.standard_normal((V, 3)), rng.standard_normal((V, 3, 12))
    kt = np.array([[2 ** 32 - 1, 0, 0, 1, 2, 2, 5], np.arange(J)], dtype=np.uint32)
    src, out = str(tmp_path / "model.npz"), str(tmp_path / "skel.npz")
    np.savez(src, J_regressor=reg, v_template=vt, shapedirs=sd, kintree_table=kt, unrelated=np.zeros(3))
    tool.main([src, "--out", out, "--body_model", "toy"])
    from regennet_amd.model.rotation2xyz import load_skeleton
    sk = load_skeleton(out)
    assert list(sk["parents"]) == [-1, 0, 0, 1, 2, 2, 5] and sk["body_model"] == "toy"
    assert np.allclose(sk["rest_joints"], reg @ vt, atol=1e-6)
    assert sk["shape_joints"].shape == (J, 3, 10)
    assert np.allclose(sk["shape_joints"][:, :, 4], reg @ sd[:, :, 4], atol=1e-6)


def _model(cfg_name="tiny", **kw):
    from regennet_amd.model.cmdm import CMDM
    cfg = synth.get_config(cfg_name)
    return CMDM("", cfg["njoints"], cfg["nfeats"], cfg["num_actions"], True, "rot6d", True, True, num_frames=cfg["num_frames"],
                latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["layers"], num_heads=cfg["num_heads"], arch="online",
                cm_mode=cfg["cm_mode"], body_model="smplx", cond_mode=cfg["cond_mode"], cond_mask_prob=cfg["cond_mask_prob"], dataset="ntu", **kw)


def test_rotation2xyz_argument_handling():
    """What needs no device: 'xyz' passes through, the vertex joint types and unknown names raise NotImplementedError, a missing glob_rot
    TypeError, differing beta rows NotImplementedError, a shape that does not fit the skeleton ValueError."""
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    sk = synth.make_skeleton(4)
    r2x = Rotation2xyz(sk, model=_model())
    x = torch.zeros(2, 5, 6, 8)
    kw = dict(mask=None, translation=True, glob=True, vertstrans=True)
    assert r2x(x, pose_rep="xyz", jointstype="smplx", **kw) is x
    for jt in ("vertices", "vibe", "a2m", "a2mpl"):
        with pytest.raises(NotImplementedError, match="vertices"):
            r2x(x, pose_rep="rot6d", jointstype=jt, **kw)
    with pytest.raises(NotImplementedError, match="not implemented"):
        r2x(x, pose_rep="rot6d", jointstype="openpose", **kw)
    with pytest.raises(NotImplementedError, match="No geometry"):
        r2x(x, pose_rep="euler", jointstype="smplx", **kw)
    with pytest.raises(TypeError, match="global rotation"):
        r2x(x, None, "rot6d", True, False, "smplx", True)
    with pytest.raises(ValueError, match=r"\[B, 5, 6, T\]"):
        r2x(torch.zeros(2, 6, 6, 8), pose_rep="rot6d", jointstype="smplx", get_rotations_back=False, some_extra=1, **kw)
    with pytest.raises(NotImplementedError, match="per-row betas"):
        r2x.rest_joints(betas=torch.tensor([[0.0, 1.0], [0.0, 2.0]]))
    assert np.array_equal(r2x.rest_joints(), sk["rest_joints"].astype(np.float64))
    want = sk["rest_joints"].astype(np.float64) + 1.5 * sk["shape_joints"][:, :, 1].astype(np.float64)
    assert np.allclose(r2x.rest_joints(beta=1.5), want, atol=1e-15)
    assert np.allclose(r2x.rest_joints(betas=torch.tensor([[0.0, 1.5, 0.0]] * 3)), want, atol=1e-15)


def test_cmdm_skeleton_and_the_guidance_wrapper_follow_set_skeleton():
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from regennet_amd.model.cmdm import _Rot2xyzUnavailable
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    model = _model()
    assert isinstance(model.rot2xyz, _Rot2xyzUnavailable)
    with pytest.raises(NotImplementedError, match="skeleton"):
        model.rot2xyz(x=None)
    wrapped = ClassifierFreeSampleModel(model)
    assert isinstance(wrapped.rot2xyz, _Rot2xyzUnavailable)
    model.set_skeleton(synth.make_skeleton(4))                    # after wrapping
    assert isinstance(model.rot2xyz, Rotation2xyz) and wrapped.rot2xyz is model.rot2xyz
    assert isinstance(_model(skeleton=synth.make_skeleton(4)).rot2xyz, Rotation2xyz)
    model.set_skeleton(None)
    assert isinstance(wrapped.rot2xyz, _Rot2xyzUnavailable)


def test_skeleton_flag_parses_in_both_clis():
    from regennet_amd.utils.parser_util import cgenerate_args, edit_args
    assert cgenerate_args(["--synthetic"]).skeleton == ""
    assert cgenerate_args(["--synthetic", "--skeleton", "synthetic"]).skeleton == "synthetic"
    assert edit_args(["--synthetic", "--skeleton", "skel.npz"]).skeleton == "skel.npz"


def test_rgn_rot2xyz_null_handle_returns_invalid_arg():
    from regennet_amd import _lib
    lib = _lib.load()
    assert lib.rgn_rot2xyz(None, None, None, 1, 1, 1, None, None, 0, 1, 0, None, None, None, None) == -1
