"""CPU: the per-frame-shape restatement (tests/rot2xyz_shaped_ref.py) is pinned to goldens recorded from the reference's own wrappers given a `betas`
row per unmasked frame (tests/golden/make_golden_rot2xyz_shaped.py), and the host side of the feature - the two entry points' argument checks, the
wrapper's routing of `betas` / `betas_per_motion`, the --betas_npz options - behaves as specified. The kernels are tested in
tests/test_rot2xyz_shaped_gpu.py.

On the commit before the feature the symbol, wrapper and option tests fail: the symbols do not exist, Rotation2xyz takes no betas_per_motion and
raises NotImplementedError for differing rows, and neither CLI knows --betas_npz."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests.rot2verts_ref import golden_body
from tests.rot2xyz_shaped_ref import expand_betas, rows_to_frames, shaped_ref
from tests.test_rot2xyz_cpu import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("p1_ragged", "p2_ragged", "smpl24", "noglob_rotvec", "nb3")
GOLDENS = [f"shaped_{k}_{c}" for k in ("rot2xyz", "rot2verts") for c in CASES]


def test_the_recorded_cases_are_all_there():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "shaped_*.npz")))
    assert have == sorted(GOLDENS)
    assert all(os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) < 200 * 1024 for n in GOLDENS)


def golden_call(g):
    mask = None if bool(g["mask_none"]) else g["mask"]
    B, T, P = g["x"].shape[0], g["x"].shape[-1], int(g["num_person"])
    kw = dict(pose_rep=str(g["pose_rep"]), translation=bool(g["translation"]), glob=bool(g["glob"]), vertstrans=bool(g["vertstrans"]),
              glob_rot=None if bool(g["glob"]) else g["glob_rot"], num_person=P, vertices=str(g["jointstype"]) == "vertices")
    return mask, rows_to_frames(g["betas"], mask, B, T, P), kw


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_reference(golden, name):
    """The bound tests/test_rot2verts_cpu.py holds its restatement to: fp64 within 1e-12 of the recorded run; fp32 within the deviation the
    recorder measured and stored (fp32_dev), which itself stays below 1e-5 at |xyz| < 4."""
    g = golden(name)
    exp, body = g["expected"], golden_body(g)
    mask, bt, kw = golden_call(g)
    assert g["betas"].shape == (int(g["mask"].sum()), 3 if name.endswith("nb3") else 10) and len(np.unique(g["betas"], axis=0)) == len(g["betas"])
    assert exp.dtype == np.float64 and float(np.abs(exp).max()) < 4.0 and float(g["fp32_dev"]) <= 1e-5
    m = None if mask is None else torch.from_numpy(mask)
    e64 = float(np.abs(shaped_ref(g["x"], m, body, bt, dtype=torch.float64, **kw).numpy() - exp).max())
    e32 = float(np.abs(shaped_ref(g["x"], m, body, bt, dtype=torch.float32, **kw).double().numpy() - exp).max())
    print(f"{name}: fp64 {e64:.2e}  fp32 {e32:.2e}  recorded fp32_dev {float(g['fp32_dev']):.2e}")
    assert e64 < 1e-12, e64
    assert e32 <= float(g["fp32_dev"]), (e32, float(g["fp32_dev"]))


def test_zero_betas_are_the_one_shape_restatements(golden):
    from tests.rot2verts_ref import rot2verts_ref
    from tests.rot2xyz_ref import rot2xyz_ref
    g = golden("shaped_rot2verts_p2_ragged")
    body = golden_body(g)
    mask, bt, kw = golden_call(g)
    one = dict(kw)
    del one["vertices"]
    m = torch.from_numpy(mask)
    zero = np.zeros_like(bt)
    assert float((shaped_ref(g["x"], m, body, zero, **dict(kw, vertices=False)) - rot2xyz_ref(g["x"], m, body, **one)).abs().max()) < 1e-12
    assert float((shaped_ref(g["x"], m, body, zero, **kw) - rot2verts_ref(g["x"], m, body, **one)).abs().max()) < 1e-12


def test_a_shape_per_person_is_two_one_person_runs(golden):
    """What the reference's interface cannot express, against what it can: persons are independent, so two persons with a shape each are the two
    one-person runs side by side (without vertstrans: the one-person translation term is relative to frame 0, :318)."""
    g = golden("shaped_rot2verts_p2_ragged")
    body = golden_body(g)
    mask, _, kw = golden_call(g)
    B, T = g["x"].shape[0], g["x"].shape[-1]
    rng = np.random.Generator(np.random.PCG64(3))
    bt = expand_betas(rng.standard_normal((B, 2, 10)), B, 2, T)
    m = torch.from_numpy(mask)
    for vertices in (False, True):
        kw2 = dict(kw, vertices=vertices, vertstrans=False)
        both = shaped_ref(g["x"], m, body, bt, **kw2)
        for p in range(2):
            one = shaped_ref(g["x"][:, :, 6 * p:6 * p + 6], m, body, bt[:, p:p + 1], **dict(kw2, num_person=1))
            assert torch.equal(both[:, :, 3 * p:3 * p + 3], one)
        assert float((both[:, :, :3] - both[:, :, 3:]).abs().max()) > 1e-3


def _dummy():
    buf = (ctypes.c_float * 4)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_both_entry_points_refuse_bad_arguments_before_a_handle_or_a_device():
    """Every new refusal, and the siblings' own, with a NULL handle: RGN_ERR_INVALID_ARG and its text (tools/shaped_args_check.cpp runs the same
    list under the host sanitizers)."""
    from regennet_amd import _lib
    lib = _lib.load()
    keep, dev = _dummy()
    rest = np.zeros((3, 3), np.float32)
    chain = np.array([-1, 0, 1], np.int32)
    gr = np.zeros(3, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    ok = dict(x=dev, out=dev, rest=rest, par=chain, sj=dev, betas=dev, nb=10, sb=10, sp=0, st=0, B=1, T=2, J=3, rep=0, P=1, flags=3, gr=None)

    def joints(a):
        rc = lib.rgn_rot2xyz_shaped(None, a["x"], None, a["B"], a["T"], a["J"], p(a["rest"]), p(a["par"]), a["sj"], a["nb"], a["betas"], a["sb"], a["sp"],
                                    a["st"], a["rep"], a["P"], a["flags"], p(a["gr"]), a["out"], None, None)
        return rc, (lib.rgn_last_error(None) or b"").decode()

    def verts(a):
        rc = lib.rgn_rot2verts_shaped(None, a["x"], None, a["B"], a["T"], p(a["rest"]), p(a["par"]), a["sj"], a["nb"], a["betas"], a["sb"], a["sp"], a["st"],
                                      a["rep"], a["P"], a["flags"], p(a["gr"]), a["out"], None, None, 0, None)
        return rc, (lib.rgn_body_last_error(None) or b"").decode()

    both = [({}, "null handle"), (dict(x=None), "null x"), (dict(out=None), "null x"), (dict(rest=None), "null x"), (dict(par=None), "null x"),
            (dict(sj=None), "null shape_joints_dev or betas_dev"), (dict(betas=None), "null shape_joints_dev or betas_dev"),
            (dict(nb=0), "nb outside [1, 16]"), (dict(nb=17), "nb outside [1, 16]"), (dict(nb=-1), "nb outside [1, 16]"), (dict(nb=16), "null handle"),
            (dict(sb=-1), "negative beta stride"), (dict(sp=-1), "negative beta stride"), (dict(st=-1), "negative beta stride"),
            (dict(sb=0), "null handle"), (dict(B=0), "B < 1"), (dict(T=0), "T < 1"), (dict(P=0), "num_person < 1"), (dict(rep=4), "unknown pose_rep"),
            (dict(flags=8), "unknown flag"), (dict(flags=1), "glob_rot is required"), (dict(flags=1, gr=gr), "null handle")]
    for kw, text in both:
        for fn, call in (("rgn_rot2xyz_shaped", joints), ("rgn_rot2verts_shaped", verts)):
            rc, err = call(dict(ok, **kw))
            assert rc == -1 and err.startswith(fn + ": ") and text in err, (fn, kw, rc, err)
    for kw, text in [(dict(J=0), "J outside [1, 64]"), (dict(J=65), "J outside [1, 64]"), (dict(par=np.array([0, 0, 1], np.int32)), "parents[0] != -1"),
                     (dict(par=np.array([-1, 1, 1], np.int32)), "parents[1]"), (dict(par=np.array([-1, 0, -1], np.int32)), "parents[2]")]:
        rc, err = joints(dict(ok, **kw))                            # (the vertices call takes J from its handle)
        assert rc == -1 and err.startswith("rgn_rot2xyz_shaped: ") and text in err, (kw, rc, err)
    n = ctypes.c_uint64()
    assert lib.rgn_rot2verts_shaped_workspace(None, 1, 2, 1, ctypes.byref(n)) == -1
    del keep


def test_the_new_symbols_are_bound():
    from regennet_amd import _lib
    assert len(_lib.SYMBOLS["rgn_rot2xyz_shaped"][1]) == 21 and len(_lib.SYMBOLS["rgn_rot2verts_shaped"][1]) == 22
    assert "rgn_rot2verts_shaped_workspace" in _lib.SYMBOLS


def test_wrapper_routes_and_refuses_on_the_host():
    """What needs no device: which route a call's shape arguments take, and every refusal."""
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    sk = synth.make_skeleton(4)
    r2x = Rotation2xyz(sk, model=_model())
    B, T = 2, 8
    x = torch.zeros(B, 5, 6, T)
    kw = dict(pose_rep="rot6d", translation=True, glob=True, vertstrans=True, jointstype="smplx")
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 3:] = False
    rows = torch.arange(11 * 10, dtype=torch.float32).reshape(11, 10)
    assert r2x.shape_plan(None, 0, None, mask, B, T, 1) is None and r2x.shape_plan(None, 1.5, None, mask, B, T, 1) is None
    assert r2x.shape_plan(rows[0], 0, None, mask, B, T, 1) is None and r2x.shape_plan(rows[:1].repeat(5, 1), 0, None, mask, B, T, 1) is None
    kind, got = r2x.shape_plan(rows, 0, None, mask, B, T, 1)
    assert kind == "frames" and torch.equal(got, rows)
    assert r2x.shape_plan(torch.randn(16, 3), 0, None, None, B, T, 2)[0] == "frames"                     # mask=None: B T rows; fewer betas than the file's
    assert r2x.shape_plan(None, 0, torch.randn(B, 10), mask, B, T, 2)[0] == "motions"
    assert r2x.shape_plan(None, 0, np.zeros((B, 2, 4), np.float32), mask, B, T, 2)[0] == "motions"
    with pytest.raises(ValueError, match="mutually exclusive"):
        r2x(x, mask, betas=rows, betas_per_motion=torch.zeros(B, 10), **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        r2x(x, mask, beta=1.5, betas_per_motion=torch.zeros(B, 10), **kw)
    with pytest.raises(ValueError, match="betas has 10 rows, but the mask leaves 11 frames"):
        r2x(x, mask, betas=rows[:10], **kw)
    with pytest.raises(ValueError, match="betas has 11 rows, but the mask leaves 16 frames"):
        r2x(x, None, betas=rows, **kw)
    with pytest.raises(ValueError, match="11 betas but the skeleton file holds 10"):
        r2x(x, mask, betas=torch.randn(11, 11), **kw)
    with pytest.raises(ValueError, match="11 betas but the skeleton file holds 10"):
        r2x(x, mask, betas_per_motion=torch.randn(B, 11), **kw)
    for bad in (torch.zeros(10), torch.zeros(B + 1, 10), torch.zeros(B, 2, 10), torch.zeros(B, 1, T, 10)):
        with pytest.raises(ValueError, match="betas_per_motion"):
            r2x(x, mask, betas_per_motion=bad, **kw)
    bare = Rotation2xyz({k: v for k, v in sk.items() if k != "shape_joints"}, model=_model())
    with pytest.raises(ValueError, match="shape_joints"):
        bare(x, mask, betas=rows, **kw)
    with pytest.raises(ValueError, match="shape_joints"):
        bare(x, mask, betas_per_motion=torch.zeros(B, 10), **kw)
    with pytest.raises(NotImplementedError, match="per-row betas"):              # (the one-shape helpers keep their refusal)
        r2x.betas_vector(rows)
    body = synth.make_body(4, 20)
    noshape = Rotation2xyz(dict(body, mesh=dict(body["mesh"], shapedirs=None)), model=_model())
    with pytest.raises(ValueError, match="shapedirs"):
        noshape(x, mask, **dict(kw, jointstype="vertices", betas_per_motion=torch.zeros(B, 10)))


def test_betas_npz_options_parse_and_load(tmp_path):
    from regennet_amd.sample import cgenerate, render
    from regennet_amd.utils.parser_util import cgenerate_args
    assert cgenerate_args(["--synthetic"]).betas_npz == ""
    args = cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--betas_npz", "synthetic", "--seed", "7"])
    assert args.betas_npz == "synthetic"
    a, b = cgenerate.load_betas(args, 3, 10), cgenerate.load_betas(args, 3, 10)
    assert a.shape == (3, 10) and a.dtype == np.float32 and np.array_equal(a, b) and len(np.unique(a, axis=0)) == 3
    assert cgenerate.load_betas(cgenerate_args(["--synthetic"]), 3, 10) is None
    with pytest.raises(SystemExit, match="--skeleton"):
        cgenerate.load_betas(cgenerate_args(["--synthetic", "--betas_npz", "synthetic"]), 3, 10)
    path = str(tmp_path / "betas.npz")
    np.savez(path, betas=np.arange(8, dtype=np.float64).reshape(2, 4))
    got = cgenerate.load_betas(cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--betas_npz", path]), 5, 10)
    assert got.dtype == np.float32 and np.array_equal(got, np.arange(8).reshape(2, 4))
    for bad in (np.zeros((2, 11)), np.zeros(10), np.zeros((0, 10))):
        np.savez(path, betas=bad)
        with pytest.raises(SystemExit, match="betas"):
            cgenerate.load_betas(cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--betas_npz", path]), 5, 10)
    np.savez(path, shapes=np.zeros((2, 10)))
    with pytest.raises(SystemExit, match="holds no 'betas'"):
        cgenerate.load_betas(cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--betas_npz", path]), 5, 10)
    # render: [N, 2, nb], actor then reactor; one person is the reactor alone
    pair = np.arange(2 * 2 * 3, dtype=np.float32).reshape(2, 2, 3)
    np.savez(path, betas=pair)
    assert np.array_equal(render.load_betas(path, 4, 10, 2), pair) and np.array_equal(render.load_betas(path, 4, 10, 1), pair[:, 1:])
    assert render.load_betas("", 4, 10, 2) is None and render.load_betas("synthetic", 4, 10, 2).shape == (4, 2, 10)
    np.savez(path, betas=np.zeros((2, 10)))
    with pytest.raises(SystemExit, match=r"\[N, 2, nb\]"):
        render.load_betas(path, 4, 10, 2)
