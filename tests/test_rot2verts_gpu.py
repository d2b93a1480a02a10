"""GPU: rgn_rot2verts (csrc/rgn_lbs.hip) against the fp64 restatement that tests/test_rot2verts_cpu.py pins to the reference.

Bound, per case, as for the joints (tests/test_rot2xyz_gpu.py): the fp32 run of the SAME restatement - whose two long sums run term by term in
index order, the order class of the fp32-input MFMA - deviates from its fp64 run by some maximum d, computed here and never taken from the kernel.
The kernel may associate the short products (3x3 chain, applying the blended transform) differently, the same order of error again in either
direction, so it must stay within 4 d; where d is 0, one fp32 spacing at the case's largest |xyz|.
REGENNET_ROT2VERTS_TABLE=<file> writes the measured table (profiles/rot2verts_parity.txt).

On the commit before the feature every test here fails: _lib has no BodyEngine (the rgn_body_* / rgn_rot2verts symbols do not exist) and
Rotation2xyz refuses 'vertices' whatever dict it is given."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests.rot2verts_ref import golden_body, golden_settings, rot2verts_ref
from tests.test_rot2xyz_gpu import make_mask, make_x, run_kernel as run_joints, skeleton

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "rot2verts_*.npz")))
TABLE = []


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    if TABLE and os.environ.get("REGENNET_ROT2VERTS_TABLE"):
        with open(os.environ["REGENNET_ROT2VERTS_TABLE"], "w") as f:
            f.write(f"rgn_rot2verts on {torch.cuda.get_device_name(0)}: max |kernel - fp64 restatement| against the bound 4 x max |fp32 restatement - fp64 restatement|\n")
            f.write(f"{'case':72s} {'max|xyz|':>9s} {'fp32 ref':>10s} {'bound':>10s} {'kernel':>10s}\n")
            for row in TABLE:
                f.write("%-72s %9.3f %10.3e %10.3e %10.3e\n" % row)


@pytest.fixture(scope="module")
def tiny():
    """One tiny model on the GPU, for the calls that go through a model (and for rgn_rot2xyz, to compare with)."""
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    return cfg, model, diffusion, eng


def make_body(kind, V):
    """synth.make_body's surface over the skeletons of tests/test_rot2xyz_gpu.py: 'one', 'pair', 'tree24', 'tree55', 'chain64'."""
    if kind == "pair":
        return synth.make_body(2, V, seed=2)
    J, seed = {"one": (1, 0), "tree24": (24, 24), "tree55": (55, 0), "chain64": (64, 3)}[kind]
    body = synth.make_body(J, V, seed=seed)
    sk = skeleton(kind)
    if kind == "chain64":                                           # (the weights name joints, not bones: any tree of 64 joints carries the surface)
        body.update(rest_joints=sk["rest_joints"], parents=sk["parents"], shape_joints=sk["shape_joints"])
    assert np.array_equal(body["parents"], sk["parents"]) and np.array_equal(body["rest_joints"], sk["rest_joints"])
    return body


def cut(body, n):
    """The body reduced to its first n vertices."""
    m = body["mesh"]
    V = m["v_template"].shape[0]
    pd = None if m["posedirs"] is None else np.ascontiguousarray(m["posedirs"].reshape(-1, V, 3)[:, :n].reshape(-1, 3 * n))
    return dict(body, mesh=dict(m, v_template=m["v_template"][:n], posedirs=pd, lbs_weights=m["lbs_weights"][:n], shapedirs=m["shapedirs"][:n],
                                faces=None))


def run_kernel(body, x, mask, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, P=1, glob_rot=None, beta=0, want_rot=False, graph=False):
    """BodyEngine.rot2verts on numpy inputs -> numpy vertices (and the rotmat tensor); graph: eager, then captured and replayed -> both."""
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    eng = _lib.BodyEngine(body["mesh"], len(body["parents"]), 0)
    try:
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        md = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        B, T, J, V = x.shape[0], x.shape[-1], len(body["parents"]), body["mesh"]["v_template"].shape[0]
        out = torch.full((B, V, 3 * P, T), float("nan"), device="cuda")
        rot = torch.full((B, P, T, J, 3, 3), float("nan"), device="cuda") if want_rot else None
        work = torch.empty(eng.workspace_bytes(B, T, P), dtype=torch.uint8, device="cuda")
        flags = (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)
        betas = None
        if beta:
            betas = np.zeros(eng.nb, np.float32)
            betas[1] = beta
        rest = Rotation2xyz(body).rest_joints(beta=beta)

        def call():
            eng.rot2verts(xd, md, rest, body["parents"], _lib.POSE_REP[pose_rep], P, flags, glob_rot, betas, out, rot, work, torch.cuda.current_stream().cuda_stream)

        call()
        torch.cuda.synchronize()
        eager = out.cpu().numpy()
        if graph:
            out.fill_(float("nan"))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call()
            g.replay()
            torch.cuda.synchronize()
            return eager, out.cpu().numpy()
        return (eager, rot) if want_rot else eager
    finally:
        eng.close()


def check(label, got, x, mask, body, **kw):
    """got within 4 x (fp32 restatement's deviation from the fp64 one), both computed here on the same inputs."""
    ref_kw = dict(pose_rep=kw.get("pose_rep", "rot6d"), translation=kw.get("translation", True), glob=kw.get("glob", True),
                  vertstrans=kw.get("vertstrans", True), glob_rot=kw.get("glob_rot"), num_person=kw.get("P", 1), beta=kw.get("beta", 0))
    m = None if mask is None else torch.from_numpy(mask)
    r64 = rot2verts_ref(torch.from_numpy(x), m, body, dtype=torch.float64, **ref_kw).numpy()
    r32 = rot2verts_ref(torch.from_numpy(x), m, body, dtype=torch.float32, **ref_kw).double().numpy()
    d = float(np.abs(r32 - r64).max())
    top = float(np.abs(r64).max())
    bound = 4 * d if d > 0 else float(np.spacing(np.float32(top)))
    assert got.shape == r64.shape and np.isfinite(got).all(), (label, got.shape, r64.shape)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    TABLE.append((label, top, d, bound, err))
    print(f"{label}: max|xyz| {top:.3f}  fp32 ref {d:.3e}  bound {bound:.3e}  kernel {err:.3e}")
    assert err <= bound, (label, err, bound)
    return r64


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(golden, name):
    g = golden(name)
    body, s = golden_body(g), golden_settings(g)
    kw = dict(pose_rep=s["pose_rep"], translation=s["translation"], glob=s["glob"], vertstrans=s["vertstrans"], P=s["num_person"], glob_rot=s["glob_rot"],
              beta=s["beta"])
    mask = None if bool(g["mask_none"]) else g["mask"]
    r64 = check(name, run_kernel(body, g["x"], mask, **kw), g["x"], mask, body, **kw)
    assert float(np.abs(r64 - g["expected"]).max()) < 1e-12          # (the restatement is the recorded reference run)


# (B, T) x persons; V, skeleton and mask cycle so that every value of each axis appears
SHAPES = [(1, 1), (3, 7), (2, 61), (5, 64), (1, 150)]
VERTS = [1, 63, 64, 65, 130, 1000]
SKELETONS = ["one", "pair", "tree24", "tree55", "chain64"]
MASKS = ["none", "true", "ragged", "false"]
RANDOM = [(B, T, P, VERTS[(2 * i + P - 1) % 6], SKELETONS[(2 * i + P + 1) % 5], MASKS[(2 * i + P - 1) % 4]) for i, (B, T) in enumerate(SHAPES) for P in (1, 2)]
assert {c[3] for c in RANDOM} == set(VERTS) and {c[4] for c in RANDOM} == set(SKELETONS) and {c[5] for c in RANDOM} == set(MASKS)


@pytest.mark.parametrize("B,T,P,V,skel,mask_kind", RANDOM)
def test_random_cases(B, T, P, V, skel, mask_kind):
    body = make_body(skel, V)
    J = len(body["parents"])
    rng = np.random.Generator(np.random.PCG64(B * 1000 + T * 10 + P))
    mask = make_mask(mask_kind, B, T, rng)
    x = make_x(rng, B, T, J, "rot6d", True, True, P)
    check(f"B{B} T{T} P{P} V{V} {skel} mask={mask_kind}", run_kernel(body, x, mask, P=P), x, mask, body, P=P)


def test_a_body_without_posedirs():
    body = make_body("tree55", 130)
    body["mesh"]["posedirs"] = None
    rng = np.random.Generator(np.random.PCG64(5))
    mask = make_mask("ragged", 3, 7, rng)
    x = make_x(rng, 3, 7, 55, "rot6d", True, True, 1)
    check("B3 T7 P1 V130 tree55 no posedirs", run_kernel(body, x, mask), x, mask, body)


@pytest.mark.parametrize("pose_rep,translation,glob,vertstrans", [("rotvec", True, True, True), ("rotquat", True, False, True), ("rotmat", False, True, True),
                                                                   ("rot6d", True, True, False), ("rot6d", False, False, True), ("rotvec", True, False, False)])
def test_random_settings(pose_rep, translation, glob, vertstrans):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(77))
    B, T, P = 2, 61, 2
    mask = make_mask("ragged", B, T, rng)
    x = make_x(rng, B, T, 55, pose_rep, translation, glob, P)
    kw = dict(pose_rep=pose_rep, translation=translation, glob=glob, vertstrans=vertstrans, P=P, glob_rot=None if glob else np.array([0.3, -2.0, 1.1], np.float32))
    check(f"B2 T61 P2 V130 tree55 {pose_rep} trans={int(translation)} glob={int(glob)} vertstrans={int(vertstrans)}", run_kernel(body, x, mask, **kw), x, mask, body, **kw)


def test_real_size_once():
    """SMPL-X's size: 10475 vertices, 55 joints (328 vertex tiles, the last one partial; 8 tiles per workgroup)."""
    body = synth.make_body(55, 10475)
    rng = np.random.Generator(np.random.PCG64(8))
    x = make_x(rng, 2, 60, 55, "rot6d", True, True, 1)
    mask = make_mask("ragged", 2, 60, rng)
    check("B2 T60 P1 V10475 tree55 mask=ragged beta=1.5", run_kernel(body, x, mask, beta=1.5), x, mask, body, beta=1.5)


def test_rows_do_not_depend_on_the_batch():
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(12))
    for P in (1, 2):
        x = make_x(rng, 5, 64, 55, "rot6d", True, True, P)
        mask = make_mask("ragged", 5, 64, rng)
        full = run_kernel(body, x, mask, P=P)
        for b in (0, 3, 4):
            one = run_kernel(body, x[b:b + 1], mask[b:b + 1], P=P)
            assert np.array_equal(full[b:b + 1].view(np.int32), one.view(np.int32)), (P, b)


def test_a_vertex_does_not_depend_on_the_other_vertices():
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(13))
    x = make_x(rng, 3, 7, 55, "rot6d", True, True, 1)
    full = run_kernel(body, x, None, beta=1.5)
    part = run_kernel(cut(body, 64), x, None, beta=1.5)
    assert part.shape == (3, 64, 3, 7) and np.array_equal(full[:, :64].view(np.int32), part.view(np.int32))


def test_rotmat_output_is_rgn_rot2xyz_bit_for_bit(tiny):
    eng = tiny[3]
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(11))
    B, T, P = 2, 61, 2
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    x[0, 4] = 0
    mask = make_mask("ragged", B, T, rng)
    _, rot = run_kernel(body, x, mask, P=P, want_rot=True)
    _, want = run_joints(eng, x, mask, body, P=P, want_rot=True)
    assert torch.equal(rot.view(torch.int32), want.view(torch.int32))          # (also for joints 22 - 24: the matrices as given, not the identity the chain used)


def test_one_hot_vertices_on_the_joints_are_the_joints_kernel(tiny):
    """Vertex j with weight 1 on joint j, resting on it, no blend shapes: the posed joint. rgn_rot2xyz subtracts joint 0 (= rest_joints[0]), vertices do not."""
    eng = tiny[3]
    sk = skeleton("tree55")
    rest = sk["rest_joints"].astype(np.float32)
    body = dict(sk, mesh={"v_template": rest, "posedirs": np.zeros((486, 165), np.float32), "lbs_weights": np.eye(55, dtype=np.float32), "shapedirs": None,
                          "faces": None, "identity_joints": np.zeros(0, np.int32)})
    rng = np.random.Generator(np.random.PCG64(14))
    x = make_x(rng, 3, 61, 55, "rot6d", False, True, 1)
    got = run_kernel(body, x, None, translation=False)
    joints = run_joints(eng, x, None, sk, translation=False) + rest[0][None, None, :, None]
    tol = 4 * float(np.spacing(np.float32(np.abs(joints).max())))
    err = float(np.abs(got.astype(np.float64) - joints).max())
    print(f"one-hot vertices vs rgn_rot2xyz joints: {err:.3e} (4 spacings: {tol:.3e})")
    assert err <= tol


def test_captured_in_a_graph_the_replay_equals_the_eager_call():
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(15))
    x = make_x(rng, 3, 61, 55, "rot6d", True, True, 2)
    mask = make_mask("ragged", 3, 61, rng)
    eager, replay = run_kernel(body, x, mask, P=2, graph=True)
    assert np.isfinite(replay).all() and np.array_equal(eager.view(np.int32), replay.view(np.int32))


def test_identity_joints_rows_change_no_output_bit(golden):
    g = golden("rot2verts_p1")
    body = golden_body(g)
    rng = np.random.Generator(np.random.PCG64(16))
    x = g["x"]
    y = x.copy()
    y[:, 22:25] = rng.standard_normal((3, 3, 6, 7))
    assert np.array_equal(run_kernel(body, x, None).view(np.int32), run_kernel(body, y, None).view(np.int32))
    free = dict(body, mesh=dict(body["mesh"], identity_joints=np.zeros(0, np.int32)))
    a, b = run_kernel(free, x, None), run_kernel(free, y, None)
    assert not np.array_equal(a, b)
    check("p1 with identity_joints=[]", b, y, None, free)


def test_model_rot2xyz_vertices_after_sampling_and_through_the_guidance_wrapper(tiny):
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg, model, diffusion, eng = tiny
    B, T = 2, cfg["num_frames"]
    wrapped = ClassifierFreeSampleModel(model)
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B)).cuda(), "action": torch.from_numpy(synth.make_actions(cfg, B)).cuda(),
         "scale": torch.full((B,), 2.5, device="cuda")}
    sample = diffusion.p_sample_loop(wrapped, (B, cfg["njoints"], cfg["nfeats"], T), clip_denoised=False, model_kwargs={"y": y}, seed=3)
    body = synth.make_body(cfg["njoints"] - 1, 70)
    model.set_skeleton(body)
    try:
        mask = torch.ones(B, T, dtype=torch.bool)
        mask[1, 5:] = False
        kw = dict(pose_rep="rot6d", glob=True, translation=True, vertstrans=True, num_person=1, betas=None, beta=0, glob_rot=None)
        for m, label in ((model, "tiny model.rot2xyz vertices"), (wrapped, "tiny guidance wrapper vertices")):
            v = m.rot2xyz(x=sample, mask=mask, jointstype="vertices", get_rotations_back=False, **kw)
            assert v.device == sample.device and tuple(v.shape) == (B, 70, 3, T)
            check(label, v.cpu().numpy(), sample.cpu().numpy(), mask.numpy(), body)
        first = model.rot2xyz._body[0]
        v2, rots, root = model.rot2xyz(x=sample, mask=mask, jointstype="vertices", get_rotations_back=True, **kw)
        assert model.rot2xyz._body[0] is first                       # the device-resident body is made once
        assert torch.equal(v2, v) and tuple(rots.shape) == (int(mask.sum()), 3, 3, 3) and tuple(root.shape) == (int(mask.sum()), 3, 3)
        check("tiny vertices beta=2", model.rot2xyz(x=sample, mask=mask, jointstype="vertices", **dict(kw, beta=2.0)).cpu().numpy(), sample.cpu().numpy(),
              mask.numpy(), body, beta=2.0)
        joints = model.rot2xyz(x=sample, mask=mask, jointstype="smplx", **kw)       # the joints path is still served by the same object
        assert tuple(joints.shape) == (B, 4, 3, T)
    finally:
        model.set_skeleton(None)


def test_cgenerate_writes_vertices_faces_and_obj_files(tmp_path):
    from regennet_amd.sample import cgenerate
    obj = tmp_path / "obj"
    out = cgenerate.main(["--synthetic", "--num_samples", "2", "--num_repetitions", "1", "--timestep_respacing", "ddim5", "--use_ddim",
                          "--guidance_param", "2.5", "--skeleton", "synthetic", "--vertices", "--obj_dir", str(obj), "--output_dir", str(tmp_path)])
    res = np.load(out, allow_pickle=True).item()
    body = synth.make_body(55)
    assert res["vertices"].shape == (2, 130, 3, 60) and res["motion"].shape == (2, 55, 3, 60) and np.array_equal(res["faces"], body["mesh"]["faces"])
    check("cgenerate --skeleton synthetic --vertices", res["vertices"], res["output"], np.ones((2, 60), bool), body)
    files = sorted(glob.glob(str(obj / "sample*" / "frame*.obj")))
    assert len(files) == 120 and files[0].endswith(os.path.join("sample00", "frame000.obj"))
    lines = open(files[61]).read().splitlines()
    assert len(lines) == 130 + 128 and lines[0] == "v %.6f %.6f %.6f" % tuple(res["vertices"][1, 0, :, 1]) and lines[130] == "f 1 2 3"


def test_argument_errors():
    body = make_body("pair", 4)
    eng = _lib.BodyEngine(body["mesh"], 2, 0)
    lib = eng.lib
    x, out = torch.zeros(1, 3, 6, 2, device="cuda"), torch.zeros(1, 4, 3, 2, device="cuda")
    work = torch.empty(eng.workspace_bytes(1, 2, 1), dtype=torch.uint8, device="cuda")
    rest, par, betas = np.zeros((2, 3), np.float32), np.array([-1, 0], np.int32), np.zeros(10, np.float32)
    vp = ctypes.c_void_p

    def call(x_=x, out_=out, rest_=rest, par_=par, rep=0, P=1, flags=3, gr=None, B=1, T=2, work_=work, nbytes=None, be=None):
        p = lambda a: None if a is None else a.ctypes.data_as(vp)      # noqa: E731
        rc = lib.rgn_rot2verts(eng.h, _lib._ptr(x_), None, B, T, p(rest_), p(par_), rep, P, flags, p(gr), p(be), _lib._ptr(out_), None, _lib._ptr(work_),
                               work.numel() if nbytes is None else nbytes, None)
        return rc, (lib.rgn_body_last_error(eng.h) or b"").decode()

    try:
        assert call()[0] == 0 and call(be=betas)[0] == 0
        for kw, text in ((dict(x_=None), "null"), (dict(out_=None), "null"), (dict(rest_=None), "null"), (dict(par_=None), "null"),
                         (dict(par_=np.array([0, 0], np.int32)), "parents[0] != -1"), (dict(par_=np.array([-1, 1], np.int32)), "parents[1]"),
                         (dict(P=0), "num_person"), (dict(rep=4), "pose_rep"), (dict(flags=1), "glob_rot"), (dict(flags=8), "unknown flag"), (dict(B=0), "B < 1"),
                         (dict(nbytes=work.numel() - 1), "workspace"), (dict(work_=None), "workspace")):
            rc, err = call(**kw)
            assert rc == -1 and text in err, (kw, rc, err)
        n = ctypes.c_uint64()
        assert lib.rgn_rot2verts_workspace(eng.h, 0, 2, 1, ctypes.byref(n)) == -1 and lib.rgn_rot2verts_workspace(eng.h, 1, 2, 1, None) == -1
        torch.cuda.synchronize()
    finally:
        eng.close()
    with pytest.raises(_lib.RgnError, match="V outside"):
        _lib.BodyEngine(dict(body["mesh"], v_template=np.zeros((0, 3), np.float32)), 2, 0)
