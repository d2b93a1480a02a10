"""GPU: rgn_rot2xyz (csrc/rgn_fk.hip) against the fp64 restatement that tests/test_rot2xyz_cpu.py pins to the reference.

Bound, per case: the fp32 run of the SAME restatement deviates from its fp64 run by some maximum d - the reference arithmetic at the kernel's
precision, computed here, never taken from the kernel. The kernel may associate the 3x3 products differently at each level of the chain,
which is the same order of error again in either direction, so it must stay within 4 d. Where d is 0, 1 ulp of the case's largest |xyz|.
REGENNET_ROT2XYZ_TABLE=<file> writes the measured table (profiles/rot2xyz_parity.txt)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests.rot2xyz_ref import CHANNELS, rot2xyz_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "rot2xyz_*.npz")))
TABLE = []


@pytest.fixture(scope="module")
def tiny():
    """One tiny model on the GPU: its engine is the finalized handle every call below runs on."""
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    yield cfg, model, diffusion, eng
    if TABLE and os.environ.get("REGENNET_ROT2XYZ_TABLE"):
        with open(os.environ["REGENNET_ROT2XYZ_TABLE"], "w") as f:
            f.write(f"rgn_rot2xyz on {torch.cuda.get_device_name(0)}: max |kernel - fp64 restatement| against the bound 4 x max |fp32 restatement - fp64 restatement|\n")
            f.write(f"{'case':58s} {'max|xyz|':>9s} {'fp32 ref':>10s} {'bound':>10s} {'kernel':>10s}\n")
            for row in TABLE:
                f.write("%-58s %9.3f %10.3e %10.3e %10.3e\n" % row)


def skeleton(kind):
    if kind == "tree55":
        return synth.make_skeleton(55)
    if kind == "tree24":
        return synth.make_skeleton(24, seed=24)
    if kind == "one":
        return synth.make_skeleton(1)
    sk = synth.make_skeleton(64, depth=63, seed=3)                  # "chain64": every joint below the one before - the deepest tree allowed
    if kind == "star64":
        sk["parents"] = np.array([-1] + [0] * 63, dtype=np.int32)
    else:
        assert kind == "chain64" and list(sk["parents"]) == list(range(-1, 63))
    return sk


def make_mask(kind, B, T, rng):
    if kind == "none":
        return None
    if kind == "true":
        return np.ones((B, T), bool)
    if kind == "false":
        return np.zeros((B, T), bool)
    m = rng.uniform(size=(B, T)) < 0.6
    m[0, 0] = False                                                 # (frame 0 masked: its translation still anchors the one-person row)
    return m


def make_x(rng, B, T, J, pose_rep, translation, glob, P):
    """[B, R, C P, T] fp32: un-normalised rot6d / quaternions, axis-angle vectors, proper rotation matrices; translation in [-1, 1]."""
    C = CHANNELS[pose_rep]
    nrot = J if glob else J - 1
    if pose_rep == "rotmat":
        q = rng.standard_normal((B, T, nrot, P, 4))
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        w, x, y, z = (q[..., i] for i in range(4))
        rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    else:
        rot = rng.standard_normal((B, T, nrot, P, C)) * (1.5 if pose_rep == "rotvec" else 1.0)
    if translation:
        tr = np.zeros((B, T, 1, P, C))
        tr[..., :3] = rng.uniform(-1, 1, (B, T, 1, P, 3))
        rot = np.concatenate([rot, tr], axis=2)
    return np.ascontiguousarray(rot.reshape(B, T, rot.shape[2], P * C).transpose(0, 2, 3, 1)).astype(np.float32)


def run_kernel(eng, x, mask, sk, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, P=1, glob_rot=None, rest=None, want_rot=False):
    """Engine.rot2xyz on numpy inputs -> numpy xyz (and the rotmat tensor)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    md = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    B, T, J = x.shape[0], x.shape[-1], len(sk["parents"])
    out = torch.full((B, J, 3 * P, T), float("nan"), device="cuda")
    rot = torch.full((B, P, T, J, 3, 3), float("nan"), device="cuda") if want_rot else None
    flags = (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)
    eng.rot2xyz(xd, md, sk["rest_joints"] if rest is None else rest, sk["parents"], _lib.POSE_REP[pose_rep], P, flags, glob_rot, out, rot,
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), rot) if want_rot else out.cpu().numpy()


def check(label, got, x, mask, sk, **kw):
    """got within 4 x (fp32 restatement's deviation from the fp64 one), both computed here on the same inputs."""
    ref_kw = dict(pose_rep=kw.get("pose_rep", "rot6d"), translation=kw.get("translation", True), glob=kw.get("glob", True),
                  vertstrans=kw.get("vertstrans", True), glob_rot=kw.get("glob_rot"), num_person=kw.get("P", 1), beta=kw.get("beta", 0))
    m = None if mask is None else torch.from_numpy(mask)
    r64 = rot2xyz_ref(torch.from_numpy(x), m, sk, dtype=torch.float64, **ref_kw).numpy()
    r32 = rot2xyz_ref(torch.from_numpy(x), m, sk, dtype=torch.float32, **ref_kw).double().numpy()
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
def test_goldens(tiny, golden, name):
    eng = tiny[3]
    g = golden(name)
    sk = {"rest_joints": g["rest_joints"], "parents": g["parents"], "shape_joints": g["shape_joints"]}
    kw = dict(pose_rep=str(g["pose_rep"]), translation=bool(g["translation"]), glob=bool(g["glob"]), vertstrans=bool(g["vertstrans"]),
              P=int(g["num_person"]), glob_rot=None if bool(g["glob"]) else g["glob_rot"])
    mask = None if bool(g["mask_none"]) else g["mask"]
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    rest = Rotation2xyz(sk).rest_joints(beta=float(g["beta"]))
    got = run_kernel(eng, g["x"], mask, sk, rest=rest, **kw)
    r64 = check(name, got, g["x"], mask, sk, beta=float(g["beta"]), **kw)
    assert float(np.abs(r64 - g["expected"]).max()) < 1e-12          # (the restatement is the recorded reference run)


# (B, T) x persons x skeleton x mask: every value of each axis appears, every (B, T) with both person counts
SHAPES = [(1, 1), (3, 7), (2, 60), (2, 61), (5, 64), (1, 150)]
SKELETONS = ["tree55", "tree24", "one", "chain64", "star64"]
MASKS = ["none", "true", "ragged", "false"]
RANDOM = [(B, T, P, SKELETONS[(2 * i + P) % 5], MASKS[(2 * i + P + i // 2) % 4]) for i, (B, T) in enumerate(SHAPES) for P in (1, 2)]
RANDOM += [(3, 7, 1, "chain64", "ragged"), (2, 61, 2, "tree55", "ragged"), (5, 64, 1, "star64", "none"), (1, 150, 2, "one", "true"),
           (2, 60, 1, "tree55", "false"), (3, 7, 2, "tree24", "none")]


@pytest.mark.parametrize("B,T,P,skel,mask_kind", RANDOM)
def test_random_cases(tiny, B, T, P, skel, mask_kind):
    eng = tiny[3]
    sk = skeleton(skel)
    J = len(sk["parents"])
    rng = np.random.Generator(np.random.PCG64(B * 1000 + T * 10 + P))
    mask = make_mask(mask_kind, B, T, rng)
    x = make_x(rng, B, T, J, "rot6d", True, True, P)
    check(f"B{B} T{T} P{P} {skel} mask={mask_kind}", run_kernel(eng, x, mask, sk, P=P), x, mask, sk, P=P)


@pytest.mark.parametrize("pose_rep,translation,glob,vertstrans", [("rotvec", True, True, True), ("rotquat", True, False, True), ("rotmat", False, True, True),
                                                                   ("rot6d", True, True, False), ("rot6d", False, False, True), ("rotvec", True, False, False)])
def test_random_settings(tiny, pose_rep, translation, glob, vertstrans):
    eng = tiny[3]
    sk = skeleton("tree55")
    rng = np.random.Generator(np.random.PCG64(77))
    B, T, P = 2, 61, 2
    mask = make_mask("ragged", B, T, rng)
    x = make_x(rng, B, T, 55, pose_rep, translation, glob, P)
    kw = dict(pose_rep=pose_rep, translation=translation, glob=glob, vertstrans=vertstrans, P=P, glob_rot=None if glob else np.array([0.3, -2.0, 1.1], np.float32))
    check(f"B2 T61 P2 tree55 {pose_rep} trans={int(translation)} glob={int(glob)} vertstrans={int(vertstrans)}", run_kernel(eng, x, mask, sk, **kw), x, mask, sk, **kw)


def test_zero_vectors_take_the_normalisation_floor(tiny):
    """All-zero 6-vectors (and a zero axis-angle vector) on some joints: F.normalize's max(||v||, 1e-12) gives a zero matrix, not NaN."""
    eng = tiny[3]
    sk = skeleton("tree55")
    rng = np.random.Generator(np.random.PCG64(9))
    x = make_x(rng, 3, 7, 55, "rot6d", True, True, 1)
    x[:, [0, 3, 17, 54]] = 0
    x[1, 9, 3:] = 0                                                   # (second vector zero: b2 degenerates alone)
    got = run_kernel(eng, x, None, sk)
    check("B3 T7 P1 tree55 zero 6-vectors", got, x, None, sk)
    xv = make_x(rng, 3, 7, 55, "rotvec", True, True, 1)
    xv[:, [0, 5]] = 0
    xv[0, 7] = 1e-7                                                   # below the small-angle switch of axis_angle_to_quaternion
    check("B3 T7 P1 tree55 zero / tiny rotvec", run_kernel(eng, xv, None, sk, pose_rep="rotvec"), xv, None, sk, pose_rep="rotvec")


def test_rotmat_output_is_rgn_rot6d_to_matrix_bit_for_bit(tiny):
    eng = tiny[3]
    sk = skeleton("tree55")
    rng = np.random.Generator(np.random.PCG64(11))
    B, T, P, J = 2, 61, 2, 55
    x = make_x(rng, B, T, J, "rot6d", True, True, P)
    x[0, 4] = 0
    _, rot = run_kernel(eng, x, make_mask("ragged", B, T, rng), sk, P=P, want_rot=True)
    d6 = torch.from_numpy(x).cuda()[:, :J].reshape(B, J, P, 6, T).permute(0, 2, 4, 1, 3).contiguous()          # [B, P, T, J, 6]
    mat = torch.empty(B, P, T, J, 3, 3, device="cuda")
    eng.rot6d_to_matrix(d6, mat, d6.numel() // 6, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(rot.view(torch.int32), mat.view(torch.int32))


def test_rows_and_frames_do_not_depend_on_the_batch(tiny):
    """Row b of a B = 5 call equals the B = 1 call, and the first 7 frames of a T = 61 call the T = 7 call, bit for bit."""
    eng = tiny[3]
    sk = skeleton("tree55")
    rng = np.random.Generator(np.random.PCG64(12))
    for P in (1, 2):
        x = make_x(rng, 5, 61, 55, "rot6d", True, True, P)
        mask = make_mask("ragged", 5, 61, rng)
        full = run_kernel(eng, x, mask, sk, P=P)
        for b in (0, 3, 4):
            one = run_kernel(eng, x[b:b + 1], mask[b:b + 1], sk, P=P)
            assert np.array_equal(full[b:b + 1].view(np.int32), one.view(np.int32)), (P, b)
        short = run_kernel(eng, np.ascontiguousarray(x[..., :7]), np.ascontiguousarray(mask[:, :7]), sk, P=P)
        assert np.array_equal(full[..., :7].view(np.int32), short.view(np.int32)), P


def test_argument_errors(tiny):
    eng = tiny[3]
    lib = eng.lib
    x = torch.zeros(1, 4, 6, 2, device="cuda")
    out = torch.zeros(1, 3, 3, 2, device="cuda")
    rest = np.zeros((65, 3), np.float32)
    par = np.arange(-1, 64, dtype=np.int32)
    glob_rot = np.zeros(3, np.float32)
    vp = ctypes.c_void_p

    def call(x_=x, out_=out, rest_=rest, par_=par, J=3, rep=0, P=1, flags=3, gr=None, B=1, T=2):
        p = lambda a: None if a is None else a.ctypes.data_as(vp)      # noqa: E731
        rc = lib.rgn_rot2xyz(eng.h, _lib._ptr(x_), None, B, T, J, p(rest_), p(par_), rep, P, flags, p(gr), _lib._ptr(out_), None, None)
        return rc, (lib.rgn_last_error(eng.h) or b"").decode()

    assert call()[0] == 0
    for kw, text in ((dict(x_=None), "null"), (dict(out_=None), "null"), (dict(rest_=None), "null"), (dict(par_=None), "null"),
                     (dict(J=0), "J outside"), (dict(J=65), "J outside"), (dict(par_=np.array([0, 0, 1], np.int32)), "parents[0] != -1"),
                     (dict(par_=np.array([-1, 1, 1], np.int32)), "parents[1]"), (dict(par_=np.array([-1, 0, 2], np.int32)), "parents[2]"),
                     (dict(par_=np.array([-1, 0, -1], np.int32)), "parents[2]"), (dict(P=0), "num_person"), (dict(rep=4), "pose_rep"),
                     (dict(rep=-1), "pose_rep"), (dict(flags=1), "glob_rot"), (dict(B=0), "B < 1")):
        rc, err = call(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
    assert call(flags=1, gr=glob_rot, x_=torch.zeros(1, 3, 6, 2, device="cuda"))[0] == 0
    torch.cuda.synchronize()


def test_model_rot2xyz_after_sampling_and_through_the_guidance_wrapper(tiny):
    """model.rot2xyz on a sampled batch of the tiny config (4 joints + translation row), on the engine the sampling call used; the same through
    ClassifierFreeSampleModel with the skeleton set AFTER wrapping; a non-contiguous x; get_rotations_back."""
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg, model, diffusion, eng = tiny
    B, T = 2, cfg["num_frames"]
    wrapped = ClassifierFreeSampleModel(model)
    y = {"cmotion": torch.from_numpy(synth.make_cmotion(cfg, B)).cuda(), "action": torch.from_numpy(synth.make_actions(cfg, B)).cuda(),
         "scale": torch.full((B,), 2.5, device="cuda")}
    sample = diffusion.p_sample_loop(wrapped, (B, cfg["njoints"], cfg["nfeats"], T), clip_denoised=False, model_kwargs={"y": y}, seed=3)
    sk = synth.make_skeleton(cfg["njoints"] - 1)
    model.set_skeleton(sk)
    try:
        mask = torch.ones(B, T, dtype=torch.bool)
        mask[1, 5:] = False
        kw = dict(pose_rep="rot6d", glob=True, translation=True, jointstype="smplx", vertstrans=True, num_person=1, betas=None, beta=0, glob_rot=None)
        for m, label in ((model, "tiny model.rot2xyz"), (wrapped, "tiny guidance wrapper rot2xyz")):
            xyz = m.rot2xyz(x=sample, mask=mask, get_rotations_back=False, **kw)
            assert xyz.device == sample.device and tuple(xyz.shape) == (B, 4, 3, T)
            check(label, xyz.cpu().numpy(), sample.cpu().numpy(), mask.numpy(), sk)
        assert model._engine is eng                                   # no second engine was built for the call
        nc = sample.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        assert not nc.is_contiguous()
        assert torch.equal(model.rot2xyz(x=nc, mask=mask, **kw), xyz)
        xyz2, rots, root = model.rot2xyz(x=sample, mask=mask, get_rotations_back=True, **kw)
        assert torch.equal(xyz2, xyz) and tuple(rots.shape) == (int(mask.sum()), 3, 3, 3) and tuple(root.shape) == (int(mask.sum()), 3, 3)
        check("tiny beta=2", model.rot2xyz(x=sample, mask=mask, **dict(kw, beta=2.0)).cpu().numpy(), sample.cpu().numpy(), mask.numpy(), sk, beta=2.0)
    finally:
        model.set_skeleton(None)


def test_cgenerate_writes_motion_with_a_skeleton(tmp_path):
    from regennet_amd.sample import cgenerate
    out = cgenerate.main(["--synthetic", "--num_samples", "3", "--num_repetitions", "1", "--timestep_respacing", "ddim5", "--use_ddim",
                          "--guidance_param", "2.5", "--skeleton", "synthetic", "--output_dir", str(tmp_path)])
    res = np.load(out, allow_pickle=True).item()
    assert list(res)[0] == "motion" and res["motion"].shape == (3, 55, 3, 60) and res["output"].shape == (3, 56, 6, 60)
    check("cgenerate --skeleton synthetic", res["motion"], res["output"], np.ones((3, 60), bool), synth.make_skeleton(55))
