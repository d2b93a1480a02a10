"""GPU: rgn_rot2xyz_shaped (csrc/rgn_fk.hip) and rgn_rot2verts_shaped (csrc/rgn_lbs.hip) - a body shape per frame, read on the device -
against the fp64 restatement that tests/test_rot2xyz_shaped_cpu.py pins to the reference (tests/rot2xyz_shaped_ref.py).

Bound, per case, the project's rule (tests/test_rot2xyz_gpu.py, tests/test_rot2verts_gpu.py): the fp32 run of the SAME restatement deviates from
its fp64 run by some maximum d, computed here and never taken from the kernel; the kernel may associate the short products differently, the same
order of error again in either direction, so it must stay within 4 d; where d is 0, one fp32 spacing at the case's largest |xyz|.
REGENNET_ROT2XYZ_SHAPED_TABLE=<file> writes the measured table (profiles/rot2xyz_shaped_parity.txt).

On the commit before the feature every test here fails: the two symbols do not exist and the wrapper raises NotImplementedError."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests.rot2verts_ref import golden_body
from tests.rot2xyz_shaped_ref import expand_betas, rows_to_frames, shaped_ref
from tests.test_rot2verts_gpu import cut, make_body, run_kernel as run_verts_one_shape
from tests.test_rot2xyz_gpu import make_mask, make_x, run_kernel as run_joints_one_shape

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[len("shaped_rot2xyz_"):-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "shaped_rot2xyz_*.npz")))
TABLE = []


@pytest.fixture(scope="module")
def tiny():
    """One tiny model on the GPU: its engine is the finalized handle the joints calls run on."""
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    yield cfg, model, diffusion, eng
    if TABLE and os.environ.get("REGENNET_ROT2XYZ_SHAPED_TABLE"):
        with open(os.environ["REGENNET_ROT2XYZ_SHAPED_TABLE"], "w") as f:
            f.write(f"rgn_rot2xyz_shaped / rgn_rot2verts_shaped on {torch.cuda.get_device_name(0)}: max |kernel - fp64 restatement| against the bound "
                    "4 x max |fp32 restatement - fp64 restatement|\n")
            f.write(f"{'case':84s} {'max|xyz|':>9s} {'fp32 ref':>10s} {'bound':>10s} {'kernel':>10s}\n")
            for row in TABLE:
                f.write("%-84s %9.3f %10.3e %10.3e %10.3e\n" % row)


def strides_of(betas, B, P, T, kind):
    """(stride_b, stride_p, stride_t) in elements of a contiguous betas array: 'motion' [B, nb], 'person' [B, P, nb], 'time' [B, T, nb],
    'frame' [B, P, T, nb]."""
    nb = betas.shape[-1]
    want = {"motion": (B, nb), "person": (B, P, nb), "time": (B, T, nb), "frame": (B, P, T, nb)}[kind]
    assert tuple(betas.shape) == want, (betas.shape, want)
    return {"motion": (nb, 0, 0), "person": (P * nb, nb, 0), "time": (T * nb, 0, nb), "frame": (P * T * nb, T * nb, nb)}[kind]


def full_betas(betas, B, P, T, kind):
    """-> [B, P, T, nb], what the restatement takes."""
    b = np.asarray(betas, np.float32)
    return expand_betas(b[:, None] if kind == "time" else b, B, P, T)


def flags_of(translation, glob, vertstrans):
    return (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)


def run_joints(eng, sk, x, mask, betas, kind, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, P=1, glob_rot=None, want_rot=False,
               graph=False):
    """Engine.rot2xyz_shaped on numpy inputs -> numpy xyz (and the rotmat tensor); graph: eager, then captured and replayed -> both."""
    B, T, J = x.shape[0], x.shape[-1], len(sk["parents"])
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    md = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    bd = torch.from_numpy(np.array(betas, dtype=np.float32)).cuda()
    sj = torch.from_numpy(np.ascontiguousarray(sk["shape_joints"][:, :, :betas.shape[-1]], dtype=np.float32)).cuda()
    out = torch.full((B, J, 3 * P, T), float("nan"), device="cuda")
    rot = torch.full((B, P, T, J, 3, 3), float("nan"), device="cuda") if want_rot else None

    def call():
        eng.rot2xyz_shaped(xd, md, sk["rest_joints"], sk["parents"], sj, bd, strides_of(betas, B, P, T, kind), _lib.POSE_REP[pose_rep], P,
                           flags_of(translation, glob, vertstrans), glob_rot, out, rot, torch.cuda.current_stream().cuda_stream)

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


def run_verts(body, x, mask, betas, kind, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, P=1, glob_rot=None, want_rot=False,
              graph=False):
    """BodyEngine.rot2verts_shaped on numpy inputs -> numpy vertices (and the rotmat tensor); graph: eager, then captured and replayed -> both."""
    eng = _lib.BodyEngine(body["mesh"], len(body["parents"]), 0)
    try:
        B, T, J, V = x.shape[0], x.shape[-1], len(body["parents"]), body["mesh"]["v_template"].shape[0]
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        md = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        bd = torch.from_numpy(np.array(betas, dtype=np.float32)).cuda()
        sj = torch.from_numpy(np.ascontiguousarray(body["shape_joints"][:, :, :betas.shape[-1]], dtype=np.float32)).cuda()
        out = torch.full((B, V, 3 * P, T), float("nan"), device="cuda")
        rot = torch.full((B, P, T, J, 3, 3), float("nan"), device="cuda") if want_rot else None
        work = torch.empty(eng.workspace_bytes_shaped(B, T, P), dtype=torch.uint8, device="cuda")

        def call():
            eng.rot2verts_shaped(xd, md, body["rest_joints"], body["parents"], sj, bd, strides_of(betas, B, P, T, kind), _lib.POSE_REP[pose_rep], P,
                                 flags_of(translation, glob, vertstrans), glob_rot, out, rot, work, torch.cuda.current_stream().cuda_stream)

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


def check(label, got, x, mask, body, bt, vertices, **kw):
    """got within 4 x (fp32 restatement's deviation from the fp64 one), both computed here on the same inputs; bt: betas [B, P, T, nb]."""
    ref_kw = dict(pose_rep=kw.get("pose_rep", "rot6d"), translation=kw.get("translation", True), glob=kw.get("glob", True),
                  vertstrans=kw.get("vertstrans", True), glob_rot=kw.get("glob_rot"), num_person=kw.get("P", 1), vertices=vertices)
    m = None if mask is None else torch.from_numpy(mask)
    r64 = shaped_ref(x, m, body, bt, dtype=torch.float64, **ref_kw).numpy()
    r32 = shaped_ref(x, m, body, bt, dtype=torch.float32, **ref_kw).double().numpy()
    d = float(np.abs(r32 - r64).max())
    top = float(np.abs(r64).max())
    bound = 4 * d if d > 0 else float(np.spacing(np.float32(top)))
    assert got.shape == r64.shape and np.isfinite(got).all(), (label, got.shape, r64.shape)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    TABLE.append((("verts  " if vertices else "joints ") + label, top, d, bound, err))
    print(f"{'verts' if vertices else 'joints'} {label}: max|xyz| {top:.3f}  fp32 ref {d:.3e}  bound {bound:.3e}  kernel {err:.3e}")
    assert err <= bound, (label, err, bound)
    return r64


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(tiny, golden, name):
    eng = tiny[3]
    for kernel in ("rot2xyz", "rot2verts"):
        g = golden(f"shaped_{kernel}_{name}")
        body = golden_body(g)
        kw = dict(pose_rep=str(g["pose_rep"]), translation=bool(g["translation"]), glob=bool(g["glob"]), vertstrans=bool(g["vertstrans"]),
                  P=int(g["num_person"]), glob_rot=None if bool(g["glob"]) else g["glob_rot"])
        mask = None if bool(g["mask_none"]) else g["mask"]
        B, T, P = g["x"].shape[0], g["x"].shape[-1], kw["P"]
        bt = rows_to_frames(g["betas"], mask, B, T, P)
        per_time = np.ascontiguousarray(bt[:, 0])                    # [B, T, nb]: the wrapper's own form, stride_p = 0
        if kernel == "rot2xyz":
            got = run_joints(eng, body, g["x"], mask, per_time, "time", **kw)
        else:
            got = run_verts(body, g["x"], mask, per_time, "time", **kw)
        r64 = check(f"golden {name}", got, g["x"], mask, body, bt, kernel == "rot2verts", **kw)
        assert float(np.abs(r64 - g["expected"]).max()) < 1e-12          # (the restatement is the recorded reference run)


# the smallest shapes at which a 32-frame tile holds frames of different motions and of different persons, with ragged last tiles
SHAPES = [(3, 20, 2), (2, 33, 1), (5, 7, 2)]
BODIES = [("tree55", 130), ("tree24", 70)]
MASKS = ["none", "ragged", "motion_off"]
KINDS = ["motion", "person", "frame"]
RANDOM = [(B, T, P, BODIES[(i + j) % 2], MASKS[(i + j) % 3], KINDS[(i + 2 * j) % 3]) for i, (B, T, P) in enumerate(SHAPES) for j in range(3)]
assert {c[3] for c in RANDOM} == set(BODIES) and {c[4] for c in RANDOM} == set(MASKS) and {c[5] for c in RANDOM} == set(KINDS)
assert all({c[4] for c in RANDOM if c[:3] == s} == set(MASKS) and {c[5] for c in RANDOM if c[:3] == s} == set(KINDS) for s in SHAPES)


def shaped_mask(kind, B, T, rng):
    if kind == "motion_off":                                        # ragged, and one motion masked throughout
        m = make_mask("ragged", B, T, rng)
        m[1] = False
        return m
    return make_mask(kind, B, T, rng)


def random_betas(rng, kind, B, P, T, nb=10):
    return rng.standard_normal({"motion": (B, nb), "person": (B, P, nb), "time": (B, T, nb), "frame": (B, P, T, nb)}[kind]).astype(np.float32)


@pytest.mark.parametrize("B,T,P,bodykind,mask_kind,kind", RANDOM)
def test_random_cases(tiny, B, T, P, bodykind, mask_kind, kind):
    body = make_body(*bodykind)
    J = len(body["parents"])
    rng = np.random.Generator(np.random.PCG64(B * 1000 + T * 10 + P + len(mask_kind)))
    mask = shaped_mask(mask_kind, B, T, rng)
    x = make_x(rng, B, T, J, "rot6d", True, True, P)
    betas = random_betas(rng, kind, B, P, T)
    bt = full_betas(betas, B, P, T, kind)
    label = f"B{B} T{T} P{P} {bodykind[0]} V{bodykind[1]} mask={mask_kind} betas per {kind}"
    check(label, run_joints(tiny[3], body, x, mask, betas, kind, P=P), x, mask, body, bt, False, P=P)
    check(label, run_verts(body, x, mask, betas, kind, P=P), x, mask, body, bt, True, P=P)


def test_other_settings_and_fewer_betas_than_the_file(tiny):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(78))
    B, T, P = 2, 33, 2
    mask = shaped_mask("ragged", B, T, rng)
    for pose_rep, translation, glob, vertstrans, nb in (("rotvec", True, False, True, 3), ("rotquat", True, True, False, 10), ("rotmat", False, True, True, 1)):
        x = make_x(rng, B, T, 55, pose_rep, translation, glob, P)
        betas = random_betas(rng, "person", B, P, T, nb)
        bt = full_betas(betas, B, P, T, "person")
        kw = dict(pose_rep=pose_rep, translation=translation, glob=glob, vertstrans=vertstrans, P=P, glob_rot=None if glob else np.array([0.3, -2.0, 1.1], np.float32))
        label = f"B2 T33 P2 tree55 V130 {pose_rep} trans={int(translation)} glob={int(glob)} vertstrans={int(vertstrans)} nb={nb}"
        check(label, run_joints(tiny[3], body, x, mask, betas, "person", **kw), x, mask, body, bt, False, **kw)
        check(label, run_verts(body, x, mask, betas, "person", **kw), x, mask, body, bt, True, **kw)


def test_a_body_without_posedirs_and_one_with_an_odd_vertex_count():
    rng = np.random.Generator(np.random.PCG64(5))
    B, T, P = 3, 20, 2
    for V, pose in ((65, True), (130, False)):
        body = make_body("tree55", V)
        if not pose:
            body["mesh"]["posedirs"] = None
        mask = shaped_mask("ragged", B, T, rng)
        x = make_x(rng, B, T, 55, "rot6d", True, True, P)
        betas = random_betas(rng, "frame", B, P, T)
        check(f"B3 T20 P2 tree55 V{V} posedirs={int(pose)} betas per frame", run_verts(body, x, mask, betas, "frame", P=P), x, mask, body, betas, True, P=P)


def test_the_same_shape_in_every_frame_agrees_with_the_one_shape_calls(tiny):
    """Not bit for bit (the summation order differs: rest joints formed in fp64 on the host there, in fp32 on the device here); both within the bound."""
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(21))
    B, T, P = 3, 20, 2
    mask = shaped_mask("ragged", B, T, rng)
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    betas = np.zeros((B, 10), np.float32)
    betas[:, 1] = 1.5
    bt = full_betas(betas, B, P, T, "motion")
    rest = Rotation2xyz(body).rest_joints(beta=1.5)
    for vertices, new, old in ((False, run_joints(tiny[3], body, x, mask, betas, "motion", P=P), run_joints_one_shape(tiny[3], x, mask, body, P=P, rest=rest)),
                               (True, run_verts(body, x, mask, betas, "motion", P=P), run_verts_one_shape(body, x, mask, P=P, beta=1.5))):
        check("beta=1.5 in every frame: shaped call", new, x, mask, body, bt, vertices, P=P)
        check("beta=1.5 in every frame: one-shape call", old, x, mask, body, bt, vertices, P=P)


def test_a_motions_rows_are_the_single_motion_call_for_every_stride_pattern(tiny):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(12))
    B, T, P = 5, 7, 2
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    mask = shaped_mask("ragged", B, T, rng)
    for kind in ("motion", "person", "time", "frame"):
        betas = random_betas(rng, kind, B, P, T)
        fj, fv = run_joints(tiny[3], body, x, mask, betas, kind, P=P), run_verts(body, x, mask, betas, kind, P=P)
        for b in (0, 3, 4):
            assert same_bits(fj[b:b + 1], run_joints(tiny[3], body, x[b:b + 1], mask[b:b + 1], betas[b:b + 1], kind, P=P)), (kind, b)
            assert same_bits(fv[b:b + 1], run_verts(body, x[b:b + 1], mask[b:b + 1], betas[b:b + 1], kind, P=P)), (kind, b)


def test_stride_0_broadcast_equals_the_expanded_tensor(tiny):
    body = make_body("tree24", 70)
    rng = np.random.Generator(np.random.PCG64(13))
    B, T, P = 3, 20, 2
    x = make_x(rng, B, T, 24, "rot6d", True, True, P)
    mask = shaped_mask("ragged", B, T, rng)
    for kind in ("motion", "person", "time"):
        betas = random_betas(rng, kind, B, P, T)
        bt = full_betas(betas, B, P, T, kind)
        assert same_bits(run_joints(tiny[3], body, x, mask, betas, kind, P=P), run_joints(tiny[3], body, x, mask, bt, "frame", P=P)), kind
        assert same_bits(run_verts(body, x, mask, betas, kind, P=P), run_verts(body, x, mask, bt, "frame", P=P)), kind


def test_nan_betas_at_masked_frames_change_no_output_bit(tiny):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(14))
    B, T, P = 3, 20, 2
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    mask = shaped_mask("motion_off", B, T, rng)
    betas = random_betas(rng, "frame", B, P, T)
    poisoned = betas.copy()
    poisoned[~mask[:, None, :].repeat(P, 1)] = np.nan
    assert np.isnan(poisoned).any()
    assert same_bits(run_joints(tiny[3], body, x, mask, betas, "frame", P=P), run_joints(tiny[3], body, x, mask, poisoned, "frame", P=P))
    assert same_bits(run_verts(body, x, mask, betas, "frame", P=P), run_verts(body, x, mask, poisoned, "frame", P=P))


def test_a_vertex_does_not_depend_on_the_other_vertices():
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(15))
    x = make_x(rng, 3, 7, 55, "rot6d", True, True, 1)
    betas = random_betas(rng, "motion", 3, 1, 7)
    full = run_verts(body, x, None, betas, "motion")
    part = run_verts(cut(body, 64), x, None, betas, "motion")
    assert part.shape == (3, 64, 3, 7) and same_bits(np.ascontiguousarray(full[:, :64]), part)


def test_rotmat_output_is_rgn_rot2xyz_bit_for_bit(tiny):
    eng = tiny[3]
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(11))
    B, T, P = 2, 33, 2
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    mask = shaped_mask("ragged", B, T, rng)
    betas = random_betas(rng, "person", B, P, T)
    _, want = run_joints_one_shape(eng, x, mask, body, P=P, want_rot=True)
    _, rj = run_joints(eng, body, x, mask, betas, "person", P=P, want_rot=True)
    _, rv = run_verts(body, x, mask, betas, "person", P=P, want_rot=True)
    assert torch.equal(rj.view(torch.int32), want.view(torch.int32)) and torch.equal(rv.view(torch.int32), want.view(torch.int32))


def test_captured_in_a_graph_the_replay_equals_the_eager_call(tiny):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(16))
    B, T, P = 3, 20, 2
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    mask = shaped_mask("ragged", B, T, rng)
    betas = random_betas(rng, "person", B, P, T)
    for eager, replay in (run_joints(tiny[3], body, x, mask, betas, "person", P=P, graph=True), run_verts(body, x, mask, betas, "person", P=P, graph=True)):
        assert np.isfinite(replay).all() and same_bits(eager, replay)


def test_real_size_once():
    """SMPL-X's size: 10475 vertices, 55 joints (328 vertex tiles, the last one partial; 8 tiles per workgroup)."""
    body = synth.make_body(55, 10475)
    rng = np.random.Generator(np.random.PCG64(8))
    B, T, P = 2, 40, 1
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    mask = shaped_mask("ragged", B, T, rng)
    betas = random_betas(rng, "motion", B, P, T)
    check("B2 T40 P1 V10475 tree55 mask=ragged betas per motion", run_verts(body, x, mask, betas, "motion"), x, mask, body, full_betas(betas, B, P, T, "motion"), True)


def test_model_rot2xyz_with_betas_rows_and_betas_per_motion_through_the_guidance_wrapper(tiny):
    from regennet_amd.model.cfg_sampler import ClassifierFreeSampleModel
    cfg, model, diffusion, eng = tiny
    B, T = 2, cfg["num_frames"]
    wrapped = ClassifierFreeSampleModel(model)
    rng = np.random.Generator(np.random.PCG64(31))
    body = synth.make_body(cfg["njoints"] - 1, 70)
    J = cfg["njoints"] - 1
    x = torch.from_numpy(make_x(rng, B, T, J, "rot6d", True, True, 1)).cuda()
    model.set_skeleton(body)
    try:
        mask = torch.ones(B, T, dtype=torch.bool)
        mask[1, 5:] = False
        rows = torch.from_numpy(rng.standard_normal((int(mask.sum()), 10)).astype(np.float32))
        per_motion = rng.standard_normal((B, 10)).astype(np.float32)
        kw = dict(pose_rep="rot6d", glob=True, translation=True, vertstrans=True, num_person=1, beta=0, glob_rot=None)
        for jointstype, vertices in (("smplx", False), ("vertices", True)):
            got = wrapped.rot2xyz(x=x, mask=mask, jointstype=jointstype, betas=rows, **kw)
            assert got.device == x.device
            check(f"wrapper betas=[N_live, nb] {jointstype}", got.cpu().numpy(), x.cpu().numpy(), mask.numpy(), body,
                  rows_to_frames(rows.numpy(), mask.numpy(), B, T, 1), vertices)
            got, rots, root = wrapped.rot2xyz(x=x, mask=mask, jointstype=jointstype, betas_per_motion=torch.from_numpy(per_motion), get_rotations_back=True,
                                              **dict(kw, betas=None))
            assert tuple(rots.shape) == (int(mask.sum()), J - 1, 3, 3) and tuple(root.shape) == (int(mask.sum()), 3, 3)
            check(f"wrapper betas_per_motion {jointstype}", got.cpu().numpy(), x.cpu().numpy(), mask.numpy(), body, full_betas(per_motion, B, 1, T, "motion"),
                  vertices)
        assert len(model.rot2xyz._sj_dev) == 1                       # the device copy of shape_joints is made once
        same = model.rot2xyz(x=x, mask=mask, jointstype="smplx", betas=rows[:1].repeat(int(mask.sum()), 1), **kw)       # equal rows: the one-shape path
        one = model.rot2xyz(x=x, mask=mask, jointstype="smplx", betas=rows[0], **kw)
        assert torch.equal(same, one)
    finally:
        model.set_skeleton(None)


def test_cgenerate_with_synthetic_betas_writes_them_and_vertices_that_differ(tmp_path):
    from regennet_amd.sample import cgenerate
    out = cgenerate.main(["--synthetic", "--num_samples", "2", "--num_repetitions", "1", "--timestep_respacing", "ddim5", "--use_ddim",
                          "--guidance_param", "2.5", "--skeleton", "synthetic", "--vertices", "--betas_npz", "synthetic", "--output_dir", str(tmp_path)])
    res = np.load(out, allow_pickle=True).item()
    body = synth.make_body(55)
    assert res["betas"].shape == (2, 10) and not np.array_equal(res["betas"][0], res["betas"][1])
    assert res["vertices"].shape == (2, 130, 3, 60) and res["motion"].shape == (2, 55, 3, 60)
    mask = np.ones((2, 60), bool)
    bt = full_betas(res["betas"], 2, 1, 60, "motion")
    check("cgenerate --betas_npz synthetic: vertices", res["vertices"], res["output"], mask, body, bt, True)
    check("cgenerate --betas_npz synthetic: joints", res["motion"], res["output"], mask, body, bt, False)
    plain = shaped_ref(res["output"], None, body, np.zeros_like(bt), "rot6d", True, True, True, vertices=True).numpy()
    assert float(np.abs(res["vertices"] - plain).max()) > 1e-3      # the shapes were used


def test_argument_errors_that_need_a_handle():
    body = make_body("pair", 4)
    eng = _lib.BodyEngine(body["mesh"], 2, 0)
    lib = eng.lib
    x, out = torch.zeros(1, 3, 6, 2, device="cuda"), torch.zeros(1, 4, 3, 2, device="cuda")
    work = torch.empty(eng.workspace_bytes_shaped(1, 2, 1), dtype=torch.uint8, device="cuda")
    rest, par = np.zeros((2, 3), np.float32), np.array([-1, 0], np.int32)
    sj, betas = torch.zeros(2, 3, 16, device="cuda"), torch.zeros(1, 16, device="cuda")
    vp = ctypes.c_void_p

    def call(nb=10, sb=16, work_=work, nbytes=None, par_=par, sj_=sj):
        p = lambda a: None if a is None else a.ctypes.data_as(vp)      # noqa: E731
        rc = lib.rgn_rot2verts_shaped(eng.h, _lib._ptr(x), None, 1, 2, p(rest), p(par_), _lib._ptr(sj_), nb, _lib._ptr(betas), sb, 0, 0, 0, 1, 3, None,
                                      _lib._ptr(out), None, _lib._ptr(work_), work.numel() if nbytes is None else nbytes, None)
        return rc, (lib.rgn_body_last_error(eng.h) or b"").decode()

    try:
        assert eng.nb == 10 and call()[0] == 0 and call(nb=1)[0] == 0
        for kw, text in ((dict(nb=11), "11 betas, but the body holds 10"), (dict(nb=0), "nb outside [1, 16]"), (dict(nb=17), "nb outside [1, 16]"),
                         (dict(sb=-1), "negative beta stride"), (dict(sj_=None), "null shape_joints_dev or betas_dev"),
                         (dict(par_=np.array([-1, 1], np.int32)), "parents[1]"), (dict(nbytes=work.numel() - 1), "workspace"), (dict(work_=None), "workspace")):
            rc, err = call(**kw)
            assert rc == -1 and err.startswith("rgn_rot2verts_shaped: ") and text in err, (kw, rc, err)
        n = ctypes.c_uint64()
        assert lib.rgn_rot2verts_shaped_workspace(eng.h, 0, 2, 1, ctypes.byref(n)) == -1 and lib.rgn_rot2verts_shaped_workspace(eng.h, 1, 2, 1, None) == -1
        torch.cuda.synchronize()
    finally:
        eng.close()
    bare = dict(body, mesh=dict(body["mesh"], shapedirs=None))
    eng = _lib.BodyEngine(bare["mesh"], 2, 0)
    try:
        rc = eng.lib.rgn_rot2verts_shaped(eng.h, _lib._ptr(x), None, 1, 2, rest.ctypes.data_as(vp), par.ctypes.data_as(vp), _lib._ptr(sj), 1, _lib._ptr(betas),
                                          16, 0, 0, 0, 1, 3, None, _lib._ptr(out), None, _lib._ptr(work), work.numel(), None)
        assert rc == -1 and "1 betas, but the body holds 0" in (eng.lib.rgn_body_last_error(eng.h) or b"").decode()
    finally:
        eng.close()
