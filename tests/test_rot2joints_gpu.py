"""GPU: rgn_rot2joints / rgn_rot2joints_shaped (csrc/rgn_lbs.hip: k_lbs_joints) - the joint types the reference's SMPL layer regresses from the
mesh - against the fp64 restatement that tests/test_rot2joints_cpu.py pins to the reference (tests/rot2joints_ref.py).

Bound, per case, the project's (tests/test_rot2verts_gpu.py check): the fp32 run of the SAME restatement - long sums term by term in index order,
the order class of the fp32-input MFMA - deviates from its fp64 run by some maximum d, computed here and never taken from the kernel; the kernel
must stay within 4 d, and where d is 0 within one fp32 spacing of the case's largest magnitude.

On the commit before the feature every test here fails: the rgn_rot2joints* symbols do not exist and Rotation2xyz refuses the three joint types."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from regennet_amd import _lib, synth
from tests.rot2joints_ref import golden_regs, rot2joints_ref, touched
from tests.rot2verts_ref import golden_body, golden_settings
from tests.rot2xyz_shaped_ref import expand_betas, rows_to_frames
from tests.test_rot2verts_gpu import make_body, run_kernel as run_verts
from tests.test_rot2xyz_gpu import make_mask, make_x, run_kernel as run_skeleton_joints

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "rot2joints_*.npz")))
TYPES = ("vibe", "a2m", "a2mpl")


@pytest.fixture(scope="module")
def tiny():
    """One tiny model on the GPU, for the calls that go through a model (and for rgn_rot2xyz, to compare with)."""
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, diffusion = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    return cfg, model, diffusion, eng


def make_regs(V, nS, Np, Jr, rng, dense=False):
    """Np picks and a [Jr, V] regressor that touch exactly nS vertices (dense: every vertex carries a weight); weights of mixed sign."""
    S = np.sort(rng.choice(V, nS, replace=False))
    picks = rng.choice(S, Np, replace=Np > nS).astype(np.int32) if Np else np.zeros(0, np.int32)
    reg = np.zeros((Jr, V), np.float32)
    if Jr:
        w = rng.uniform(0.2, 1.0, (Jr, nS)) * rng.choice([-1.0, 1.0], (Jr, nS))
        if not dense:
            w *= rng.uniform(size=(Jr, nS)) < 0.5
        reg[:, S] = w
        for s in S:                                                 # every vertex of S is picked or weighed
            if s not in picks and not reg[:, s].any():
                reg[rng.integers(Jr), s] = -0.75
    regs = {"vertex_joints": picks, "J_regressor_extra": reg}
    assert len(touched(regs, V)) == nS, (len(touched(regs, V)), nS)
    return regs


def random_map(J, Np, Jr, n, rng):
    """n entries over all three blocks, with repeats, and a root row that is not row 0."""
    nall = J + Np + Jr
    m = rng.integers(0, nall, n).astype(np.int32)
    m[0], m[1], m[2], m[n - 1] = J - 1, J, nall - 1, m[3]
    return m, int(rng.integers(1, n))


def run_kernel(body, regs, jmap, root, x, mask, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, P=1, glob_rot=None, beta=0,
               frame_betas=None, want_rot=False, graph=False, nan_masked_betas=False):
    """BodyEngine.rot2joints (frame_betas [B, P, T, nb]: rot2joints_shaped) on numpy inputs -> numpy joints; graph: (eager, replayed)."""
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    eng = _lib.BodyEngine(body["mesh"], len(body["parents"]), 0)
    try:
        eng.set_joint_regressors(regs["vertex_joints"], regs["J_regressor_extra"])
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        md = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        B, T, J = x.shape[0], x.shape[-1], len(body["parents"])
        out = torch.full((B, len(jmap), 3 * P, T), float("nan"), device="cuda")
        rot = torch.full((B, P, T, J, 3, 3), float("nan"), device="cuda") if want_rot else None
        flags = (_lib.R2X_TRANSLATION if translation else 0) | (_lib.R2X_GLOB if glob else 0) | (_lib.R2X_VERTSTRANS if vertstrans else 0)
        stream = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731  (asked at the call: under capture it is the capturing stream)
        if frame_betas is None:
            work = torch.empty(eng.joints_workspace_bytes(B, T, P), dtype=torch.uint8, device="cuda")
            betas = None
            if beta:
                betas = np.zeros(eng.nb, np.float32)
                betas[1] = beta
            rest = Rotation2xyz(body).rest_joints(beta=beta)

            def call():
                eng.rot2joints(xd, md, rest, body["parents"], _lib.POSE_REP[pose_rep], P, flags, glob_rot, betas, jmap, root, out, rot, work, stream())
        else:
            work = torch.empty(eng.joints_workspace_bytes_shaped(B, T, P), dtype=torch.uint8, device="cuda")
            fb = np.array(frame_betas, dtype=np.float32)
            if nan_masked_betas:
                fb[np.broadcast_to(~np.asarray(mask, bool)[:, None, :], fb.shape[:3])] = np.nan
            nb = fb.shape[-1]
            bd = torch.from_numpy(np.ascontiguousarray(fb)).cuda()
            sj = torch.from_numpy(np.ascontiguousarray(body["shape_joints"][:, :, :nb], dtype=np.float32)).cuda()

            def call():
                eng.rot2joints_shaped(xd, md, body["rest_joints"], body["parents"], sj, bd, (P * T * nb, T * nb, nb), _lib.POSE_REP[pose_rep], P, flags,
                                      glob_rot, jmap, root, out, rot, work, stream())

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


def check(label, got, x, mask, body, regs, jmap, root, **kw):
    """got within 4 x (fp32 restatement's deviation from the fp64 one), both computed here on the same inputs."""
    ref_kw = dict(pose_rep=kw.get("pose_rep", "rot6d"), translation=kw.get("translation", True), glob=kw.get("glob", True),
                  vertstrans=kw.get("vertstrans", True), glob_rot=kw.get("glob_rot"), num_person=kw.get("P", 1), beta=kw.get("beta", 0),
                  frame_betas=kw.get("frame_betas"))
    m = None if mask is None else torch.from_numpy(mask)
    r64 = rot2joints_ref(x, m, body, regs, jmap, root, dtype=torch.float64, **ref_kw).numpy()
    r32 = rot2joints_ref(x, m, body, regs, jmap, root, dtype=torch.float32, **ref_kw).double().numpy()
    d = float(np.abs(r32 - r64).max())
    top = float(np.abs(r64).max())
    bound = 4 * d if d > 0 else float(np.spacing(np.float32(top)))
    assert got.shape == r64.shape and np.isfinite(got).all(), (label, got.shape, r64.shape)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"{label}: max|xyz| {top:.3f}  fp32 ref {d:.3e}  bound {bound:.3e}  kernel {err:.3e}")
    assert err <= bound, (label, err, bound)
    return r64


def golden_case(g):
    body = golden_body(g)
    regs = golden_regs(g, body)
    t = str(g["jointstype"])
    mask = None if bool(g["mask_none"]) else g["mask"]
    s = golden_settings(g)
    kw = dict(pose_rep=s["pose_rep"], translation=s["translation"], glob=s["glob"], vertstrans=s["vertstrans"], P=s["num_person"], glob_rot=s["glob_rot"],
              beta=s["beta"])
    if g["betas"].size:
        kw["frame_betas"] = rows_to_frames(g["betas"], mask, g["x"].shape[0], g["x"].shape[-1], s["num_person"])
    return body, regs, t, mask, kw


# ---- 1 ----
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(golden, name):
    g = golden(name)
    body, regs, t, mask, kw = golden_case(g)
    jmap, root = regs["joint_maps"][t], regs["map_roots"][t]
    r64 = check(name, run_kernel(body, regs, jmap, root, g["x"], mask, **kw), g["x"], mask, body, regs, jmap, root, **kw)
    assert float(np.abs(r64 - g["expected"]).max()) < 1e-12          # (the restatement is the recorded reference run)


# ---- 2 ----  (B, T) x persons; |S| on V, (Np, Jr), skeleton and mask cycle so that every value of each axis appears. |S| = 0: a dense regressor, |S| = V
RANDOM = [(1, 1, 1, 33, 1, (7, 0), "one", "none"), (1, 1, 2, 70, 31, (0, 5), "pair", "ragged"),
          (3, 7, 1, 130, 32, (21, 9), "tree24", "false"), (3, 7, 2, 1000, 33, (16, 16), "tree55", "none"),
          (2, 61, 1, 70, 70, (21, 9), "chain64", "ragged"), (2, 61, 2, 1000, 0, (0, 5), "tree24", "ragged"),
          (5, 64, 1, 130, 70, (16, 16), "tree55", "ragged"), (5, 64, 2, 33, 0, (21, 9), "one", "none")]
assert {c[:2] for c in RANDOM} == {(1, 1), (3, 7), (2, 61), (5, 64)} and {c[3] for c in RANDOM} == {33, 70, 130, 1000}
assert {c[4] for c in RANDOM} == {1, 31, 32, 33, 70, 0} and {c[5] for c in RANDOM} == {(21, 9), (0, 5), (7, 0), (16, 16)}
assert {c[6] for c in RANDOM} == {"one", "pair", "tree24", "tree55", "chain64"} and {c[7] for c in RANDOM} == {"none", "ragged", "false"}


@pytest.mark.parametrize("B,T,P,V,nS,counts,skel,mask_kind", RANDOM)
def test_random_cases(B, T, P, V, nS, counts, skel, mask_kind):
    body = make_body(skel, V)
    J = len(body["parents"])
    rng = np.random.Generator(np.random.PCG64(B * 1000 + T * 10 + P))
    regs = make_regs(V, nS or V, counts[0], counts[1], rng, dense=nS == 0)
    jmap, root = random_map(J, counts[0], counts[1], int(rng.integers(5, 65)), rng)
    mask = make_mask(mask_kind, B, T, rng)
    x = make_x(rng, B, T, J, "rot6d", True, True, P)
    check(f"B{B} T{T} P{P} V{V} |S|{nS or V} Np,Jr{counts} {skel} mask={mask_kind} n_map={len(jmap)} root={root}",
          run_kernel(body, regs, jmap, root, x, mask, P=P), x, mask, body, regs, jmap, root, P=P)


@pytest.mark.parametrize("pose_rep,translation,glob,vertstrans", [("rotvec", True, True, True), ("rotquat", True, False, True), ("rotmat", False, True, True),
                                                                   ("rot6d", True, True, False)])
def test_random_settings(pose_rep, translation, glob, vertstrans):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(78))
    B, T, P = 2, 61, 2
    regs = make_regs(130, 33, 21, 9, rng)
    jmap, root = random_map(55, 21, 9, 40, rng)
    mask = make_mask("ragged", B, T, rng)
    x = make_x(rng, B, T, 55, pose_rep, translation, glob, P)
    kw = dict(pose_rep=pose_rep, translation=translation, glob=glob, vertstrans=vertstrans, P=P, glob_rot=None if glob else np.array([0.3, -2.0, 1.1], np.float32))
    check(f"B2 T61 P2 tree55 {pose_rep} trans={int(translation)} glob={int(glob)} vertstrans={int(vertstrans)}",
          run_kernel(body, regs, jmap, root, x, mask, **kw), x, mask, body, regs, jmap, root, **kw)


# ---- 3 ----
def test_picked_rows_are_the_vertices_of_rgn_rot2verts_bit_for_bit():
    """Pose blend shapes and betas. The root row is chain joint 0, whose posed position is its rest position itself; that joint is put at the
    origin for every shape, so that undoing the root row is exact (v - 0 is v, and the root row is an output: it must be 0), and without a
    translation the picked rows are then the skinned vertices as rgn_rot2verts writes them."""
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(31))
    regs = make_regs(130, 70, 21, 9, rng)
    B, T = 3, 40
    x = make_x(rng, B, T, 55, "rot6d", True, True, 1)
    mask = make_mask("ragged", B, T, rng)
    from regennet_amd.model.rotation2xyz import Rotation2xyz
    rj, sj = body["rest_joints"].copy(), body["shape_joints"].copy()
    rj[0], sj[0] = 0, 0
    body = dict(body, rest_joints=rj, shape_joints=sj)
    assert not Rotation2xyz(body).rest_joints(beta=1.5)[0].any()
    jmap = np.r_[0, 55 + np.arange(21), 3].astype(np.int32)         # root row, every picked vertex, a chain joint
    got = run_kernel(body, regs, jmap, 0, x, mask, vertstrans=False, beta=1.5)
    verts = run_verts(body, x, mask, vertstrans=False, beta=1.5)
    assert not got[:, 0].any() and np.abs(verts).max() > 0.1
    assert np.array_equal(got[:, 1:22], verts[:, regs["vertex_joints"]])
    assert (got[:, 1:22] == verts[:, regs["vertex_joints"]]).all()


# ---- 4 ----
def test_skeleton_rows_are_the_joints_of_rgn_rot2xyz(tiny):
    eng = tiny[3]
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(32))
    regs = make_regs(130, 33, 21, 9, rng)
    B, T, P = 2, 61, 2
    x = make_x(rng, B, T, 55, "rot6d", True, True, P)
    mask = make_mask("ragged", B, T, rng)
    jmap = np.r_[np.arange(55)[::-1], 60, 80].astype(np.int32)       # the root row (54) is chain joint 0, as rgn_rot2xyz subtracts it
    got = run_kernel(body, regs, jmap, 54, x, mask, P=P)[:, :55][:, ::-1]
    want =run_skeleton_joints(eng, x, mask, body, P=P)
    tol = 4 * float(np.spacing(np.float32(np.abs(want).max())))
    # joints 22 - 24 take the identity in the body's chain (identity_joints) but their rows' rotations in rgn_rot2xyz: leaves, so only their
    # own positions are the same either way and every joint can be compared
    err = float(np.abs(got.astype(np.float64) - want).max())
    bits = np.array_equal(got.view(np.int32), want.view(np.int32))
    print(f"skeleton rows vs rgn_rot2xyz: max difference {err:.3e} (4 spacings: {tol:.3e}); bit-equal: {bits}")
    assert err <= tol


# ---- 5 ----
def test_rows_do_not_depend_on_the_batch():
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(33))
    regs = make_regs(130, 70, 21, 9, rng)
    jmap, root = random_map(55, 21, 9, 49, rng)
    for P in (1, 2):
        x = make_x(rng, 5, 64, 55, "rot6d", True, True, P)
        mask = make_mask("ragged", 5, 64, rng)
        full = run_kernel(body, regs, jmap, root, x, mask, P=P)
        for b in range(5):
            one = run_kernel(body, regs, jmap, root, x[b:b + 1], mask[b:b + 1], P=P)
            assert np.array_equal(full[b:b + 1].view(np.int32), one.view(np.int32)), (P, b)


def test_the_body_cut_to_the_touched_vertices_gives_the_same_bits():
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(34))
    regs = make_regs(130, 33, 21, 9, rng)
    jmap, root = random_map(55, 21, 9, 49, rng)
    x = make_x(rng, 3, 40, 55, "rot6d", True, True, 1)
    S = touched(regs, 130)
    m = body["mesh"]
    small = dict(body, mesh=dict(m, v_template=m["v_template"][S], lbs_weights=m["lbs_weights"][S], shapedirs=m["shapedirs"][S], faces=None,
                                 posedirs=np.ascontiguousarray(m["posedirs"].reshape(-1, 130, 3)[:, S].reshape(-1, 3 * len(S)))))
    at = {int(v): i for i, v in enumerate(S)}
    cut = {"vertex_joints": np.array([at[int(v)] for v in regs["vertex_joints"]], np.int32), "J_regressor_extra": regs["J_regressor_extra"][:, S]}
    full = run_kernel(body, regs, jmap, root, x, None, beta=1.5)
    part = run_kernel(small, cut, jmap, root, x, None, beta=1.5)
    assert np.array_equal(full.view(np.int32), part.view(np.int32))


# ---- 6 ----
@pytest.mark.parametrize("shaped", [False, True])
def test_captured_in_a_graph_the_replay_equals_the_eager_call(shaped):
    body = make_body("tree55", 130)
    rng = np.random.Generator(np.random.PCG64(35))
    regs = make_regs(130, 70, 21, 9, rng)
    jmap, root = random_map(55, 21, 9, 49, rng)
    x = make_x(rng, 3, 61, 55, "rot6d", True, True, 2)
    mask = make_mask("ragged", 3, 61, rng)
    fb = expand_betas(rng.standard_normal((3, 2, 10)).astype(np.float32), 3, 2, 61) if shaped else None
    eager, replay = run_kernel(body, regs, jmap, root, x, mask, P=2, graph=True, frame_betas=fb)
    assert np.isfinite(replay).all() and np.array_equal(eager.view(np.int32), replay.view(np.int32))


# ---- 7 ----
@pytest.mark.parametrize("shaped", [False, True])
def test_masked_frames_are_never_read_into_the_result(shaped):
    body = make_body("tree24", 70)
    rng = np.random.Generator(np.random.PCG64(36))
    regs = make_regs(70, 33, 21, 9, rng)
    jmap, root = random_map(24, 21, 9, 49, rng)
    B, T = 3, 70
    x = make_x(rng, B, T, 24, "rot6d", True, True, 1)
    mask = make_mask("ragged", B, T, rng)
    mask[1] = False                                                 # (and whole tiles of masked frames)
    fb = expand_betas(rng.standard_normal((B, 1, T, 10)).astype(np.float32), B, 1, T) if shaped else None
    clean = run_kernel(body, regs, jmap, root, x, mask, frame_betas=fb)
    y = x.copy()
    y[:, :24][np.broadcast_to(~mask[:, None, None, :], y[:, :24].shape)] = np.nan       # the rotation rows of masked frames (the translation row is added)
    dirty = run_kernel(body, regs, jmap, root, y, mask, frame_betas=fb, nan_masked_betas=shaped)
    assert np.isfinite(dirty).all() and np.array_equal(clean.view(np.int32), dirty.view(np.int32))


# ---- 8 ----
def test_the_workspace_does_not_grow_with_V():
    """The relation implemented: bytes = 4 x (3 Sp [one shape only] + ntiles x 32 x (4 + 12 J + 9 (J - 1) [+ nbp, per-frame shapes] + 3 J)), Sp = |S|
    rounded up to 32 (at least 32), ntiles = ceil(B P T / 32): V does not appear. Against the vertex array [B, V, 3 P, T] it is smaller at V = 1000
    (and at a body model's size); at V = 130 the chain's own outputs - 12 J + 9 (J - 1) + 3 J floats a frame - outweigh 3 V."""
    B, T, P, J = 4, 61, 2, 24
    ntiles = (B * P * T + 31) // 32
    sizes = {}
    for V in (130, 1000):
        body = make_body("tree24", V)
        regs = make_regs(V, 33, 21, 9, np.random.Generator(np.random.PCG64(37)))
        eng = _lib.BodyEngine(body["mesh"], J, 0)
        try:
            eng.set_joint_regressors(regs["vertex_joints"], regs["J_regressor_extra"])
            sizes[V] = (eng.joints_workspace_bytes(B, T, P), eng.joints_workspace_bytes_shaped(B, T, P), eng.workspace_bytes(B, T, P))
        finally:
            eng.close()
    per_tile = 32 * (4 + 12 * J + 9 * (J - 1) + 3 * J)
    assert sizes[130][:2] == sizes[1000][:2] == (4 * (3 * 64 + ntiles * per_tile), 4 * ntiles * (per_tile + 32 * 16))       # (nbp: 10 betas padded to 16)
    assert sizes[1000][2] > sizes[130][2]                           # (rgn_rot2verts's does grow: its shaped template)
    assert sizes[1000][0] < B * 1000 * 3 * P * T * 4


# ---- 9 ----
def test_shaped_calls():
    body = make_body("tree24", 70)
    rng = np.random.Generator(np.random.PCG64(38))
    regs = make_regs(70, 33, 21, 9, rng)
    jmap, root = random_map(24, 21, 9, 49, rng)
    B, T, P = 3, 40, 2
    x = make_x(rng, B, T, 24, "rot6d", True, True, P)
    mask = make_mask("ragged", B, T, rng)
    one = np.zeros(10, np.float32)
    one[1] = 1.5
    same = expand_betas(np.broadcast_to(one, (B, 10)), B, P, T)      # betas_per_motion with equal rows: the one-shape call's values within the bound
    got = run_kernel(body, regs, jmap, root, x, mask, P=P, frame_betas=same)
    check("betas_per_motion, equal rows, against the one-shape restatement", got, x, mask, body, regs, jmap, root, P=P, beta=1.5)
    rows = expand_betas(rng.standard_normal((B, P, 10)).astype(np.float32), B, P, T)
    check("betas_per_motion [B, P, nb], differing rows", run_kernel(body, regs, jmap, root, x, mask, P=P, frame_betas=rows), x, mask, body, regs, jmap, root,
          P=P, frame_betas=rows)
    frames = expand_betas(rng.standard_normal((B, P, T, 3)).astype(np.float32), B, P, T)
    check("a shape per frame, 3 betas", run_kernel(body, regs, jmap, root, x, mask, P=P, frame_betas=frames), x, mask, body, regs, jmap, root, P=P,
          frame_betas=frames)


# ---- 10 ----
def test_model_rot2xyz_serves_the_joint_types(tiny, golden):
    cfg, model, diffusion, eng = tiny
    for name in ("rot2joints_vibe_p1", "rot2joints_a2mpl_p2_ragged", "rot2joints_vibe_frame_betas"):
        g = golden(name)
        body, regs, t, mask, kw = golden_case(g)
        body["mesh"].update(regs)
        model.set_skeleton(body)
        try:
            betas = torch.from_numpy(g["betas"]) if g["betas"].size else None
            out = model.rot2xyz(x=torch.from_numpy(g["x"]), mask=None if mask is None else torch.from_numpy(mask), pose_rep=kw["pose_rep"],
                                translation=kw["translation"], glob=kw["glob"], jointstype=t, vertstrans=kw["vertstrans"], betas=betas, beta=kw["beta"],
                                glob_rot=kw["glob_rot"], num_person=kw["P"])
            assert tuple(out.shape) == g["expected"].shape
            check(f"model.rot2xyz {name}", out.cpu().numpy(), g["x"], mask, body, regs, regs["joint_maps"][t], regs["map_roots"][t], **kw)
            if name.endswith("vibe_p1"):
                out2, rots, root_rot = model.rot2xyz(x=torch.from_numpy(g["x"]), mask=None, pose_rep="rot6d", translation=True, glob=True, jointstype=t,
                                                     vertstrans=True, get_rotations_back=True)
                assert torch.equal(out2, out) and tuple(rots.shape) == (21, 23, 3, 3) and tuple(root_rot.shape) == (21, 3, 3)
                per_motion = model.rot2xyz(x=torch.from_numpy(g["x"]), mask=None, pose_rep="rot6d", translation=True, glob=True, jointstype="a2m",
                                           vertstrans=True, betas_per_motion=torch.zeros(3, 10))
                assert tuple(per_motion.shape) == (3, 18, 3, 7)
                without = dict(body, mesh=dict(body["mesh"], joint_maps={"vibe": regs["joint_maps"]["vibe"]}))
                model.set_skeleton(without)
                with pytest.raises(NotImplementedError, match="map_a2m"):
                    model.rot2xyz(x=torch.from_numpy(g["x"]), mask=None, pose_rep="rot6d", translation=True, glob=True, jointstype="a2m", vertstrans=True)
        finally:
            model.set_skeleton(None)


def test_cgenerate_writes_the_joint_type(tmp_path):
    from regennet_amd.sample import cgenerate
    out = cgenerate.main(["--synthetic", "--num_samples", "2", "--num_repetitions", "1", "--timestep_respacing", "ddim5", "--use_ddim",
                          "--guidance_param", "2.5", "--skeleton", "synthetic", "--jointstype", "a2m", "--output_dir", str(tmp_path)])
    res = np.load(out, allow_pickle=True).item()
    assert res["motion"].shape == (2, 18, 3, 60)
    body = synth.make_body(55)
    regs = synth.make_joint_regressors(body)
    check("cgenerate --skeleton synthetic --jointstype a2m", res["motion"], res["output"], np.ones((2, 60), bool), body, regs, regs["joint_maps"]["a2m"], 0)


def test_argument_errors_that_need_a_body():
    body = make_body("pair", 40)
    eng = _lib.BodyEngine(body["mesh"], 2, 0)
    lib = eng.lib
    vp = ctypes.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)      # noqa: E731
    x, out = torch.zeros(1, 3, 6, 2, device="cuda"), torch.zeros(1, 3, 3, 2, device="cuda")
    rest, par = np.zeros((2, 3), np.float32), np.array([-1, 0], np.int32)
    work = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def call(jmap=(0, 2, 4), root=0, nbytes=None, be=None):
        jm = np.asarray(jmap, np.int32)
        rc = lib.rgn_rot2joints(eng.h, _lib._ptr(x), None, 1, 2, p(rest), p(par), 0, 1, 3, None, p(be), len(jm), p(jm), root, _lib._ptr(out), None,
                                _lib._ptr(work), work.numel() if nbytes is None else nbytes, None)
        return rc, (lib.rgn_body_last_error(eng.h) or b"").decode()

    try:
        n = ctypes.c_uint64()
        rc, err = call()
        assert rc == -1 and "no joint regressors" in err, (rc, err)
        assert lib.rgn_rot2joints_workspace(eng.h, 1, 2, 1, ctypes.byref(n)) == -1
        with pytest.raises(_lib.RgnError, match=r"vertex_joints\[1\] outside"):
            eng.set_joint_regressors(np.array([0, 40]), None)
        with pytest.raises(_lib.RgnError, match="not finite"):
            eng.set_joint_regressors(None, np.full((1, 40), np.inf, np.float32))
        with pytest.raises(_lib.RgnError, match="> 32"):
            eng.set_joint_regressors(np.arange(33), None)
        eng.set_joint_regressors(np.array([5, 7]), np.ones((1, 40), np.float32))
        eng.set_joint_regressors(np.array([5, 7]), np.eye(40, dtype=np.float32)[:1])        # again: replaced
        assert lib.rgn_rot2joints_workspace(eng.h, 1, 2, 1, ctypes.byref(n)) == 0 and n.value <= work.numel()
        assert call()[0] == 0
        for kw, text in ((dict(jmap=(0, 5)), "map[1] = 5 outside"), (dict(jmap=(0, -1)), "map[1] < 0"), (dict(root=3), "root outside"), (dict(root=-1), "root outside"),
                         (dict(jmap=()), "n_map outside"), (dict(jmap=[0] * 65), "n_map outside"), (dict(nbytes=n.value - 1), "workspace")):
            rc, err = call(**kw)
            assert rc == -1 and text in err, (kw, rc, err)
        torch.cuda.synchronize()
    finally:
        eng.close()
