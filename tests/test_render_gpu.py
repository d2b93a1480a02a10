"""GPU: rgn_render / utils.render.MeshRenderer against the NumPy oracle of its contract (tests/render_ref.py).

Every test here fails on the commit before the renderer: the rgn_render_* symbols, _lib.RenderEngine and utils.render.MeshRenderer do not exist
there, and cgenerate has no --render_dir.

Scenes: synth.make_body(55, 130, seed=0) and make_body(24, 70, seed=24) in their rest pose, a second copy shifted by (0.35, 0, 0.1) as person 1,
centred and scaled so that frame 0 fills 90 % of the image under cam = (0.75, 0.75, 0, 0). B = 2 (motion 1 is motion 0 mirrored in x), T = 3
(frame t is shifted by 0.02 t in x, so the later frames hang over the image's edge), frame 1 of motion 1 masked.

Bounds. Coverage is integer arithmetic: the covered / background masks must be bit-equal. The winner may differ from the oracle's only at
near-tie pixels, where the oracle's nearest and second-nearest depths (of different faces) lie within 1e-5: the fp32 interpolation error is about
3 x 2^-24 |z| < 2e-7 at |z| < 1 (asserted of the scenes: they reach 0.84 and 0.91), so 1e-5 is a 50-fold margin; such pixels may be at most 1 % of the covered ones, which
is first asserted of the oracle itself. Depth within 1e-5 and colour within 1 level (only the final rounding can differ) where the winners agree."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from regennet_amd import synth
from tests import render_ref as rr
from tests.test_render_cpu import _decode_png

pytestmark = pytest.mark.gpu

CAM = (0.75, 0.75, 0.0, 0.0)
SCENES = {"b55": (55, 130, 0), "b24": (24, 70, 24)}
TIE, TIE_SHARE = 1e-5, 0.01
CASES = [(s, w, h) for s in SCENES for (w, h) in ((64, 64), (96, 80), (33, 17))] + [("b24", 1024, 1024)]   # 1024^2: one frame, 256 tiles


@functools.lru_cache(maxsize=None)
def scene(name):
    """(verts fp32 [2, V, 6, 3], faces int32 [F, 3], mask bool [2, 3])"""
    body = synth.make_body(*SCENES[name][:2], seed=SCENES[name][2])
    vt, faces = body["mesh"]["v_template"].astype(np.float64), body["mesh"]["faces"]
    both = np.stack([vt, vt + np.array([0.35, 0.0, 0.1])], axis=1)                       # [V, 2, 3]
    lo, hi = both.reshape(-1, 3).min(0), both.reshape(-1, 3).max(0)
    both = (both - 0.5 * (lo + hi)) * (0.9 / 0.75 / (0.5 * (hi - lo)[:2].max()))
    assert np.abs(both[..., 2]).max() < 1.0
    frames = np.stack([both + np.array([0.02 * t, 0.0, 0.0]) for t in range(3)], axis=-1)  # [V, 2, 3, T]
    m0 = frames.reshape(len(vt), 6, 3)
    m1 = (frames * np.array([-1.0, 1.0, 1.0])[None, None, :, None]).reshape(len(vt), 6, 3)
    mask = np.ones((2, 3), bool)
    mask[1, 1] = False
    return np.stack([m0, m1]).astype(np.float32), np.ascontiguousarray(faces, dtype=np.int32), mask


def case_inputs(name, W, H):
    verts, faces, mask = scene(name)
    if W >= 1024:
        return np.ascontiguousarray(verts[:1, :, :, :1]), faces, None
    return verts, faces, mask


@functools.lru_cache(maxsize=None)
def renderer(name, perm_seed=None):
    from regennet_amd.utils.render import MeshRenderer
    faces = scene(name)[1]
    if perm_seed is not None:
        faces = faces[np.random.Generator(np.random.PCG64(perm_seed)).permutation(len(faces))]
    return MeshRenderer(faces, "cuda:0")


def gpu_render(r, verts, mask, W, H, **kw):
    rgb, depth, face = r.render(torch.from_numpy(verts).cuda(), None if mask is None else torch.from_numpy(mask).cuda(), width=W, height=H,
                                return_buffers=True, **{"cam": CAM, "center": False, **kw})
    torch.cuda.synchronize()
    return {"rgb": rgb.cpu().numpy(), "depth": depth.cpu().numpy(), "face": face.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def both(name, W, H):
    """(the device's buffers, the oracle's) for a case: computed once, shared by the tests below, not modified."""
    verts, faces, mask = case_inputs(name, W, H)
    got = gpu_render(renderer(name), verts, mask, W, H)
    ref = rr.render(verts, faces, mask=mask, width=W, height=H, cam=CAM, center=False)
    return got, ref


@pytest.mark.parametrize("name,W,H", CASES)
def test_winner_buffer_matches_the_oracle(name, W, H):
    got, ref = both(name, W, H)
    covered = ref["face"] >= 0
    near = rr.near_tie(ref, TIE)
    print(f"{name} {W}x{H}: covered {covered.sum()}, oracle near-tie {near.sum()} ({near.sum() / covered.sum():.4%}), "
          f"winner differs at {(got['face'] != ref['face']).sum()}")
    assert covered.sum() > 0.05 * covered.size
    assert near.sum() <= TIE_SHARE * covered.sum(), "the scene itself has too many near-ties for the test to mean anything"
    assert np.array_equal(got["face"] >= 0, covered), "coverage is integer arithmetic: no tolerance"
    differ = got["face"] != ref["face"]
    assert not (differ & ~near).any(), f"{(differ & ~near).sum()} pixels with another winner than the oracle's away from any near-tie"


@pytest.mark.parametrize("name,W,H", CASES)
def test_depth_matches_the_oracle(name, W, H):
    got, ref = both(name, W, H)
    same = (got["face"] == ref["face"]) & (ref["face"] >= 0)
    err = np.abs(got["depth"][same].astype(np.float64) - ref["depth"][same]).max()
    print(f"{name} {W}x{H}: max |depth - oracle| = {err:.3e} over {same.sum()} pixels")
    assert err <= 1e-5
    assert np.all(np.isposinf(got["depth"][ref["face"] < 0])) and np.all(got["face"][ref["face"] < 0] == -1)


@pytest.mark.parametrize("name,W,H", CASES)
def test_colour_matches_the_oracle(name, W, H):
    got, ref = both(name, W, H)
    same = (got["face"] == ref["face"]) & (ref["face"] >= 0)
    err = np.abs(got["rgb"][same].astype(np.int32) - ref["rgb"][same].astype(np.int32))
    print(f"{name} {W}x{H}: max |rgb - oracle| = {err.max()} level(s), {np.count_nonzero(err)} of {err.size} values differ")
    assert err.max() <= 1
    assert np.all(got["rgb"][ref["face"] < 0] == 255), "background pixels are exactly the background colour"
    assert len(np.unique(got["rgb"][same].reshape(-1, 3), axis=0)) > 20, "shaded, not flat"


@pytest.mark.parametrize("name", list(SCENES))
def test_face_order_does_not_matter_and_calls_repeat_bit_for_bit(name):
    W, H = 96, 80
    verts, faces, mask = case_inputs(name, W, H)
    got, ref = both(name, W, H)
    again = gpu_render(renderer(name), verts, mask, W, H)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    seed = 7
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(len(faces))              # permuted face q is original face perm[q]
    other = gpu_render(renderer(name, seed), verts, mask, W, H)
    assert np.array_equal(other["depth"], got["depth"])
    F = len(faces)
    back = np.where(other["face"] >= 0, (other["face"] // F) * F + perm[np.maximum(other["face"], 0) % F], -1)
    differ = back != got["face"]
    # The face buffers may differ only where two faces have the SAME fp32 depth at the pixel: the lower index wins, and the permutation changes
    # which that is. Such a pixel is identified from depth: the contract's fp32 depth (rr.depth_f32, the kernel's arithmetic operation by
    # operation) of BOTH faces at that pixel must equal the depth buffer's value, bit for bit.
    for b, t, y, x in np.argwhere(differ):
        pos, scr = rr.project(verts, mask, b, t, CAM, W, H, False)
        for g in (int(got["face"][b, t, y, x]), int(back[b, t, y, x])):
            assert g >= 0 and rr.depth_f32(pos[g // F], scr[g // F], faces[g % F], int(x), int(y)) == got["depth"][b, t, y, x], (b, t, y, x, g)
    print(f"{name}: {differ.sum()} pixel(s) with an exact fp32 depth tie between two faces")
    assert np.array_equal(other["rgb"][~differ], got["rgb"][~differ]) and differ.sum() <= TIE_SHARE * (got["face"] >= 0).sum()


def test_an_exact_depth_tie_goes_to_the_lower_face_index_in_any_order():
    """Faces 0 - 2 appended once more at the end of the table: wherever one of them is nearest, two faces tie EXACTLY. In table order the original
    (lower index) wins; with the table reversed the copy comes first and wins. Depth and colour do not change, and at every pixel where the face
    buffers differ the contract's fp32 depth of both faces (rr.depth_f32) equals the depth buffer bit for bit."""
    from regennet_amd.utils.render import MeshRenderer
    name, W, H = "b24", 96, 80
    verts, faces, mask = scene(name)
    F = len(faces)
    twice = np.concatenate([faces, faces[:3]])
    perm = np.arange(len(twice))[::-1].copy()
    r1, r2 = MeshRenderer(twice, "cuda:0"), MeshRenderer(twice[perm], "cuda:0")
    got, other = gpu_render(r1, verts, mask, W, H), gpu_render(r2, verts, mask, W, H)
    r1.close(), r2.close()
    F2 = len(twice)
    assert np.array_equal(other["depth"], got["depth"]) and np.array_equal(other["rgb"], got["rgb"])
    back = np.where(other["face"] >= 0, (other["face"] // F2) * F2 + perm[np.maximum(other["face"], 0) % F2], -1)
    differ = back != got["face"]
    assert differ.sum() > 20, "faces 0 - 2 are visible somewhere"
    assert not (got["face"] % F2 >= F)[got["face"] >= 0].any() and np.all(back[differ] % F2 == got["face"][differ] % F2 + F)
    where = np.argwhere(differ)
    for b, t, y, x in where[::max(1, len(where) // 200)]:
        pos, scr = rr.project(verts, mask, b, t, CAM, W, H, False)
        for g in (int(got["face"][b, t, y, x]), int(back[b, t, y, x])):
            assert rr.depth_f32(pos[g // F2], scr[g // F2], twice[g % F2], int(x), int(y)) == got["depth"][b, t, y, x], (b, t, y, x, g)


def engine_render(eng, verts, mask, W, H, cam, center, work=None):
    """_lib.RenderEngine.render, ONE rgn_render call for all of verts [B, V, 3 P, T]: dict of numpy buffers."""
    B, _, C3, T = verts.shape
    P = C3 // 3
    v = torch.from_numpy(np.ascontiguousarray(verts)).cuda()
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda().to(torch.uint8)
    if work is None:
        work = torch.empty(eng.workspace_bytes(B, T, P, W, H), dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((B, T, H, W, 3), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((B, T, H, W), dtype=torch.float32, device="cuda")
    face = torch.zeros((B, T, H, W), dtype=torch.int32, device="cuda")
    eng.render(v, m, P, eng.params(W, H, cam, center, rr.DEFAULT_COLORS, (1, 1, 1)), rgb, depth, face, work, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {"rgb": rgb.cpu().numpy(), "depth": depth.cpu().numpy(), "face": face.cpu().numpy()}


@pytest.mark.parametrize("name,W,H", [("b55", 64, 64), ("b24", 96, 80)])
def test_one_call_for_two_motions_equals_one_call_per_motion_and_frame(name, W, H):
    """rgn_render itself with B = 2, T = 3 in ONE call (MeshRenderer issues one call per motion, so nothing above runs the per-motion indexing:
    the centroid's workgroup per motion, the mask's and the input's motion stride, the frame index across motions in every pass): frame 1 of
    motion 1 masked, centring on, workspace of workspace_bytes(2, 3, 2, ...). Bit-equal to one B = 1, T = 1 call per frame on vertices centred
    beforehand with the oracle's centroid of that motion; covered pixels equal to the oracle's."""
    from regennet_amd import _lib
    verts, faces, mask = scene(name)
    verts = (verts + np.float32([0.25, -0.125, 0.0625] * 2)[None, None, :, None]).astype(np.float32)
    cam = (0.75, 0.75, 0.0, 0.10)
    eng = _lib.RenderEngine(faces, verts.shape[1], 0)
    assert eng.workspace_bytes(2, 3, 2, W, H) > eng.workspace_bytes(1, 3, 2, W, H)
    for m in (mask, np.array([[True, True, True], [False, False, True]])):
        got = engine_render(eng, verts, m, W, H, cam, True)
        c = np.stack([rr.centroid(verts, m, b) for b in range(2)])
        assert np.abs(c[0] - c[1]).max() > 0.1, "the two motions have different centroids"
        pre = (verts.reshape(2, -1, 2, 3, 3) - c[:, None, None, :, None]).reshape(verts.shape).astype(np.float32)
        for b in range(2):
            for t in range(3):
                if not m[b, t]:
                    assert np.all(got["face"][b, t] == -1) and np.all(np.isposinf(got["depth"][b, t])) and np.all(got["rgb"][b, t] == 255)
                    continue
                one = engine_render(eng, pre[b:b + 1, :, :, t:t + 1], None, W, H, cam, False)
                for k in got:
                    assert np.array_equal(one[k][0, 0], got[k][b, t]), (k, b, t)
        ref = rr.render(verts, faces, mask=m, width=W, height=H, cam=cam, center=True)
        assert np.array_equal(got["face"] >= 0, ref["face"] >= 0) and (got["face"] >= 0).sum() > 500
        differ = got["face"] != ref["face"]
        assert not (differ & ~rr.near_tie(ref, TIE)).any()
        same = ~differ & (ref["face"] >= 0)
        assert np.abs(got["depth"][same].astype(np.float64) - ref["depth"][same]).max() <= 1e-5
        assert np.abs(got["rgb"][same].astype(np.int32) - ref["rgb"][same].astype(np.int32)).max() <= 1
    # the same call through MeshRenderer (one call per motion) gives the same buffers
    via = gpu_render(renderer(name), verts, mask, W, H, cam=cam, center=True)
    got = engine_render(eng, verts, mask, W, H, cam, True)
    for k in got:
        assert np.array_equal(via[k], got[k]), k
    eng.close()


def test_batch_independence_masked_frames_and_centring():
    name, W, H = "b55", 64, 64
    verts, faces, mask = scene(name)
    got, _ = both(name, W, H)
    r = renderer(name)
    for b in range(2):
        for t in range(3):
            if not mask[b, t]:
                assert np.all(got["face"][b, t] == -1) and np.all(np.isposinf(got["depth"][b, t])) and np.all(got["rgb"][b, t] == 255)
                continue
            one = gpu_render(r, np.ascontiguousarray(verts[b:b + 1, :, :, t:t + 1]), None, W, H)
            for k in got:
                assert np.array_equal(one[k][0, 0], got[k][b, t]), (k, b, t)
    # centring: motion 1's first unmasked frame is frame 0; with frame 0 masked too it is frame 2
    cam = (0.75, 0.75, 0.0, 0.10)
    for m in (mask, np.array([[True, True, True], [False, False, True]])):
        shifted = verts + np.float32(0.25)
        cen = gpu_render(r, shifted, m, W, H, cam=cam, center=True)
        c = np.stack([rr.centroid(shifted, m, b) for b in range(2)])                        # fp32 [2, 3]
        pre = (shifted.reshape(2, -1, 2, 3, 3) - c[:, None, None, :, None]).reshape(shifted.shape).astype(np.float32)
        want = gpu_render(r, pre, m, W, H, cam=cam, center=False)
        for k in cen:
            assert np.array_equal(cen[k], want[k]), k
        ref = rr.render(shifted, faces, mask=m, width=W, height=H, cam=cam, center=True)
        assert np.array_equal(cen["face"] >= 0, ref["face"] >= 0) and (cen["face"] >= 0).sum() > 500


def test_edges_of_the_domain():
    """A triangle far larger than the image, one wholly off-screen, vertices beyond the +-2^20 clamp (4096 pixels), zero-area triangles and a
    single-pixel triangle, each on a depth plane of its own, and a repeated face (an exact tie in depth: the lower index wins)."""
    from regennet_amd.utils.render import MeshRenderer
    W = H = 32
    ident = (1.0, 1.0, 0.0, 0.0)                                                             # col = 16 (1 + X)
    pts = [(-50, -40, 0.5), (60, -45, 0.5), (3, 70, 0.5),                                    # 0-2 huge
           (2.0, 2.0, 0.1), (3.0, 2.0, 0.1), (2.0, 3.5, 0.1),                                # 3-5 off-screen
           (-300.0, -0.5, 0.3), (300.0, -0.45, 0.3), (0.1, 0.2, 0.3),                        # 6-8 beyond the clamp on both sides
           (0.0, 0.0, 0.0), (0.25, 0.25, 0.0), (0.5, 0.5, 0.0),                              # 9-11 collinear
           (-0.55, -0.55, 0.2), (-0.50, -0.54, 0.2), (-0.54, -0.50, 0.2)]                   # 12-14 around the centre of pixel (7, 7) alone
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [9, 9, 10], [12, 13, 14], [0, 1, 2]], np.int32)      # (6 repeats 0: an exact depth tie, 0 wins)
    verts = np.asarray(pts, np.float32).reshape(1, -1, 3, 1)
    ref = rr.render(verts, faces, width=W, height=H, cam=ident, center=False)
    r = MeshRenderer(faces, "cuda:0")
    got = gpu_render(r, verts, None, W, H, cam=ident)
    r.close()
    assert set(np.unique(ref["face"])) == {0, 2, 5} and (ref["face"] == 5).sum() == 1 and ref["face"][0, 0, 7, 7] == 5
    assert np.array_equal(got["face"], ref["face"])
    assert np.abs(got["depth"].astype(np.float64) - ref["depth"]).max() <= 1e-5
    assert np.abs(got["rgb"].astype(np.int32) - ref["rgb"].astype(np.int32)).max() <= 1


def test_a_captured_graph_replays_the_eager_call():
    name, W, H = "b24", 96, 80
    verts, faces, mask = scene(name)
    got, _ = both(name, W, H)
    r = renderer(name)
    v, m = torch.from_numpy(verts).cuda(), torch.from_numpy(mask).cuda()
    kw = dict(width=W, height=H, cam=CAM, center=False, return_buffers=True)
    r.render(v, m, **kw)                                                                     # (handle and workspace exist before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rgb, depth, face = r.render(v, m, **kw)
    rgb.zero_(), depth.zero_(), face.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy(), got["rgb"]) and np.array_equal(depth.cpu().numpy(), got["depth"]) and np.array_equal(face.cpu().numpy(), got["face"])


def test_argument_errors():
    from regennet_amd import _lib
    eng = _lib.RenderEngine(scene("b24")[1], 70, 0)
    v = torch.zeros((1, 70, 3, 2), device="cuda")
    rgb, work = torch.empty((1, 2, 8, 8, 3), dtype=torch.uint8, device="cuda"), torch.empty(eng.workspace_bytes(1, 2, 1, 8, 8), dtype=torch.uint8, device="cuda")
    ok = lambda w=8, h=8: eng.params(w, h, CAM, True, [(0.5, 0.5, 0.5)], (1, 1, 1))
    eng.render(v, None, 1, ok(), rgb, None, None, work, 0)
    for bad, word in ((lambda: eng.render(v, None, 1, ok(0, 8), rgb, None, None, work, 0), "width or height"),
                      (lambda: eng.render(v, None, 1, ok(8, 4097), rgb, None, None, work, 0), "width or height"),
                      (lambda: eng.render(v, None, 1, ok(), rgb, None, None, work[:-16], 0), "workspace of"),
                      (lambda: eng.workspace_bytes(1, 2, 0, 8, 8), "num_person < 1"),
                      (lambda: eng.workspace_bytes(1, 2, 2 ** 31 // 68 + 1, 8, 8), "2^31"),
                      (lambda: eng.workspace_bytes(64, 64, 1, 4096, 4096), "tiles of 64 x 64 pixels")):      # 4096 frames x 4096 tiles = 2^24 workgroups
        with pytest.raises(_lib.RgnError) as e:
            bad()
        assert e.value.code == -1 and word in str(e.value), str(e.value)
    lib = eng.lib
    assert lib.rgn_render(eng.h, None, None, 1, 2, 1, ok(), rgb.data_ptr(), None, None, work.data_ptr(), work.numel(), None) == -1
    assert b"null verts, rgb or work" in lib.rgn_render_last_error(eng.h)
    eng.close()


def test_cgenerate_render_dir_writes_png_sequences(tmp_path):
    from regennet_amd.sample import cgenerate
    png = tmp_path / "png"
    out = cgenerate.main(["--synthetic", "--num_samples", "2", "--num_repetitions", "1", "--timestep_respacing", "ddim5", "--use_ddim", "--skeleton", "synthetic",
                    "--vertices", "--render_dir", str(png), "--render_size", "64", "--output_dir", str(tmp_path)])
    files = sorted(glob.glob(str(png / "sample*" / "frame*.png")))
    assert len(files) == 2 * 60 and files[0].endswith(os.path.join("sample00", "frame000.png")) and files[-1].endswith(os.path.join("sample01", "frame059.png"))
    imgs = np.stack([_decode_png(open(f, "rb").read()) for f in files])
    assert imgs.shape == (120, 64, 64, 3)
    assert all((im != 255).any() for im in imgs), "every frame shows the body"
    # ... and the counterpart of render.crendermotion on the file just written: actor and reactor, smoothed, posed, rendered, cropped
    from regennet_amd.sample import render
    d = render.main(["--data_path", out, "--skeleton", "synthetic", "--num_person", "2", "--setting", "cmdm", "--size", "64", "--out", str(tmp_path / "r")])
    files = sorted(glob.glob(os.path.join(d, "sample*", "frame*.png")))
    assert len(files) == 120
    a, b = _decode_png(open(files[0], "rb").read()), _decode_png(open(files[59], "rb").read())
    assert a.shape == b.shape and a.shape[0] <= 64 and a.shape[1] <= 64 and min(a.shape[:2]) >= 8, "one crop box for all frames of a motion"
    assert (a != 255).any() and (a == np.array([158, 158, 158])).all(-1).sum() == 0, "shaded persons, nothing flat"
