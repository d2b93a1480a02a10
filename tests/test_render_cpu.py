"""CPU: properties of the rasteriser's NumPy oracle (tests/render_ref.py), the PNG writer, rgn_render_create's argument checks (they run before the
device is touched) and the CLI flags. No GPU."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from tests import render_ref as rr

IDENT = (1.0, 1.0, 0.0, 0.0)                            # with W = H = 2 n: col = (1 + X) n, so X = col / n - 1


def _verts(points):
    """[V, 3] -> the [1, V, 3, 1] tensor of one person, one frame."""
    return np.asarray(points, dtype=np.float32).reshape(1, -1, 3, 1)


def _at(cols_rows, n):
    """Pixel coordinates (col, row) -> X, Y under IDENT at W = H = 2 n (exact in fp32 for the half-pixel positions used here)."""
    return [(c / n - 1.0, r / n - 1.0) for c, r in cols_rows]


def test_quad_on_half_pixel_positions_covers_the_analytic_rectangle_once():
    """Corners ON pixel centres (c + 0.5): the top and left edges own their centres, the bottom and right ones do not, and every centre on the
    diagonal the two triangles share is covered by exactly one of them."""
    n = 8
    xy = _at([(2.5, 3.5), (10.5, 3.5), (10.5, 11.5), (2.5, 11.5)], n)
    v = _verts([(x, y, 0.25) for x, y in xy])
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[1, 2, 3], [1, 3, 0]]):
        out = rr.render(v, np.array(faces), width=2 * n, height=2 * n, cam=IDENT, center=False)
        want = np.zeros((2 * n, 2 * n), bool)
        want[3:11, 2:10] = True                            # rows 3.5 .. 10.5, columns 2.5 .. 9.5
        assert np.array_equal(out["face"][0, 0] >= 0, want)
        assert np.array_equal(out["count"][0, 0], want.astype(np.int32)), "a centre on the shared diagonal must belong to exactly one triangle"
        assert np.all(out["depth"][0, 0][want] == 0.25) and np.all(np.isinf(out["depth"][0, 0][~want]))
        assert np.all(out["rgb"][0, 0][~want] == 255)


def _soup(seed, nv=40, nf=60):
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = np.concatenate([rng.uniform(-0.9, 0.9, (nv, 2)), rng.uniform(-0.5, 0.5, (nv, 1))], axis=1)
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)])
    return _verts(pts), faces


def test_permuting_the_faces_leaves_the_depth_image_unchanged():
    v, faces = _soup(1)
    a = rr.render(v, faces, width=48, height=40, cam=IDENT, center=False)
    perm = np.random.Generator(np.random.PCG64(2)).permutation(len(faces))
    b = rr.render(v, faces[perm], width=48, height=40, cam=IDENT, center=False)
    assert (a["face"] >= 0).sum() > 300
    assert np.array_equal(a["depth"], b["depth"]) and np.array_equal(a["second"], b["second"])
    assert np.array_equal(np.where(b["face"] >= 0, perm[np.maximum(b["face"], 0)], -1), a["face"])


def test_a_triangle_and_its_mirror_wound_copy_cover_the_same_pixels():
    v, faces = _soup(3, nf=12)
    for f in faces:
        a = rr.render(v, f[None, :], width=48, height=40, cam=IDENT, center=False)
        b = rr.render(v, f[None, [0, 2, 1]], width=48, height=40, cam=IDENT, center=False)
        assert np.array_equal(a["face"], b["face"]) and np.allclose(a["depth"], b["depth"], rtol=0, atol=1e-12)
        assert np.array_equal(a["rgb"], b["rgb"])          # (two-sided: the normal is turned to the camera either way)


def test_centring_masks_and_zero_area():
    v, faces = _soup(4)
    v2 = np.concatenate([v, v + np.float32(0.125)], axis=3)             # two frames; the second is shifted
    out = rr.render(v2, faces, mask=np.array([[False, True]]), width=32, height=32, cam=IDENT, center=True)
    assert np.all(out["face"][0, 0] == -1) and np.all(out["rgb"][0, 0] == 255)
    c = rr.centroid(v2, np.array([[False, True]]), 0)                     # ... of the first UNMASKED frame
    assert np.allclose(c, v2[0, :, :, 1].mean(0), atol=1e-6)
    ref = rr.render(v2[..., 1:] - c.reshape(1, 1, 3, 1), faces, width=32, height=32, cam=IDENT, center=False)
    assert np.array_equal(out["face"][0, 1], ref["face"][0, 0])
    flat = rr.render(_verts([(0, 0, 0), (0.5, 0.5, 0), (-0.5, -0.5, 0)]), np.array([[0, 1, 2], [0, 0, 1]]), width=16, height=16, cam=IDENT, center=False)
    assert np.all(flat["face"] == -1)


def _decode_png(data):
    """8-bit RGB, non-interlaced, filter 0 on every row: what write_png writes."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert np.all(raw[:, 0] == 0)
    return raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trips(tmp_path):
    from regennet_amd.utils.mesh_io import write_png, write_png_sequences
    rng = np.random.Generator(np.random.PCG64(5))
    for shape in ((1, 1, 3), (17, 33, 3), (64, 64, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        path = write_png(str(tmp_path / "a.png"), img)
        assert np.array_equal(_decode_png(open(path, "rb").read()), img)
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
    frames = rng.integers(0, 256, (2, 3, 4, 5, 3), dtype=np.uint8)
    assert write_png_sequences(str(tmp_path / "seq"), frames, [3, 2]) == 5
    assert np.array_equal(_decode_png((tmp_path / "seq" / "sample01" / "frame001.png").read_bytes()), frames[1, 1])
    assert not (tmp_path / "seq" / "sample01" / "frame002.png").exists()
    with pytest.raises(AssertionError):
        write_png(str(tmp_path / "b.png"), np.zeros((4, 4), np.uint8))


def test_crop_to_content():
    from regennet_amd.utils.render import crop_to_content
    fr = np.full((3, 20, 30, 3), 255, np.uint8)
    assert crop_to_content(fr) is None
    fr[0, 4, 7] = (10, 255, 255)
    fr[2, 11, 5, 2] = 254
    assert crop_to_content(fr) == (4, 5, 12, 8)
    import torch
    assert crop_to_content(torch.from_numpy(fr)) == (4, 5, 12, 8)


def _create(V, F, faces, out=True):
    from regennet_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    f = None if faces is None else np.ascontiguousarray(faces, dtype=np.int32)
    rc = lib.rgn_render_create(0, V, F, None if f is None else f.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h) if out else None)
    err = (lib.rgn_render_last_error(None) or b"").decode()
    if rc == 0:
        assert lib.rgn_render_destroy(h) == 0
    return rc, err


def test_render_create_checks_its_arguments_before_the_device():
    tri = [[0, 1, 2]]
    for V, F, faces, word in ((0, 1, tri, "V outside"), (65537, 1, tri, "V outside"), (3, 0, tri, "F < 1"), (3, 1, None, "null faces"),
                              (3, 1, [[0, 1, 3]], "faces[0][2] = 3 outside [0, V)"), (3, 2, [[0, 1, 2], [-1, 1, 2]], "faces[1][0] = -1 outside")):
        rc, err = _create(V, F, faces)
        assert rc == -1 and word in err, (V, F, rc, err)
    rc, err = _create(3, 1, tri, out=False)
    assert rc == -1 and "null out" in err
    rc, err = _create(3, 1, tri)                            # a good one reaches the device: a handle, or no device
    assert rc == 0 or (rc == -6 and "no HIP device" in err), (rc, err)
    from regennet_amd import _lib
    lib = _lib.load()
    assert lib.rgn_render_destroy(None) == -1 and lib.rgn_render_workspace(None, 1, 1, 1, 8, 8, None) == -1
    assert lib.rgn_render(None, None, None, 1, 1, 1, None, None, None, None, None, 0, None) == -1
    assert ctypes.sizeof(_lib.RgnRenderParams) == 4 * (2 + 4 + 1 + 24 + 3)


def test_render_dir_needs_vertices_like_obj_dir():
    from regennet_amd.sample.cgenerate import set_skeleton
    from regennet_amd.utils.parser_util import cgenerate_args
    a = cgenerate_args(["--synthetic"])
    assert a.render_dir == "" and a.render_size == 1024
    a = cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--vertices", "--render_dir", "out", "--render_size", "64"])
    assert a.render_dir == "out" and a.render_size == 64
    with pytest.raises(SystemExit, match="--render_dir"):
        set_skeleton(None, cgenerate_args(["--synthetic", "--skeleton", "synthetic", "--render_dir", "out"]))
    with pytest.raises(SystemExit, match="--render_dir"):
        set_skeleton(None, cgenerate_args(["--synthetic", "--render_dir", "out"]))
