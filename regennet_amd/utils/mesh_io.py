"""Plain-text Wavefront OBJ output for the meshes `model.rot2xyz(..., jointstype='vertices')` gives (the reference writes them through
trimesh, visualize/vis_utils.py:43-55; nothing but numpy is needed here), and PNG output for the frames utils/render.py draws (the reference
hands them to imageio, render/crendermotion.py:21, 40-42; zlib and struct are enough for 8-bit RGB)."""
import os
import struct
import zlib

import numpy as np


def obj_text(vertices, faces=None):
    """`v x y z` per vertex [V, 3], then `f a b c` per triangle [F, 3] (0-based in, 1-based out)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lines = ["v %.6f %.6f %.6f" % (float(a), float(b), float(c)) for a, b, c in v]
    if faces is not None:
        lines += ["f %d %d %d" % (a + 1, b + 1, c + 1) for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return "\n".join(lines) + "\n"


def write_obj(path, vertices, faces=None):
    with open(path, "w") as f:
        f.write(obj_text(vertices, faces))
    return path


def write_obj_sequences(obj_dir, vertices, faces=None, lengths=None):
    """vertices [N, V, 3, T] -> obj_dir/sample{i:02d}/frame{t:03d}.obj for the first lengths[i] (default T) frames; returns the file count."""
    vertices = np.asarray(vertices)
    n = 0
    for i in range(vertices.shape[0]):
        d = os.path.join(obj_dir, "sample%02d" % i)
        os.makedirs(d, exist_ok=True)
        for t in range(vertices.shape[3] if lengths is None else int(lengths[i])):
            write_obj(os.path.join(d, "frame%03d.obj" % t), vertices[i, :, :, t], faces)
            n += 1
    return n


def png_bytes(rgb):
    """An 8-bit RGB PNG (colour type 2, no interlace, filter 0 on every row) of rgb uint8 [H, W, 3]."""
    a = np.ascontiguousarray(np.asarray(rgb), dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3 and a.shape[0] >= 1 and a.shape[1] >= 1, a.shape
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, 3 * w)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def write_png(path, rgb):
    with open(path, "wb") as f:
        f.write(png_bytes(rgb))
    return path


def write_png_sequences(png_dir, frames, lengths=None, first=0):
    """frames uint8 [N, T, H, W, 3] -> png_dir/sample{first + i:02d}/frame{t:03d}.png for the first lengths[i] (default T) frames; returns the
    file count. `first`: the sample number of frames[0], for a caller that hands the motions over one at a time."""
    n = 0
    for i in range(len(frames)):
        d = os.path.join(png_dir, "sample%02d" % (first + i))
        os.makedirs(d, exist_ok=True)
        for t in range(len(frames[i]) if lengths is None else int(lengths[i])):
            write_png(os.path.join(d, "frame%03d.png" % t), frames[i][t])
            n += 1
    return n
