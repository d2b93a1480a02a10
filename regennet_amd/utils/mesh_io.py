"""Plain-text Wavefront OBJ output for the meshes `model.rot2xyz(..., jointstype='vertices')` gives (the reference writes them through
trimesh, visualize/vis_utils.py:43-55; nothing but numpy is needed here)."""
import os

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
