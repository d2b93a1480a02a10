"""NumPy oracle of rgn_render's contract (include/regennet_hip.h, above rgn_render).

What decides COVERAGE is computed exactly as the contract words it: the centroid (fp64 sum, rounded to fp32), the centred positions and the
projection in fp32 in the stated order, the snap to 1/256 pixel, and from there 64-bit integers (edge functions, winding swap, top-left
ownership). Depth, normals and shading run in fp64 from those fp32 positions. Each triangle is evaluated over its own pixel box only. Per pixel
the oracle returns the winner, its depth and the depth of the nearest DIFFERENT face, so a test can tell a wrong winner from a near-tie."""
import numpy as np

LIGHTS = np.array([[0.0, 1.0, -1.0], [0.0, -1.0, -1.0], [1.0, -1.0, -2.0]])
DEFAULT_CAM = (0.75, 0.75, 0.0, 0.10)
DEFAULT_COLORS = ((0.11, 0.53, 0.8), (0.618, 0.618, 0.618))
SNAP, CLAMP = 256, 1 << 20


def centroid(verts, mask, b):
    """fp32 [3]: the mean over person 0's vertices in motion b's first unmasked frame (zeros when every frame is masked)."""
    T = verts.shape[3]
    live = [t for t in range(T) if mask is None or mask[b, t]]
    if not live:
        return np.zeros(3, np.float32)
    return verts[b, :, 0:3, live[0]].astype(np.float64).mean(axis=0).astype(np.float32)


def project(verts, mask, b, t, cam, W, H, center):
    """Frame (b, t) of verts fp32 [B, V, 3 P, T] -> (pos fp32 [P, V, 3] centred, scr int64 [P, V, 2] snapped)."""
    verts = np.asarray(verts, dtype=np.float32)
    V, P = verts.shape[1], verts.shape[2] // 3
    c = centroid(verts, mask, b) if center else np.zeros(3, np.float32)
    pos = (verts[b, :, :, t].reshape(V, P, 3).transpose(1, 0, 2) - c[None, None, :]).astype(np.float32)
    sx, sy, tx, ty = (np.float32(v) for v in cam)
    one, hw, hh = np.float32(1), np.float32(0.5) * np.float32(W), np.float32(0.5) * np.float32(H)
    col = (one + sx * (pos[..., 0] + tx)) * hw
    row = (one + sy * (pos[..., 1] + ty)) * hh
    assert col.dtype == np.float32 and row.dtype == np.float32
    snap = lambda a: np.clip(np.rint(a * np.float32(SNAP)), -CLAMP, CLAMP).astype(np.int64)
    return pos, np.stack([snap(col), snap(row)], axis=-1)


def vertex_normals(pos, faces):
    """fp64 [P, V, 3]: per vertex the sum of (v1 - v0) x (v2 - v0) over its faces, divided by its length (0 stays 0)."""
    p = pos.astype(np.float64)
    out = np.zeros_like(p)
    for q in range(p.shape[0]):
        fn = np.cross(p[q, faces[:, 1]] - p[q, faces[:, 0]], p[q, faces[:, 2]] - p[q, faces[:, 0]])
        for k in range(3):
            np.add.at(out[q], faces[:, k], fn)
    ln = np.linalg.norm(out, axis=-1, keepdims=True)
    return np.divide(out, ln, out=np.zeros_like(out), where=ln > 0)


def _edge(a, b, px, py):
    return (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])


def _owns(a, b):
    return (b[1] - a[1] < 0) or (b[1] == a[1] and b[0] - a[0] > 0)


def render_frame(pos, scr, faces, W, H, colors=DEFAULT_COLORS, background=(1.0, 1.0, 1.0)):
    """One frame: dict(face int32 [H, W] (-1: background), depth fp64 (+inf), second fp64 (depth of the nearest different face, +inf),
    rgb uint8 [H, W, 3], count int32 (how many triangles cover the pixel))."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    P, F = pos.shape[0], len(faces)
    nrm = vertex_normals(pos, faces)
    p64 = pos.astype(np.float64)
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    win = np.full((H, W), -1, np.int64)
    count = np.zeros((H, W), np.int32)
    wn = np.zeros((H, W, 3))
    wp = np.zeros((H, W, 3))
    for q in range(P):
        for f in range(F):
            idx = [int(i) for i in faces[f]]
            a, b, c = ([int(v) for v in scr[q, i]] for i in idx)
            area = _edge(a, b, c[0], c[1])
            if area == 0:
                continue
            if area < 0:
                b, c, idx, area = c, b, [idx[0], idx[2], idx[1]], -area
            xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
            x0, x1 = max((min(xs) - 128 + 255) >> 8, 0), min(((max(xs) - 128) >> 8) + 1, W)
            y0, y1 = max((min(ys) - 128 + 255) >> 8, 0), min(((max(ys) - 128) >> 8) + 1, H)
            if x0 >= x1 or y0 >= y1:
                continue
            px = (np.arange(x0, x1, dtype=np.int64) * SNAP + SNAP // 2)[None, :]
            py = (np.arange(y0, y1, dtype=np.int64) * SNAP + SNAP // 2)[:, None]
            e0, e1, e2 = _edge(b, c, px, py), _edge(c, a, px, py), _edge(a, b, px, py)
            inside = ((e0 > 0) | ((e0 == 0) & _owns(b, c))) & ((e1 > 0) | ((e1 == 0) & _owns(c, a))) & ((e2 > 0) | ((e2 == 0) & _owns(a, b)))
            if not inside.any():
                continue
            b0, b1, b2 = e0 / float(area), e1 / float(area), e2 / float(area)
            z = b0 * p64[q, idx[0], 2] + b1 * p64[q, idx[1], 2] + b2 * p64[q, idx[2], 2]
            g = q * F + f
            sl = (slice(y0, y1), slice(x0, x1))
            ob, os_, ow = best[sl], second[sl], win[sl]
            better = inside & ((z < ob) | ((z == ob) & (g < ow)))
            worse = inside & ~better
            os_[better] = ob[better]
            os_[worse] = np.minimum(os_[worse], z[worse])
            ob[better] = z[better]
            ow[better] = g
            count[sl] += inside
            for k in range(3):
                wn[sl][..., k][better] = (b0 * nrm[q, idx[0], k] + b1 * nrm[q, idx[1], k] + b2 * nrm[q, idx[2], k])[better]
                wp[sl][..., k][better] = (b0 * p64[q, idx[0], k] + b1 * p64[q, idx[1], k] + b2 * p64[q, idx[2], k])[better]
    covered = win >= 0
    ln = np.linalg.norm(wn, axis=-1, keepdims=True)
    n = np.divide(wn, ln, out=np.zeros_like(wn), where=ln > 0)
    n = np.where(n[..., 2:3] > 0, -n, n)
    inten = np.full((H, W), 0.4)
    for L in LIGHTS:
        d = L[None, None, :] - wp
        dl = np.linalg.norm(d, axis=-1)
        inten += 0.2 * np.maximum(0.0, (n * d).sum(-1) / np.where(dl > 0, dl, 1.0))
    base = np.asarray([colors[min(q, len(colors) - 1)] for q in range(P)], dtype=np.float32).astype(np.float64)
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = np.clip(np.rint(255.0 * np.asarray(background, dtype=np.float32).astype(np.float64)), 0, 255).astype(np.uint8)
    person = np.where(covered, win // F, 0)
    shaded = np.clip(np.rint(255.0 * base[person] * inten[..., None]), 0, 255).astype(np.uint8)
    rgb[covered] = shaded[covered]
    return {"face": win.astype(np.int32), "depth": best, "second": second, "rgb": rgb, "count": count}


def depth_f32(pos, scr, tri, x, y):
    """The fp32 depth the contract assigns to pixel (x, y) under the triangle with vertex indices `tri` of one person (pos fp32 [V, 3], scr
    int64 [V, 2]), operation by operation: z = (fp32(e0) za + fp32(e1) zb + fp32(e2) zc) / fp32(area), each product and sum rounded to fp32, left
    to right. For tests that must tell an EXACT fp32 tie between two faces from a near one."""
    i = [int(v) for v in tri]
    a, b, c = ([int(v) for v in scr[k]] for k in i)
    area = _edge(a, b, c[0], c[1])
    assert area != 0
    if area < 0:
        b, c, i, area = c, b, [i[0], i[2], i[1]], -area
    px, py = x * SNAP + SNAP // 2, y * SNAP + SNAP // 2
    e = [np.float32(_edge(b, c, px, py)), np.float32(_edge(c, a, px, py)), np.float32(_edge(a, b, px, py))]
    z = [np.float32(pos[k, 2]) for k in i]
    return np.float32(np.float32(np.float32(e[0] * z[0]) + np.float32(e[1] * z[1])) + np.float32(e[2] * z[2])) / np.float32(area)


def near_tie(out, bound):
    """Covered pixels whose nearest and second-nearest depths (of different faces) lie within `bound`."""
    with np.errstate(invalid="ignore"):
        return (out["face"] >= 0) & (out["second"] - out["depth"] < bound)


def render(verts, faces, mask=None, width=64, height=64, cam=DEFAULT_CAM, colors=DEFAULT_COLORS, background=(1.0, 1.0, 1.0), center=True):
    """Every frame of verts fp32 [B, V, 3 P, T]: dict of arrays [B, T, H, W(, 3)] as render_frame names them. Masked frames are background."""
    verts = np.asarray(verts, dtype=np.float32)
    B, T = verts.shape[0], verts.shape[3]
    out = None
    for b in range(B):
        for t in range(T):
            if mask is not None and not mask[b, t]:
                pos = np.zeros((verts.shape[2] // 3, verts.shape[1], 3), np.float32)
                fr = render_frame(pos, np.zeros(pos.shape[:2] + (2,), np.int64), faces, width, height, colors, background)   # (all zero area)
            else:
                pos, scr = project(verts, mask, b, t, cam, width, height, center)
                fr = render_frame(pos, scr, faces, width, height, colors, background)
            if out is None:
                out = {k: np.empty((B, T) + v.shape, v.dtype) for k, v in fr.items()}
            for k, v in fr.items():
                out[k][b, t] = v
    return out
