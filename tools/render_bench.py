"""Time rgn_render (csrc/rgn_render.hip) on the GPU:  python tools/render_bench.py [--out profiles/render_bench.txt]

Two persons, 60 frames, 1 and 64 motions, 256 x 256 and 1024 x 1024, default camera, centring on, through utils.render.MeshRenderer (one launch
sequence per motion), for two meshes of SMPL-X's size:
  strip    synth.make_body(55, 10475) in its rest pose: its faces are a triangle strip over a RANDOM vertex order, so nearly every triangle spans
           a limb or the whole body and a pixel lies under hundreds of them. It is the body the other tools use, and a rasteriser's worst case.
  surface  a closed ellipsoid of 100 x 105 = 10500 vertices and 20800 faces (SMPL-X: 10475 / 20908) with a person's proportions: triangles of a
           few pixels and a depth complexity of 2, as a body model's mesh has them.
Per configuration, after a warm-up, every repetition between its own pair of device events: median (min .. max), frames/s from the median, and
beside it the time a plain device fill of as many bytes as the RGB output (3 W H per frame) takes in the same process - what merely storing the
frames costs. Repetitions: as many as fit about two seconds, between 3 and 20.

Per-kernel times come from a run of their own under the profiler (tracing slows the host):
  rocprofv3 --kernel-trace -d DIR -o trace --output-format csv -- python tools/render_bench.py --trace
  python tools/render_bench.py --summarise DIR/.../trace_kernel_trace.csv
--trace runs the four one-motion configurations, 2 + 5 calls each; --summarise averages the last 5 of each, per kernel.
Nothing here is a pass / fail check. profiles/render_bench.txt holds both outputs."""
import argparse
import csv
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import synth  # noqa: E402
from regennet_amd.utils.render import MeshRenderer  # noqa: E402

T, P = 60, 2
KERNELS = ["k_rnd_centroid", "k_rnd_project", "k_rnd_normals", "k_rnd_bbox", "k_rnd_raster"]
TRACE_WARM, TRACE_CALLS = 2, 5


def strip_mesh():
    m = synth.make_body(55, 10475)["mesh"]
    return m["v_template"].astype(np.float32), m["faces"]


def surface_mesh(nu=100, nv=105):
    u, v = np.arange(nu) * (2 * np.pi / nu), (np.arange(nv) + 0.5) * (np.pi / nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")                                       # [nu, nv]
    pts = np.stack([0.25 * np.cos(uu) * np.sin(vv), 0.85 * np.cos(vv), 0.15 * np.sin(uu) * np.sin(vv)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv - 1), indexing="ij")
    a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + j + 1, i * nv + j + 1
    return pts.astype(np.float32), np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int32)


def motion(points, B, dev):
    """[B, V, 6, T]: person 1 is person 0 shifted by (0.35, 0, 0.1); frame t walks 2 mm further in x, motion b 1 mm in y."""
    base = torch.from_numpy(np.concatenate([points, points + np.float32([0.35, 0.0, 0.1])], axis=1)).to(dev)            # [V, 6]
    out = base[None, :, :, None].repeat(B, 1, 1, T)
    out[:, :, 0::3, :] += 0.002 * torch.arange(T, device=dev)
    out[:, :, 1::3, :] += 0.001 * torch.arange(B, device=dev)[:, None, None, None]
    return out.contiguous()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn):
    first = event_ms(fn)                                                               # (warm-up: code objects, the workspace, the output's pages)
    second = event_ms(fn)
    reps = int(min(20, max(3, 2000.0 / max(second, 1e-3))))
    ms = [event_ms(fn) for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms), reps, first


def summarise(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if name:
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    per = len(KERNELS) * (TRACE_WARM + TRACE_CALLS)
    configs = [(m, s) for m in ("strip", "surface") for s in (256, 1024)]
    assert len(rows) == per * len(configs), (len(rows), per, len(configs))
    lines = [f"per-kernel ms for ONE motion (2 persons x 60 frames), mean of {TRACE_CALLS} calls under rocprofv3 --kernel-trace:",
             f"{'mesh':>8s} {'size':>5s} | " + " ".join(f"{k[6:]:>9s}" for k in KERNELS) + f" | {'sum':>8s}"]
    for ci, (m, s) in enumerate(configs):
        chunk = rows[ci * per + len(KERNELS) * TRACE_WARM:(ci + 1) * per]
        mean = {k: np.mean([ms for _, n, ms in chunk if n == k]) for k in KERNELS}
        lines.append(f"{m:>8s} {s:5d} | " + " ".join(f"{mean[k]:9.3f}" for k in KERNELS) + f" | {sum(mean.values()):8.3f}")
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", default="")
    args = ap.parse_args(argv)
    if args.summarise:
        text = summarise(args.summarise)
    else:
        assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
        dev = torch.device("cuda:0")
        meshes = {"strip": strip_mesh(), "surface": surface_mesh()}
        lines = [f"rgn_render on {torch.cuda.get_device_name(0)}: 2 persons x 60 frames a motion, MeshRenderer.render (one launch sequence per motion); every "
                 "repetition between its own device events: median (min .. max)",
                 f"{'mesh':>8s} {'V':>6s} {'F':>6s} {'B':>3s} {'size':>5s} | {'ms':>34s} {'reps':>4s} | {'frames/s':>9s} | {'rgb GB':>7s} {'fill ms':>8s} {'x fill':>7s}"]
        for name, (pts, faces) in meshes.items():
            r = MeshRenderer(faces, dev)
            one = {}
            for B in ((1,) if args.trace else (1, 64)):
                verts = motion(pts, B, dev)
                for size in (256, 1024):
                    if B > 1 and one[size] * B * 5 > 60e3:
                        lines.append(f"{name:>8s} {len(pts):6d} {len(faces):6d} {B:3d} {size:5d} | not measured: {B} x the one-motion time x 5 calls is more than a minute")
                        continue
                    fn = lambda: r.render(verts, width=size, height=size)                  # noqa: E731
                    if args.trace:
                        for _ in range(TRACE_WARM + TRACE_CALLS):
                            fn()
                        torch.cuda.synchronize()
                        continue
                    med, lo, hi, reps, _ = timed(fn)
                    one.setdefault(size, med)
                    nbytes = B * T * size * size * 3
                    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                    fill = timed(lambda: buf.fill_(255))[0]
                    del buf
                    lines.append(f"{name:>8s} {len(pts):6d} {len(faces):6d} {B:3d} {size:5d} | {med:12.3f} ({lo:.3f} .. {hi:.3f}) {reps:4d} | {B * T / med * 1e3:9.0f} | "
                                 f"{nbytes / 1e9:7.3f} {fill:8.3f} {med / fill:7.1f}")
                del verts
            r.close()
        text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
