"""Time the per-frame-shape calls (rgn_rot2xyz_shaped, rgn_rot2verts_shaped) beside what they replace, on the GPU:

    python tools/rot2xyz_shaped_bench.py [--out profiles/rot2xyz_shaped_bench.txt] [--rounds 5] [--reps 10]

Synthetic body of SMPL-X's size (synth.make_body(55, 10475)), rot6d, translation, no mask; B = 256, T = 60 and B = 128, T = 150, one and two
persons; joints and vertices. Three figures per row, measured in ONE process in ALTERNATING windows (a, b, c, a, b, c, ...; each window: `reps`
back-to-back calls from Python between one pair of device events, after a warm-up of every form), so that a drift of the box hits all three alike;
per figure the median over the rounds and the spread (min .. max) of the per-call time:
  (a) one shape    the existing one-shape call (Engine.rot2xyz / BodyEngine.rot2verts, betas[0] for every motion): the reference point. Its kernels'
                   instruction streams are the ones of the commit before this feature (k_fk<false>, k_lbs_chain<false>, k_lbs_skin<false>).
  (b) shaped       the new call with betas [B, nb] on the device, a shape per motion
  (c) loop         what a user had to do for per-motion shapes: B one-motion calls of (a), each with its own betas (one window = one loop)
and what the feature adds by count: nb of 9 (J - 1) + nb k-rows in the skinning loop (padded: nbp of nbp + Kp), 3 nb FMAs twice per joint in the
chain. The timed calls are checked against each other: (c) comes from the one-shape kernels, whose rest joints the host forms in fp64, and agrees
with (b) to fp32 rounding; motion 0 of (c) is motion 0 of (a) in every bit. Nothing here is a pass / fail check of speed."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import _lib, synth  # noqa: E402

SHAPES = [(256, 60, 1), (256, 60, 2), (128, 150, 1), (128, 150, 2)]
J, V, NB = 55, 10475, 10


def window(fn, reps):
    """ms per call of `reps` back-to-back calls of fn() between one pair of device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(forms, rounds):
    """forms: [(fn, reps)] -> per form (median, min, max) ms per call over `rounds` alternating windows."""
    for fn, _ in forms:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in forms]
    for _ in range(rounds):
        for i, (fn, reps) in enumerate(forms):
            ms[i].append(window(fn, reps))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--reps", default=10, type=int)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    from tests.helpers import build_hip
    cfg = synth.get_config("tiny")
    model, _ = build_hip(cfg, synth.make_state_dict(cfg, seed=0), resp="5")
    eng, _ = model._get_engine(2, cfg["num_frames"])
    dev = torch.device("cuda:0")
    body = synth.make_body(J, V)
    beng = _lib.BodyEngine(body["mesh"], J, 0)
    stream = torch.cuda.current_stream().cuda_stream
    flags = _lib.R2X_TRANSLATION | _lib.R2X_GLOB | _lib.R2X_VERTSTRANS
    rest64, sj64, parents = body["rest_joints"].astype(np.float64), body["shape_joints"].astype(np.float64), body["parents"]
    sj = torch.from_numpy(np.ascontiguousarray(body["shape_joints"], dtype=np.float32)).to(dev)
    Kp, nbp = (9 * (J - 1) + 7) // 8 * 8, (NB + 7) // 8 * 8
    fmt = lambda m: f"{m[0]:9.3f} ({m[1]:.3f} .. {m[2]:.3f})"            # noqa: E731
    lines = [f"rgn_rot2xyz_shaped / rgn_rot2verts_shaped on {torch.cuda.get_device_name(0)} (synthetic body: {J} joints, {V} vertices, {NB} betas; rot6d, "
             f"translation, no mask); ms per call from Python, {args.rounds} alternating windows of {args.reps} calls (loop: 1): median (min .. max)",
             f"k-rows of the skinning loop: {9 * (J - 1)} + {NB} ({Kp} + {nbp} padded: +{nbp / Kp:.1%}); chain: 2 x 3 x {NB} FMAs per joint and frame",
             f"{'kernel':>7s} {'B':>4s} {'T':>4s} {'P':>2s} | {'(a) one shape':>28s} | {'(b) shaped':>28s} {'b / a':>6s} | {'(c) loop of B':>30s} {'c / b':>7s}"]
    for B, T, P in SHAPES:
        rng = np.random.Generator(np.random.PCG64(B + T + P))
        x = torch.from_numpy(rng.standard_normal((B, J + 1, 6 * P, T)).astype(np.float32)).to(dev)
        betas = rng.standard_normal((B, NB)).astype(np.float32)
        bd = torch.from_numpy(betas).to(dev)
        rests = [rest64 + sj64 @ betas[b].astype(np.float64) for b in range(B)]          # what Rotation2xyz.rest_joints forms per call
        for kernel in ("joints", "verts"):
            rows = J if kernel == "joints" else V
            oa, ob, oc = (torch.empty((B, rows, 3 * P, T), device=dev) for _ in range(3))
            if kernel == "joints":
                a = lambda: eng.rot2xyz(x, None, rests[0], parents, 0, P, flags, None, oa, None, stream)                       # noqa: E731
                b = lambda: eng.rot2xyz_shaped(x, None, rest64, parents, sj, bd, (NB, 0, 0), 0, P, flags, None, ob, None, stream)      # noqa: E731

                def c():
                    for i in range(B):
                        eng.rot2xyz(x[i:i + 1], None, rests[i], parents, 0, P, flags, None, oc[i:i + 1], None, stream)
            else:
                wa = torch.empty(beng.workspace_bytes(B, T, P), dtype=torch.uint8, device=dev)
                wb = torch.empty(beng.workspace_bytes_shaped(B, T, P), dtype=torch.uint8, device=dev)
                a = lambda: beng.rot2verts(x, None, rests[0], parents, 0, P, flags, None, betas[0], oa, None, wa, stream)              # noqa: E731
                b = lambda: beng.rot2verts_shaped(x, None, rest64, parents, sj, bd, (NB, 0, 0), 0, P, flags, None, ob, None, wb, stream)       # noqa: E731

                def c():
                    for i in range(B):
                        beng.rot2verts(x[i:i + 1], None, rests[i], parents, 0, P, flags, None, betas[i], oc[i:i + 1], None, wa, stream)
            ta, tb, tc = alternate([(a, args.reps), (b, args.reps), (c, 1)], args.rounds)
            err = float((ob - oc).abs().max())
            assert err < 1e-4 and torch.equal(oa[:1], oc[:1]), err       # (the timed calls computed the same thing; parity is tests/test_rot2xyz_shaped_gpu.py)
            lines.append(f"{kernel:>7s} {B:4d} {T:4d} {P:2d} | {fmt(ta):>28s} | {fmt(tb):>28s} {tb[0] / ta[0]:6.3f} | {fmt(tc):>30s} {tc[0] / tb[0]:7.1f}"
                         f"   max|b - c| {err:.1e}")
            del oa, ob, oc
    beng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
