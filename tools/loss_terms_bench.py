"""Time rgn_loss_terms (csrc/rgn_loss.hip) against the composition it replaces:  python tools/loss_terms_bench.py [--out profiles/loss_terms_bench.txt]

Per shape, on the same GPU in the same process, the two sides alternating, each figure the median of 7 windows of at least 0.1 s of back-to-back
calls between device events, warmed up:
  fused     one Engine.loss_terms call: target, output, cmotion [B, 56, 6, T] + mask -> [B, 7] (55-joint synthetic skeleton, ragged mask)
  composed  what a user would otherwise write on device tensors: three Engine.rot2xyz calls (mask=None, vertstrans=False: get_xyz of
            gaussian_diffusion.py:1254-1258) and the torch expressions of tests/losses_ref.py in fp32 on their outputs
Bytes: what the fused call must touch once (the three inputs, the mask, the terms) over its time is its achieved bandwidth; the composition
also writes and re-reads three [B, 55, 3, T] joint tensors. Nothing here is a pass / fail check."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import _lib, synth  # noqa: E402
from tests import loss_cases  # noqa: E402
from tests.losses_ref import FOOT_JOINTS, TERMS, loss_terms_ref  # noqa: E402

SHAPES = [(256, 60), (128, 150)]


def window(fn, min_seconds=0.1):
    """ms per call of fn() from device events around n back-to-back calls; n doubles until the window lasts min_seconds."""
    n = 8
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_seconds * 1e3:
            return ms / n
        n *= 2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    cfg = synth.get_config("tiny")
    model, _ = synth.build_model(cfg, synth.make_state_dict(cfg, seed=0), precision="f32")
    eng, dev = model._get_engine(1, cfg["num_frames"])
    sk = synth.make_skeleton(55)
    J, thr = 55, 0.03
    stream = torch.cuda.current_stream().cuda_stream
    flags = _lib.R2X_TRANSLATION | _lib.R2X_GLOB
    lines = [f"rgn_loss_terms on {torch.cuda.get_device_name(0)} against 3 x rgn_rot2xyz + the torch expressions of the seven terms (fp32, on the device); "
             "device events, the two sides alternating, median of 7 windows >= 0.1 s (min .. max)",
             f"{'B':>4s} {'T':>4s} {'MB in':>7s} | {'fused us':>22s} {'GB/s':>7s} | {'composed us':>24s} | {'composed / fused':>16s}"]
    for B, T in SHAPES:
        inp = loss_cases.make_motions(B, T, J, 0.01, B + T)
        t, o, c = (torch.from_numpy(inp[k]).to(dev) for k in ("target", "output", "cmotion"))
        mask = torch.from_numpy(loss_cases.make_mask("ragged", B, T, B)).to(dev)
        terms = torch.empty((B, 7), device=dev)
        xyz = [torch.empty((B, J, 3, T), device=dev) for _ in range(3)]
        nbytes = 3 * t.numel() * 4 + mask.numel() + terms.numel() * 4

        def fused():
            eng.loss_terms(t, o, c, mask, sk["rest_joints"], sk["parents"], FOOT_JOINTS, 55, thr, _lib.LOSS_FC, terms, stream)

        def composed():
            for x, out in zip((t, o, c), xyz):
                eng.rot2xyz(x, None, sk["rest_joints"], sk["parents"], 0, 1, flags, None, out, None, stream)
            d = loss_terms_ref(t, o, c, mask, sk, thr, dtype=torch.float32, xyz=xyz)
            return torch.stack([d[k] for k in TERMS], 1)

        for _ in range(5):
            fused()
            ref = composed()
        torch.cuda.synchronize()
        rel = ((terms - ref).abs() / ref.abs()).max().item()
        assert rel < 1e-3, rel                  # (both sides computed the same thing; parity is tests/test_losses_gpu.py)
        f_ms, c_ms = [], []
        for _ in range(7):
            f_ms.append(window(fused))
            c_ms.append(window(composed))
        fm, cm = statistics.median(f_ms), statistics.median(c_ms)
        lines.append(f"{B:4d} {T:4d} {nbytes / 1e6:7.2f} | {fm * 1e3:8.1f} ({min(f_ms) * 1e3:5.1f} .. {max(f_ms) * 1e3:5.1f}) {nbytes / fm / 1e6:7.1f} | "
                     f"{cm * 1e3:9.1f} ({min(c_ms) * 1e3:5.1f} .. {max(c_ms) * 1e3:5.1f}) | {cm / fm:16.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
