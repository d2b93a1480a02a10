"""Time rgn_rot2xyz (csrc/rgn_fk.hip) on the GPU:  python tools/rot2xyz_bench.py [--out profiles/rot2xyz_bench.txt]

Per shape, with device events around a run of back-to-back calls, warmed up, repeated until at least 0.2 s are timed:
  call     one Engine.rot2xyz call (55-joint synthetic skeleton, rot6d, translation, ragged mask): time and bytes moved / time, where the
           bytes are what the call must touch once: x [B, 56, 6 P, T] + mask [B, T] + xyz [B, 55, 3 P, T]
  alone    the kernel without the call's host side: the engine's own event pair around the launch (rgn_profile_query), mean of 256 calls, minus
           the same pair around an empty kernel (rgn_profile_bracket_overhead)
  copy     a device-to-device copy of the same byte count (read + write together), in the same process: the rate the memory system gives
  torch    the composition a user would otherwise write: tests/rot2xyz_ref.py in fp32 on the device (about 60 small matmuls and their glue)
Nothing here is a pass / fail check; the numbers go into profiles/rot2xyz_bench.txt by hand of whoever ran it on an MI355X."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import _lib, synth  # noqa: E402
from tests.rot2xyz_ref import rot2xyz_ref  # noqa: E402

SHAPES = [(256, 60, 1), (256, 60, 2), (128, 150, 2)]


def timed(fn, min_seconds=0.2, warmup=5):
    """ms per call of fn(), from device events around n back-to-back calls; n doubles until the timed run lasts min_seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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
            return ms / n, n
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
    J = 55
    stream = torch.cuda.current_stream().cuda_stream
    flags = _lib.R2X_TRANSLATION | _lib.R2X_GLOB | _lib.R2X_VERTSTRANS
    lines = [f"rgn_rot2xyz on {torch.cuda.get_device_name(0)} (55-joint synthetic skeleton, rot6d, translation, ragged mask); device events, >= 0.2 s per figure",
             f"{'B':>4s} {'T':>4s} {'P':>2s} {'MB moved':>9s} | {'call us':>10s} {'GB/s':>8s} | {'alone us':>9s} {'GB/s':>8s} | {'copy us':>9s} {'GB/s':>8s} | {'torch fp32 us':>13s} {'x call':>9s}"]
    for B, T, P in SHAPES:
        rng = np.random.Generator(np.random.PCG64(B + T + P))
        x = torch.from_numpy(rng.standard_normal((B, J + 1, 6 * P, T)).astype(np.float32)).to(dev)
        mask = torch.from_numpy(rng.uniform(size=(B, T)) < 0.8).to(dev)
        out = torch.empty((B, J, 3 * P, T), device=dev)
        nbytes = x.numel() * 4 + mask.numel() + out.numel() * 4
        k_ms, _ = timed(lambda: eng.rot2xyz(x, mask, sk["rest_joints"], sk["parents"], 0, P, flags, None, out, None, stream))
        eng.profile_enable(True)
        for _ in range(256):
            eng.rot2xyz(x, mask, sk["rest_joints"], sk["parents"], 0, P, flags, None, out, None, stream)
        (a_total, a_n), = [v for v in eng.profile_query().values() if v[1] > 0]
        a_ms = a_total / a_n - eng.profile_bracket_overhead_ms()
        eng.profile_enable(False)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)          # a copy reads and writes: nbytes / 2 each way
        dst = torch.empty_like(src)
        c_ms, _ = timed(lambda: dst.copy_(src))
        t_ms, _ = timed(lambda: rot2xyz_ref(x, mask, sk, "rot6d", True, True, True, num_person=P, dtype=torch.float32))
        ref = rot2xyz_ref(x, mask, sk, "rot6d", True, True, True, num_person=P, dtype=torch.float32)
        assert float((out - ref).abs().max()) < 1e-4                           # (the timed call computed the right thing; parity is tests/test_rot2xyz_gpu.py)
        lines.append(f"{B:4d} {T:4d} {P:2d} {nbytes / 1e6:9.2f} | {k_ms * 1e3:10.1f} {nbytes / k_ms / 1e6:8.1f} | {a_ms * 1e3:9.1f} {nbytes / a_ms / 1e6:8.1f} | {c_ms * 1e3:9.1f} {nbytes / c_ms / 1e6:8.1f} | "
                     f"{t_ms * 1e3:13.1f} {t_ms / k_ms:9.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
