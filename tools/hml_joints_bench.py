"""Time rgn_hml_to_joints (csrc/rgn_hml.hip) against the torch composition it replaces:  python tools/hml_joints_bench.py [--out profiles/hml_joints_bench.txt]

Per shape, on the same GPU in the same process, the two sides alternating, each figure the median of 7 windows of at least 0.1 s of back-to-back
calls between device events, warmed up:
  fused     one Engine.hml_to_joints call: x [B, 263, 1, T] + mean + std -> xyz [B, 22, 3, T]
  composed  the same lines as torch expressions in fp32 on device tensors, as a user would otherwise write them: the permute and data * std + mean,
            the shifted cumsum of the rotation velocities, cos / sin, two cross products per rotation for the root velocities and for the local
            positions, the cumsum of the turned velocities, the x / z offsets, the concatenation and the closing permute (about fifteen launches and
            several [B, T, J, 3] temporaries)
Bytes: what the fused call must touch once (rows 0 .. 3 (J-1) + 3 of x, and xyz) over its time is its achieved bandwidth. Nothing here is a pass /
fail check beyond the two sides agreeing; parity is tests/test_hml_gpu.py."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd.sample.render import postprocessing_engine  # noqa: E402
from tests import hml_ref  # noqa: E402

SHAPES = [(256, 196), (1, 196)]
J = 22


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


def turn(c, s, v):
    """qrot(qinv(q), v) for q = (c, 0, s, 0): qvec = (0, -s, 0), uv = qvec x v, uuv = qvec x uv, v + 2 (c uv + uuv)."""
    qvec = torch.stack((torch.zeros_like(s), -s, torch.zeros_like(s)), -1).expand(v.shape)
    uv = torch.cross(qvec, v, dim=-1)
    uuv = torch.cross(qvec, uv, dim=-1)
    return v + 2 * (c.unsqueeze(-1) * uv + uuv)


def composed(x, mean, std):
    data = x.permute(0, 2, 3, 1) * std + mean                       # [B, 1, T, D]
    ang = torch.zeros_like(data[..., 0])
    ang[..., 1:] = data[..., :-1, 0]
    ang = torch.cumsum(ang, dim=-1)
    c, s = torch.cos(ang), torch.sin(ang)
    vel = torch.zeros(data.shape[:-1] + (3,), device=data.device)
    vel[..., 1:, 0] = data[..., :-1, 1]
    vel[..., 1:, 2] = data[..., :-1, 2]
    r_pos = torch.cumsum(turn(c, s, vel), dim=-2)
    r_pos[..., 1] = data[..., 3]
    pos = data[..., 4:4 + 3 * (J - 1)]
    pos = turn(c.unsqueeze(-1), s.unsqueeze(-1), pos.reshape(pos.shape[:-1] + (J - 1, 3)))
    pos[..., 0] += r_pos[..., 0:1]
    pos[..., 2] += r_pos[..., 2:3]
    pos = torch.cat((r_pos.unsqueeze(-2), pos), dim=-2)              # [B, 1, T, J, 3]
    return pos.reshape((-1,) + pos.shape[2:]).permute(0, 2, 3, 1).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    dev = torch.device("cuda", 0)
    _, eng = postprocessing_engine(dev)
    stream = torch.cuda.current_stream().cuda_stream
    D = hml_ref.rows_of(J)
    lines = [f"rgn_hml_to_joints on {torch.cuda.get_device_name(0)} against the torch composition of the same lines (fp32, on the device); "
             "device events, the two sides alternating, median of 7 windows >= 0.1 s (min .. max)",
             f"{'B':>4s} {'T':>4s} {'MB':>7s} | {'fused us':>22s} {'GB/s':>7s} | {'composed us':>26s} | {'composed / fused':>16s}"]
    for B, T in SHAPES:
        x, mean, std = (torch.from_numpy(a).to(dev) for a in hml_ref.make_inputs(B, D, T, seed=B + T))
        xyz = torch.empty((B, J, 3, T), device=dev)
        nbytes = (B * (3 * (J - 1) + 4) * T + xyz.numel()) * 4

        def fused():
            eng.hml_to_joints(x, mean, std, J, xyz, stream)

        for _ in range(5):
            fused()
            ref = composed(x, mean, std)
        torch.cuda.synchronize()
        gap = (xyz - ref).abs().max().item()
        assert gap < 1e-4, gap                  # (both sides computed the same thing)
        f_ms, c_ms = [], []
        for _ in range(7):
            f_ms.append(window(fused))
            c_ms.append(window(lambda: composed(x, mean, std)))
        fm, cm = statistics.median(f_ms), statistics.median(c_ms)
        lines.append(f"{B:4d} {T:4d} {nbytes / 1e6:7.2f} | {fm * 1e3:8.1f} ({min(f_ms) * 1e3:5.1f} .. {max(f_ms) * 1e3:5.1f}) {nbytes / fm / 1e6:7.1f} | "
                     f"{cm * 1e3:9.1f} ({min(c_ms) * 1e3:6.1f} .. {max(c_ms) * 1e3:6.1f}) | {cm / fm:16.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
