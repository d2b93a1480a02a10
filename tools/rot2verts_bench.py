"""Time rgn_rot2verts (csrc/rgn_lbs.hip) on the GPU:  python tools/rot2verts_bench.py [--out profiles/rot2verts_bench.txt] [--reps 20]

Synthetic body of SMPL-X's size (synth.make_body(55, 10475)), rot6d, translation, no mask, at B = 256, T = 60 and at B = 1, T = 60. Per shape,
after a warm-up, every repetition between its own pair of device events; the median and the spread (min .. max) are reported.
  kernel   one BodyEngine.rot2verts call (its three launches)
  torch    the composition a user would otherwise write (`composition` below): the same six steps in fp32 on the device with resident constants,
           one matmul per sum, no mask handling, written straight into a preallocated [B, V, 3, T]; in pieces of 64 motions so that its
           [frames, 12, V] intermediate (1.9 GB a piece) fits
  output   bytes of [B, V, 3, T] fp32 / kernel time, beside the rate a device-to-device copy of as many bytes reaches in the same process
  MFMA     2 x (9 (J - 1) x 3 V + 12 x J x V) multiply-adds per frame / kernel time (the guide's untuned fp32-MFMA GEMM: 122 TFLOP/s)
Nothing here is a pass / fail check. profiles/rot2verts_bench.txt holds this output and tools/kernel_resources.sh rgn_lbs.hip."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from regennet_amd import _lib, synth  # noqa: E402
from tests.rot2xyz_ref import rotation_6d_to_matrix  # noqa: E402

SHAPES = [(256, 60), (1, 60)]
J, V = 55, 10475


class Composition:
    """Linear blend skinning from torch operations, fp32, constants resident on the device."""

    def __init__(self, body, dev):
        m = body["mesh"]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)      # noqa: E731
        self.parents = [int(p) for p in body["parents"]]
        self.rest = t(body["rest_joints"])
        self.rel = self.rest.clone()
        self.rel[1:] -= self.rest[self.parents[1:]]
        self.vt, self.posedirs, self.wt = t(m["v_template"]).reshape(1, -1), t(m["posedirs"]), t(m["lbs_weights"]).t().contiguous()
        self.idj = [int(j) for j in m["identity_joints"]]
        self.eye = torch.eye(3, device=dev)

    def __call__(self, x, out):
        """x [B, J + 1, 6, T] -> out [B, V, 3, T] (one person, translation relative to frame 0)."""
        B, _, _, T = x.shape
        J, V, N = len(self.parents), self.wt.shape[1], B * T
        rot = rotation_6d_to_matrix(x[:, :J].permute(0, 3, 1, 2).reshape(N, J, 6))
        rot[:, self.idj] = self.eye
        v_posed = torch.addmm(self.vt, (rot[:, 1:] - self.eye).reshape(N, -1), self.posedirs).view(N, V, 3)
        grot, gpos = [rot[:, 0]], [self.rest[0].expand(N, 3)]
        for i in range(1, J):
            p = self.parents[i]
            gpos.append(gpos[p] + grot[p] @ self.rel[i])
            grot.append(grot[p] @ rot[:, i])
        R, t = torch.stack(grot, 1), torch.stack(gpos, 1)                          # [N, J, 3, 3], [N, J, 3]
        A = torch.cat([R, (t - (R @ self.rest[:, :, None]).squeeze(-1))[..., None]], dim=3)       # [N, J, 3, 4]
        Tm = (A.reshape(N, J, 12).transpose(1, 2) @ self.wt).view(N, 3, 4, V)      # [N, 3, 4, V]
        vp = v_posed.transpose(1, 2)                                               # [N, 3, V]
        verts = (Tm[:, :, :3] * vp[:, None]).sum(2) + Tm[:, :, 3]                  # [N, 3, V]
        tr = x[:, J, :3] - x[:, J, :3, :1]                                         # [B, 3, T]
        torch.add(verts.view(B, T, 3, V).permute(0, 3, 2, 1), tr[:, None], out=out)
        return out


def event_times(fn, reps, warmup=3):
    """ms of each of `reps` calls of fn(), each between its own pair of device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return np.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", default=20, type=int)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU: numbers that were not measured on one are reported as 'not measured'"
    reps = max(20, args.reps)
    dev = torch.device("cuda:0")
    body = synth.make_body(J, V)
    eng = _lib.BodyEngine(body["mesh"], J, 0)
    comp = Composition(body, dev)
    stream = torch.cuda.current_stream().cuda_stream
    flags = _lib.R2X_TRANSLATION | _lib.R2X_GLOB | _lib.R2X_VERTSTRANS
    lines = [f"rgn_rot2verts on {torch.cuda.get_device_name(0)} (synthetic body: {J} joints, {V} vertices; rot6d, translation, no mask); "
             f"{reps} repetitions, each between its own device events: median (min .. max)",
             f"{'B':>4s} {'T':>4s} | {'kernel ms':>30s} | {'torch fp32 ms':>30s} {'x kernel':>9s} | {'out GB':>7s} {'GB/s':>7s} {'copy GB/s':>9s} | {'TFLOP/s':>8s} {'of 122':>7s}"]
    for B, T in SHAPES:
        rng = np.random.Generator(np.random.PCG64(B + T))
        x = torch.from_numpy(rng.standard_normal((B, J + 1, 6, T)).astype(np.float32)).to(dev)
        out = torch.empty((B, V, 3, T), device=dev)
        work = torch.empty(eng.workspace_bytes(B, T, 1), dtype=torch.uint8, device=dev)
        k = event_times(lambda: eng.rot2verts(x, None, body["rest_joints"], body["parents"], 0, 1, flags, None, None, out, None, work, stream), reps)
        chunk = 64                                 # motions per piece (the one-person translation is relative to each motion's own frame 0)
        ref = torch.empty_like(out)

        def composition():
            for i in range(0, B, chunk):
                comp(x[i:i + chunk], ref[i:i + chunk])

        t = event_times(composition, reps)
        err = float((out - ref).abs().max())
        assert err < 1e-4, err                     # (the timed call computed the right thing; parity is tests/test_rot2verts_gpu.py)
        del ref
        nbytes = out.numel() * 4
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)          # a copy reads and writes: nbytes / 2 each way
        dst = torch.empty_like(src)
        c = event_times(lambda: dst.copy_(src), reps)
        del src, dst
        flop = 2.0 * (9 * (J - 1) * 3 * V + 12 * J * V) * B * T
        fmt = lambda m: f"{m[0]:10.3f} ({m[1]:.3f} .. {m[2]:.3f})"            # noqa: E731
        lines.append(f"{B:4d} {T:4d} | {fmt(k):>30s} | {fmt(t):>30s} {t[0] / k[0]:9.2f} | {nbytes / 1e9:7.3f} {nbytes / k[0] / 1e6:7.0f} {nbytes / c[0] / 1e6:9.0f} | "
                     f"{flop / k[0] / 1e9:8.2f} {flop / k[0] / 1e9 / 122:7.1%}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
