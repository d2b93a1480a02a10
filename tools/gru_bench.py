"""Time the GRU action classifier (rgn_gru_forward, one launch) against the torch composition it replaces, on the same GPU in the same process.

    python tools/gru_bench.py [--N 64 256 1024] [--T 60] [--repeats 30] [--out profiles/gru_eval_bench.txt]

The torch composition is the reference's module restated here: nn.GRU(72, 128, 2) + Linear(128, 30) + tanh + Linear(30, 12) with the permute to
[T, N, I] and the gather of each sequence's last valid frame. Both get the same weights, inputs, lengths and hidden state, and their outputs are
compared before anything is timed. Per N: 5 warm-up calls of each, then `repeats` rounds that ALTERNATE the two; each call is bracketed by device
events and at least 20 calls are batched per bracket so that a bracket spans milliseconds. Reported: the median and the min .. max of the per-call
times, and the ratio of the medians."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TorchComposition(torch.nn.Module):
    def __init__(self, I, H, L, C):
        super().__init__()
        self.recurrent = torch.nn.GRU(I, H, L)
        self.linear1 = torch.nn.Linear(H, 30)
        self.linear2 = torch.nn.Linear(30, C)

    def forward(self, x, lengths, h0):
        bs, nj, nf, T = x.shape
        seq = x.reshape(bs, nj * nf, T).permute(2, 0, 1)
        out, _ = self.recurrent(seq.float(), h0)
        out = out[lengths - 1, torch.arange(bs, device=x.device)]
        feats = torch.tanh(self.linear1(out))
        return feats, self.linear2(feats)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--N", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--T", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20, help="calls per event bracket")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_bench needs an AMD GPU (no CPU fallback)")
    from regennet_amd import synth
    from regennet_amd.eval import gru
    dev = "cuda:0"
    I, H, L, C = 72, 128, 2, 12
    sd = {k: torch.from_numpy(v) for k, v in synth.make_gru_state_dict(I, H, L, 30, C, seed=0).items()}
    ours = gru.MotionDiscriminator(I, H, L, device=dev, output_size=C)
    ours.load_state_dict(sd)
    ours = ours.to(dev).eval()
    ref = TorchComposition(I, H, L, C)
    ref.load_state_dict(sd)
    ref = ref.to(dev).eval()
    lines = [f"# tools/gru_bench.py on {torch.cuda.get_device_name(0)}: rgn_gru_forward (one launch) vs nn.GRU + 2 nn.Linear in torch {torch.__version__}",
             f"# geometry {I}/{H}/{L}/{C}, T = {args.T}, lengths uniform in [T/2, T]; per-call ms from device events over {args.calls} calls per bracket,",
             f"# median (min .. max) of {args.repeats} alternating rounds after 5 warm-up calls; ratio = torch / hip (> 1: the kernel is faster)",
             "#    N      hip ms (min .. max)          torch ms (min .. max)        ratio   max|hip - torch| features / logits"]
    with torch.no_grad():
        for N in args.N:
            x, ln, h0 = synth.make_gru_inputs(N, I, args.T, hidden=H, layers=L, seed=N)
            ln = np.random.Generator(np.random.PCG64(N)).integers(args.T // 2, args.T + 1, N)
            x, ln, h0 = torch.from_numpy(x).to(dev), torch.from_numpy(ln).to(dev), torch.from_numpy(h0).to(dev)
            f_h, l_h = ours.forward_both(x, ln, h0)
            f_t, l_t = ref(x, ln, h0)
            df, dl = (f_h - f_t).abs().max().item(), (l_h - l_t).abs().max().item()
            run_h, run_t = (lambda: ours.forward_both(x, ln, h0)), (lambda: ref(x, ln, h0))
            for _ in range(5):
                run_h()
                run_t()
            torch.cuda.synchronize()
            th, tt = [], []
            for _ in range(args.repeats):
                th.append(timed(run_h, args.calls))
                tt.append(timed(run_t, args.calls))
            mh, mt = float(np.median(th)), float(np.median(tt))
            lines.append(f"{N:6d}   {mh:8.4f} ({min(th):.4f} .. {max(th):.4f})   {mt:8.4f} ({min(tt):.4f} .. {max(tt):.4f})   {mt / mh:6.2f}   {df:.2e} / {dl:.2e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
