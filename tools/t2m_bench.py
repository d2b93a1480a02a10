"""Times the text-to-motion evaluator's device encoders (regennet_amd.eval.t2m over rgn_t2m.hip) against the torch composition of the same modules
(nn.Conv1d / nn.Linear / nn.GRU on packed sequences / nn.LayerNorm) on the same GPU, at the real geometry (263 / 512 / 512 / 1024 / 300 / 15 / 512 / 512).

    python tools/t2m_bench.py --out profiles/t2m_eval_bench.txt

Each batch size is timed in a child process of its own under `timeout`, so a hang ends that size alone. Per-call milliseconds come from device events
around `--calls` calls, the median (min .. max) of `--repeats` alternating rounds after warm-up. The recurrent kernel is built with a 16-sequence tile
only; no 32-sequence tile exists to report."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TorchEvaluator(nn.Module):
    """modules.py:79-98, :311-386 composed as evaluator_wrapper.py:154-172 composes them"""

    def __init__(self, sds, dev):
        super().__init__()
        from regennet_amd.eval import t2m

        class _Plain(nn.Module):
            pass
        self.mov = t2m.MovementConvEncoder(259, 512, 512)
        self.text = t2m.TextEncoderBiGRUCo(300, 15, 512, 512, dev)
        self.motion = t2m.MotionEncoderBiGRUCo(512, 1024, 512, dev)
        for m, k in ((self.mov, "movement_encoder"), (self.text, "text_encoder"), (self.motion, "motion_encoder")):
            m.load_state_dict({kk: torch.from_numpy(v) for kk, v in sds[k].items()})
        self.to(dev).eval()

    @staticmethod
    def _bigru(m, emb, lens):
        order = torch.argsort(lens, descending=True)
        packed = pack_padded_sequence(emb[order], lens[order].cpu(), batch_first=True)
        _, last = m.gru(packed, m.hidden.repeat(1, emb.shape[0], 1))
        out = m.output_net(torch.cat([last[0], last[1]], dim=-1))
        return out[torch.argsort(order)]

    def forward(self, d):
        x = d["motions"][..., :-4].permute(0, 2, 1)
        mov = self.mov.out_net(self.mov.main(x).permute(0, 2, 1))
        motion = self._bigru(self.motion, self.motion.input_emb(mov), d["m_lens"] // 4)
        text = self._bigru(self.text, self.text.input_emb(d["word_embs"] + self.text.pos_emb(d["pos_ohot"])), d["cap_lens"])
        return text, motion


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def one(N, T, Lw, repeats, calls):
    from regennet_amd import synth
    from regennet_amd.eval import t2m
    dev = "cuda:0"
    sds = synth.make_t2m_state_dicts(seed=0)
    ours = t2m.EvaluatorMDMWrapper("humanml", dev, state_dicts=sds)
    ref = TorchEvaluator(sds, dev)
    inp = synth.make_t2m_inputs(N, T, Lw, seed=N)
    d = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    with torch.no_grad():
        run_h = lambda: ours.get_co_embeddings(d["word_embs"], d["pos_ohot"], d["cap_lens"], d["motions"], d["m_lens"], keep_order=True)
        run_m = lambda: ours.get_motion_embeddings(d["motions"], d["m_lens"], keep_order=True)
        run_t = lambda: ref(d)
        th_, mh_ = run_h()
        tt_, mt_ = run_t()
        dt, dm = (th_ - tt_).abs().max().item(), (mh_ - mt_).abs().max().item()
        for _ in range(3):
            run_h(), run_m(), run_t()
        torch.cuda.synchronize()
        th, tm, tt = [], [], []
        for _ in range(repeats):
            th.append(timed(run_h, calls))
            tm.append(timed(run_m, calls))
            tt.append(timed(run_t, calls))
    f = lambda v: f"{float(np.median(v)):9.3f} ({min(v):.3f} .. {max(v):.3f})"
    print(f"{N:6d}   {f(th)}   {f(tm)}   {f(tt)}   {np.median(tt) / np.median(th):6.2f}   {dt:.2e} / {dm:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--N", type=int, nargs="+", default=[32, 1024])
    ap.add_argument("--T", type=int, default=196)
    ap.add_argument("--Lw", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3, help="calls per event bracket")
    ap.add_argument("--limit", type=int, default=240, help="seconds per batch size")
    ap.add_argument("--one", type=int, help="(internal) time this batch size in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("t2m_bench needs an AMD GPU (no CPU fallback)")
    if args.one:
        return one(args.one, args.T, args.Lw, args.repeats, args.calls)
    lines = [f"# tools/t2m_bench.py on {torch.cuda.get_device_name(0)}: EvaluatorMDMWrapper.get_co_embeddings on rgn_t2m.hip (k_rows x 12, k_bigru<1024>, k_bigru<512>,",
             f"# k_ln_lrelu x 2; 16-sequence tile) vs the torch {torch.__version__} composition of the same modules (nn.GRU on packed sequences), same GPU.",
             f"# real geometry, T = {args.T}, Lw = {args.Lw}, mixed lengths; per-call ms from device events over {args.calls} calls per bracket, median (min .. max) of",
             f"# {args.repeats} alternating rounds after 3 warm-up calls; ratio = torch / hip co-embeddings (> 1: the kernels are faster)",
             "#    N   hip text + motion ms          hip motion only ms            torch text + motion ms        ratio   max|hip - torch| text / motion"]
    for N in args.N:
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(N), "--T", str(args.T), "--Lw", str(args.Lw),
                            "--repeats", str(args.repeats), "--calls", str(args.calls)], capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"{N:6d}   ended with status {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ''}")
            print(lines[-1], flush=True)
            break                                            # nothing more is started on the GPU behind a failed step
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
