"""arch='gru' on one box: the HIP layer-wavefront GRU stack against fp32 torch.nn.GRU on the same GPU and in the same process, for both scans.

    python tools/gru_arch_bench.py --config ntu_gru --batch 256 --respacing 10 --calls 3

Prints one JSON line per scan ('batch': the reference's recurrence over the B samples of a call, T sequences; 'frames': T steps, B sequences):
  hip_ms_per_eval          a sampling step of the engine (captured graphs, default precision schedule): --calls windows of one S-step sampling call
                           each, between device events; median (min / max beside it)
  hip_stack_ms             the stack alone per evaluation: the event pair the engine's profiling mode puts around the stack's launches (S_scan + L - 1
                           diagonal launches and the three elementwise kernels at its ends; eager launches, no graph), less the bracket's own
                           overhead; --calls windows of one S-step sampling call each, ALTERNATING with the torch windows; median (min / max)
  torch_gru_ms             torch.nn.GRU(d, d, L, batch_first=True) in fp32 with the same weights on the same input shape: --calls windows of S
                           evaluations back to back between device events; median (min / max)
  launches_per_eval        of the stack, from the engine's plan
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from regennet_amd import synth  # noqa: E402
from tests.helpers import y_to_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ntu_gru")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--respacing", default="10")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--precision", default="bf16_x3tail")
    ap.add_argument("--scans", default="batch,frames")
    a = ap.parse_args()
    B = a.batch
    cfg = synth.get_config(a.config)
    sd = synth.make_state_dict(cfg, seed=0)
    L, d, T = cfg["layers"], cfg["latent_dim"], cfg["num_frames"]
    model, diffusion = synth.build_model(cfg, sd, resp=a.respacing, precision=a.precision, device="cuda:0")
    S = diffusion.num_timesteps
    y = {"cmotion": synth.make_cmotion(cfg, B, seed=1)}
    if "action" in cfg["cond_mode"]:
        y["action"] = synth.make_actions(cfg, B, seed=2)
    y = y_to_device(y)
    shape = (B, cfg["njoints"], cfg["nfeats"], T)

    ref = torch.nn.GRU(d, d, num_layers=L, batch_first=True)
    ref.load_state_dict({k[len("gru."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("gru.")})
    ref = ref.cuda().eval()

    def call(seed):
        """One sampling call of S steps between two device events on the caller's stream (the engine joins it by events): ms per call."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, seed=seed)
        e1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return e0.elapsed_time(e1)

    for scan in a.scans.split(","):
        model.gru_scan = scan
        xs = torch.randn((T, B, d) if scan == "batch" else (B, T, d), device="cuda")     # batch_first: dim 0 are the independent sequences

        def torch_window(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                e0.record()
                for _ in range(iters):
                    out, _ = ref(xs)
                e1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            return e0.elapsed_time(e1) / iters

        call(1)                                       # warm-up: engine build, graph capture
        torch_window(2)
        eng = model._engine
        hip_w = [call(100 + i) / S for i in range(a.calls)]
        bracket = None
        stack_w, torch_w = [], []
        for i in range(a.calls):                      # the two sides alternate
            eng.profile_enable(True)
            call(200 + i)
            ms, n = eng.profile_query()["gru_stack"]
            bracket = eng.profile_bracket_overhead_ms()
            eng.profile_enable(False)
            stack_w.append((ms - n * bracket) / S)
            torch_w.append(torch_window(S))
        plan = eng.plan_query(B, split_phase=True)
        hip_eval = statistics.median(hip_w)
        print(json.dumps(dict(config=a.config, scan=scan, batch=B, steps=S, precision=a.precision, device=torch.cuda.get_device_name(0),
                              hip_ms_per_eval=hip_eval, hip_ms_per_eval_min_max=[min(hip_w), max(hip_w)], motions_per_s=B / (hip_eval * S / 1e3),
                              hip_stack_ms=statistics.median(stack_w), hip_stack_ms_min_max=[min(stack_w), max(stack_w)],
                              torch_gru_ms=statistics.median(torch_w), torch_gru_ms_min_max=[min(torch_w), max(torch_w)],
                              hip_stack_over_torch=statistics.median(stack_w) / statistics.median(torch_w), evals_per_window=S,
                              stack=plan["gru_stack"], launches_per_eval={c: v["launches_per_eval"] for c, v in plan.items()})), flush=True)


if __name__ == "__main__":
    main()
